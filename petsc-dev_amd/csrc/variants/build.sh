#!/bin/bash
# build a variant of the kernel library that differs in spmv_csr.hip only: build.sh NAME -DFOO=1 -DBAR=2   (development aid for A/B runs on one box)
# knobs: SPMV_NT (0/1), SPMV_REMAP (0/2), SPMV_CH, SPMV_MINWAVES, SPMV_SEQ_AVG, SPMV_VPAT_RPL, MI355X_BSR_XLDS_DEFAULT (0/1)
# every other object of the Makefile's SRCS is linked as `make` left it, so the list cannot go stale
cd "$(dirname "$0")/.." || exit 1
name=$1; shift
vary=spmv_csr
others=$(sed -n 's/^SRCS *:= *//p' Makefile | tr ' ' '\n' | sed -n 's/\.hip$/.o/p' | grep -v "^$vary\.o$")
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I../../include "$@" -c $vary.hip -o variants/${vary}_$name.o 2>/dev/null || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/libmi355x_kernels_$name.so $others variants/${vary}_$name.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
