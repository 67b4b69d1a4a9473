#!/bin/bash
# build a variant of the kernel library that differs in spmv_tiled.hip only: build_tiled.sh NAME -DTL_TW=... -DTL_WAVES=...   (development aid for A/B runs on one box)
# every other object of the Makefile's SRCS is linked as `make` left it, so the list cannot go stale
cd "$(dirname "$0")/.." || exit 1
name=$1; shift
vary=spmv_tiled
others=$(sed -n 's/^SRCS *:= *//p' Makefile | tr ' ' '\n' | sed -n 's/\.hip$/.o/p' | grep -v "^$vary\.o$")
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -I../../include "$@" -c $vary.hip -o variants/${vary}_$name.o 2>/dev/null || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/libmi355x_kernels_$name.so $others variants/${vary}_$name.o -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
