#!/bin/bash
# development build of the kernel library with timestamps in the sync-free triangular solves: variants/libmi355x_kernels_tritrace.so
exec bash "$(dirname "$0")/build_tri.sh" tritrace -DMI355X_TRI_TRACE
