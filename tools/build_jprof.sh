#!/bin/bash
# tools/wide_lab_jprof: tools/wide_lab with the block-Jacobi phase timers (RSVD_BJ_PROF) compiled in.
# Run after `make -C rsvd_kamaneh_raganato_terrana_amd/csrc all` (links the other objects from build/obj).
set -e
cd "$(dirname "$0")/../rsvd_kamaneh_raganato_terrana_amd/csrc"
F="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-result -DRSVD_BJ_PROF"
T=$(mktemp -d)
/opt/rocm/bin/hipcc $F -c wide_svd.hip -o $T/wide_svd.o
/opt/rocm/bin/hipcc $F -I. -c ../../tools/wide_lab.cpp -o $T/wide_lab.o
O=../../build/obj
/opt/rocm/bin/hipcc --offload-arch=gfx950 -o ../../tools/wide_lab_jprof $T/wide_lab.o $T/wide_svd.o $O/util.o $O/proj.o \
  $O/qr.o $O/jacobi.o $O/wide_proj.o $O/wide_plan.o $O/wide_gram.o $O/wide_chol.o $O/wide_panel.o $O/dense.o $O/gemm.o
rm -rf $T
