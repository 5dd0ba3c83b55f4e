#!/bin/bash
# libsed.so variants for the stripe-parallel traceback's band map kernel: fewer staged columns left of each block
# (SED_TBMAP_LEFT, default 512) and shorter insert runs (SED_TBMAP_RUN, default 96) before an entry is left unknown
set -e
cd "$(dirname "$0")/../../rna-sequence-diff-patch_amd/csrc"
make -s OBJDIR=../../tools/ab_libs/obj_m1 OUT=../../tools/ab_libs/libsed_m1.so EXTRA="-DSED_TBMAP_LEFT=192 -DSED_TBMAP_RUN=48" ../../tools/ab_libs/libsed_m1.so
make -s OBJDIR=../../tools/ab_libs/obj_m2 OUT=../../tools/ab_libs/libsed_m2.so EXTRA="-DSED_TBMAP_RUN=48" ../../tools/ab_libs/libsed_m2.so
make -s OBJDIR=../../tools/ab_libs/obj_m3 OUT=../../tools/ab_libs/libsed_m3.so EXTRA="-DSED_TBMAP_LEFT=192" ../../tools/ab_libs/libsed_m3.so
