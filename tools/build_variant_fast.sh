#!/bin/bash
# A/B build that recompiles ONLY har_kernels.hip with the extra flags and links it with the default build's other objects (mitsuba3_amd/csrc/obj, `make` first):
# tools/build_variant_fast.sh <name> <extra hipcc flags...>  -> tools/variants/lib_<name>.so   (for switches that only har_kernels.hip reads)
# Sources and flags are the Makefile's: the variant's object directory starts as a copy of obj/ without the kernels' object.
set -e
cd "$(dirname "$0")/../mitsuba3_amd/csrc"
NAME=$1; shift
mkdir -p ../../tools/variants obj_variants/$NAME
cp -p obj/*.o obj_variants/$NAME/ && rm -f obj_variants/$NAME/har_kernels.o
make OUT=../../tools/variants/lib_$NAME.so OBJDIR=obj_variants/$NAME EXTRA="$(printf '%q ' "$@")"
