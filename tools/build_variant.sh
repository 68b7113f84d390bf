#!/bin/bash
# A/B builds of libhip_ad_rgb.so: tools/build_variant.sh <name> <extra hipcc flags...>  -> tools/variants/lib_<name>.so
# Sources and flags are the Makefile's; the variant's objects go to mitsuba3_amd/csrc/obj_variants/<name>/.
set -e
cd "$(dirname "$0")/../mitsuba3_amd/csrc"
NAME=$1; shift
mkdir -p ../../tools/variants
make OUT=../../tools/variants/lib_$NAME.so OBJDIR=obj_variants/$NAME EXTRA="$(printf '%q ' "$@")"
