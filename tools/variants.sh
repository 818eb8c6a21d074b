#!/bin/bash
# Build variants of the library with extra compile flags: tools/variants/<name>/liboetr_hip.so
# (csrc/Makefile's `variant` target: the shipped recipe - sources, per-file flags - plus the flags given here)
# usage: tools/variants.sh name "-DFLAG1 -DFLAG2" [name2 "flags2" ...]
set -e
cd "$(dirname "$0")/../imagematching_oetr_amd/csrc"
while [ $# -gt 0 ]; do
  make -j16 variant NAME="$1" EXTRA="$2"
  shift; [ $# -gt 0 ] && shift
done
