#!/bin/bash
# usage: tools/ab_build_seg.sh <name> [SEGFLAGS ...]  -> vcfgl_amd/lib_ab/<name>.so = the library built from the WORKING TREE with the given options for
# vgl_sample_seg.hip alone (the k_sample_seg kernels; Makefile: SEGFLAGS); A/B timing with tools/ab_time.sh
# The options REPLACE the Makefile's SEGFLAGS, so name its scheduler strategy again where it is to stay, e.g. the pool loop of two attempts per iteration:
#   tools/ab_build_seg.sh attempts -mllvm -amdgpu-sched-strategy=iterative-minreg -DVGL_POOL_HALVES=0
# or the two half-steps without carried lanes:
#   tools/ab_build_seg.sh nocarry -mllvm -amdgpu-sched-strategy=iterative-minreg -DVGL_POOL_CARRY=0
set -eu
name=$1; shift || true
tmp=$(mktemp -d)
mkdir -p "$tmp/vcfgl_amd" "$tmp/build"
cp -r vcfgl_amd/csrc "$tmp/vcfgl_amd/csrc"; cp -r include "$tmp/include"
mkdir -p vcfgl_amd/lib_ab
( cd "$tmp/vcfgl_amd/csrc" && make -s -j8 ../lib/libvcfgl_hip.so SEGFLAGS="$*" >/dev/null 2>"$tmp/err.txt" ) || { tail -5 "$tmp/err.txt"; exit 1; }
cp "$tmp/vcfgl_amd/lib/libvcfgl_hip.so" "vcfgl_amd/lib_ab/$name.so"
rm -rf "$tmp"
ls -la "vcfgl_amd/lib_ab/$name.so"
