#!/bin/bash
# builds an alternative libcpecan_hip.so with extra -D flags into build_ab/<tag>.so (for A/B timing in ONE call on the GPU
# box: boxes differ by several % in clock, so variants are only comparable within a call).  usage: tools/ab_build.sh tag -DX=1 ...
# The recipe is the `ab` target of cpecan_amd/csrc/Makefile: the same host objects as the shipped library.
set -e
tag=$1; shift
make -C "$(dirname "$0")/../cpecan_amd/csrc" ab AB_TAG="$tag" AB_FLAGS="$*"
echo built build_ab/$tag.so
