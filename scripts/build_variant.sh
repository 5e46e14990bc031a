#!/bin/bash
# build_variant.sh <out.so> [extra hipcc -D flags...]: libg4c variant with extra defines for mlp_fused.hip and mlp_run.hip (A/B tuning;
# e.g. -DG4C_TILE_FORM_DEFAULT=0, -DG4C_ABLATE=1024), linked with the other objects of the shipped build (run `make` first)
# G4C_SRC=<file in csrc/> builds the variant from another copy of the kernel source
set -e
OUT=$1; shift
cd "$(dirname "$0")/../graphs4cfd_amd/csrc"
mkdir -p build/variant
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
$HIPCC -O3 -std=c++17 -fPIC --offload-arch=gfx950 "$@" -c "${G4C_SRC:-mlp_fused.hip}" -o build/variant/mlp_fused.o
$HIPCC -O3 -std=c++17 -fPIC --offload-arch=gfx950 "$@" -c mlp_run.hip -o build/variant/mlp_run.o
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" build/variant/mlp_fused.o build/variant/mlp_run.o \
  $(ls build/*.o | grep -v -e '/mlp_fused\.o$' -e '/mlp_run\.o$')
