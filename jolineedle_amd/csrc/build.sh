#!/bin/bash
# Builds libjnroll.so for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${JN_LIB_OUT:-$HERE/../lib}"
mkdir -p "$OUT" "$HERE/obj"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -Wno-unused-result ${JN_EXTRA_FLAGS:-}"
UNITS="kernels_conv kernels_pwres kernels_pwxs kernels_bwd kernels_bwd_pw kernels_train kernels_gptbwd kernels_conv3 kernels_det kernels_detloss kernels_aug kernels_env kernels_view kernels_ragged kernels_eval kernels_gpt kernels_gptwide api_ctx api_net api_det api_env api_ops api_kernels api_rollout api_train"
pids=()
for f in $UNITS; do
  if [ ! -f "$HERE/obj/$f.o" ] || [ "$HERE/$f.hip" -nt "$HERE/obj/$f.o" ] || [ -n "$(find "$HERE" -maxdepth 1 -name '*.h' -newer "$HERE/obj/$f.o")" ] || [ "$HERE/../../include/jnroll.h" -nt "$HERE/obj/$f.o" ]; then
    while [ "$(jobs -rp | wc -l)" -ge 16 ]; do wait -n; done     # at most 16 compilers at a time
    $HIPCC $FLAGS -c "$HERE/$f.hip" -o "$HERE/obj/$f.o" &
    pids+=($!)
  fi
done
$HIPCC $FLAGS -x hip -c "$HERE/plan.cpp" -o "$HERE/obj/plan.o" &
pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
objs=("$HERE/obj/plan.o")
for f in $UNITS; do objs+=("$HERE/obj/$f.o"); done
# (the listed objects only: a stale object of a removed unit left in obj/ must not be linked)
$HIPCC -shared -fPIC --offload-arch=gfx950 "${objs[@]}" -o "$OUT/libjnroll.so"
echo "built $OUT/libjnroll.so"
