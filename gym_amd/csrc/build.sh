#!/usr/bin/env bash
# Builds gym_amd/_lib/libmxv.so for gfx950 (cross-compiles without a GPU).
#   -ffp-contract=off : the reference rounds every operation; never fuse a*b+c into an FMA.
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../_lib"
mkdir -p "$out"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS=(--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-result ${MXV_EXTRA_FLAGS:-})
# stale objects must never survive a failed compile: remove them first, then wait for every compile BY PID
# (a bare `wait` returns 0 even when a background job failed, so `set -e` would not fire).
srcs=(mxv_kernels.hip mxv_api.cpp mxv_norm.hip mxv_subnorm.hip mxv_tab.hip mxv_bj.hip mxv_placed.hip mxv_render.hip mxv_gae.hip mxv_policy.hip mxv_gaussian.hip mxv_policy_eval.hip mxv_ppo.hip mxv_vtrace.hip mxv_dqn.hip mxv_replay.hip mxv_prio.hip mxv_c51.hip mxv_squashed.hip mxv_nstep.hip mxv_qr.hip mxv_targets.hip mxv_sac.hip)
objs=()
pids=()
for s in "${srcs[@]}"; do
    o="$out/${s%.*}.o"
    rm -f "$o"
    objs+=("$o")
    "$HIPCC" "${FLAGS[@]}" -c "$here/$s" -o "$o" &
    pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
rm -f "$out/libmxv.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$out/libmxv.so" "${objs[@]}" ${MXV_EXTRA_LIBS:-}
echo "built $out/libmxv.so"
