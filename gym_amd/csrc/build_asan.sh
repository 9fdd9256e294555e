#!/usr/bin/env bash
# Builds gym_amd/_lib/asan/libmxv_asan.so: the same library with the HOST side of every translation unit under AddressSanitizer and
# UndefinedBehaviorSanitizer (SURVEY.md §5 "sanitizers": debug builds with -fsanitize=address host-side).  The device code is compiled as
# always (-fno-gpu-sanitize: GPU ASan needs xnack+ code objects, which this pool refuses); what is instrumented is the C ABI itself —
# argument validation, host staging, bookkeeping, the packed tables — which tests/c_consumer/abi_fuzz.c then drives with hostile arguments.
#   -fno-sanitize=alignment: the fuzzer hands the library MISALIGNED host structs on purpose; reading them is the caller's bug, not ours
#   -fno-sanitize=vptr,function: need RTTI / are off for C linkage anyway
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../_lib/asan"
mkdir -p "$out"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
SAN=(-fsanitize=address,undefined -fno-sanitize=alignment,vptr,function -fno-gpu-sanitize -fno-omit-frame-pointer -g)
FLAGS=(--offload-arch=gfx950 -O1 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wno-unused-result "${SAN[@]}")
srcs=(mxv_kernels.hip mxv_api.cpp mxv_norm.hip mxv_subnorm.hip mxv_tab.hip mxv_bj.hip mxv_placed.hip mxv_render.hip mxv_gae.hip mxv_policy.hip mxv_gaussian.hip mxv_policy_eval.hip mxv_ppo.hip mxv_vtrace.hip mxv_dqn.hip mxv_replay.hip mxv_prio.hip mxv_c51.hip mxv_squashed.hip mxv_nstep.hip mxv_qr.hip mxv_targets.hip mxv_sac.hip)
objs=(); pids=()
for s in "${srcs[@]}"; do
    o="$out/${s%.*}.o"; rm -f "$o"; objs+=("$o")
    "$HIPCC" "${FLAGS[@]}" -c "$here/$s" -o "$o" &
    pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
rm -f "$out/libmxv_asan.so"
"$HIPCC" --offload-arch=gfx950 -shared -fPIC "${SAN[@]}" -o "$out/libmxv_asan.so" "${objs[@]}"
rm -f "${objs[@]}"
echo "built $out/libmxv_asan.so"
