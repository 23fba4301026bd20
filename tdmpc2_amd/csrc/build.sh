#!/bin/bash
# Build the planner's C-ABI shared library for gfx950 (cross-compiles without a GPU).
# Five host units (the C ABI of include/tdmpc2_plan.h) and one translation unit per kernel family (for the fused 512-wide family,
# per action padding), compiled in parallel and linked into ONE libtdmpc2_plan.so:
#   plan_core.hip              host: error reporting, handle create / destroy (sizes: plan_layout.h), guards, allocations, fault recovery, tuning, profiling
#   plan_weights.hip           host: binds, job tables of the weight packer, refresh / soft update, packed blob
#   plan_run.hip               host: planning -- host side of the fused family, run / estimate_value / refit, sharded plans, noise export
#   plan_obs.hip               host: state and pixel encoders, policy prior (encode, run_obs, run_pix, pix_batch, pi, act_pi)
#   plan_train.hip             host: policy_value / td_target, model rollout and losses, policy loss (what they share: plan_host.h)
#   k_plan.hip                 kernels outside the families: k_refit (elite selection + refit), ks_task_bias, state encoder (k_encode / k_enc_gemv / k_enc_norm),
#                              pixel encoder's planning routes (k_pix_image / k_pix_spread / k_pix_pack), k_export_noise
#   k_fused.hip   x {16,32,48,64}   ks_setup / ks_pitraj / ks_rollout / ks_value
#   k_cluster.hip x {16,32,48,64}   ks_rollout_cl
#   k_layered.hip              layered GEMMs + row kernels + their host orchestration
#   k_policy.hip               policy prior (WorldModel.pi, act() with mpc = False): row route, GEMV, head
#   k_model.hip   x {16,32,48,64}   ks_value_roll / ks_value_chain (model rollout and losses, fused family)
#   k_model.hip                generic unit (no TU_APAD): the loss row kernels of both families
#   k_policy_loss.hip x {16,32,48,64}   ks_value_ent (update_pi's forward per row, fused family)
#   k_policy_loss.hip          generic unit: running scale, policy-loss tail, termination statistics
#   k_refresh.hip              the weight packer (every bind, refresh_weights) + target-Q soft update
#   k_pixel_batch.hip          pixel encoder, batch route: MFMA implicit-GEMM convolutions (encode_pix_batch)
#   k_buffer.hip               replay buffer: episode ring, slice draws, grouped gather, and its own C ABI (tdmpc2_buffer_*)
#   k_layer_grad.hip           trainable layer: NormedLinear forward / backward, its own C ABI (tdmpc2_layer_*)
#   k_optim.hip                optimiser step: gradient clip + Adam over flat arenas, its own C ABI (tdmpc2_optim_*); no fp contraction
#   k_loss_grad.hip            loss seeds: the four losses of _update and their gradients, its own C ABI (tdmpc2_loss_*)
#   k_pi_grad.hip              policy loss seeds: update_pi's head, value, loss and their gradients, its own C ABI and header (tdmpc2_pigrad_*, include/tdmpc2_pi_grad.h)
#   k_dropout.hip              dropout masks: Philox multipliers for the Q ensemble's first layer, its own C ABI and header (tdmpc2_dropout_*, include/tdmpc2_dropout.h)
#   k_draw.hip                 draws of a training step: Philox normals and a pair of Q heads, its own C ABI and header (tdmpc2_draw_*, include/tdmpc2_draw.h)
#   k_task.hip                 task conditioning: embedding renorm, [x | emb | a] gather and their backward, its own C ABI and header (tdmpc2_task_*, include/tdmpc2_task.h); no fp contraction
#   k_pixel_grad.hip           pixel encoder in training: a forward that keeps its activations and the convolutions' backward, its own C ABI and header (tdmpc2_pixgrad_*, include/tdmpc2_pixel_grad.h)
# Objects are cached under build/ and rebuilt when a source they include is newer (make-style), so an experiment on one
# family recompiles one file.  TDMPC2_EXTRA_FLAGS (all units), TDMPC2_FLAGS_<unit> (one unit: main = the five host units plan_*.hip, plank, fused, cluster, layered, policy, model, ploss, refresh, pixbatch, buffer, lgrad, optim, lossgrad, pigrad, dropout, draw, task, pixgrad),
# TDMPC2_ONLY_APAD=48 (experiment builds: the fused / cluster / model / policy-loss units of one padding only; reaches plan_core.hip, whose *_ops(apad) accessors then name that padding alone), TDMPC2_OUT, TDMPC2_BUILD_DIR, JOBS.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
OUT="${TDMPC2_OUT:-${HERE}/../libtdmpc2_plan.so}"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
BUILD="${TDMPC2_BUILD_DIR:-${HERE}/build}"
JOBS="${JOBS:-$(nproc)}"
mkdir -p "${BUILD}"
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function ${TDMPC2_EXTRA_FLAGS:-}"
APADS="${TDMPC2_ONLY_APAD:-16 32 48 64}"
ONLY=""
[ -n "${TDMPC2_ONLY_APAD:-}" ] && ONLY="-DTDMPC2_ONLY_APAD=${TDMPC2_ONLY_APAD}"

# unit name | source | extra flags
UNITS=()
# the host units (no kernels, no launches: everything goes through launch.h)
UNITS+=("core|plan_core.hip|${ONLY} ${TDMPC2_FLAGS_main:-}")
# plan_core.hip once more with the test hooks compiled in (TDMPC2_CLUSTER_FAULT, TDMPC2_DEBUG_NO_TURN, TDMPC2_POISON; every use of the
# macro is in that unit): libtdmpc2_plan_hooks.so is the product's objects with this one in place of core.o, and only the GPU tests
# of the fault paths load it (tdmpc2_amd/native.py)
[ -z "${TDMPC2_NO_HOOKS_LIB:-}" ] && UNITS+=("core_hooks|plan_core.hip|${ONLY} -DTDMPC2_TEST_HOOKS ${TDMPC2_FLAGS_main:-}")
UNITS+=("weights|plan_weights.hip|${TDMPC2_FLAGS_main:-}")
UNITS+=("run|plan_run.hip|${TDMPC2_FLAGS_main:-}")
UNITS+=("obs|plan_obs.hip|${TDMPC2_FLAGS_main:-}")
UNITS+=("train|plan_train.hip|${TDMPC2_FLAGS_main:-}")
UNITS+=("plank|k_plan.hip|${TDMPC2_FLAGS_plank:-}")
UNITS+=("layered|k_layered.hip|${TDMPC2_FLAGS_layered:-}")
UNITS+=("policy|k_policy.hip|${TDMPC2_FLAGS_policy:-}")
UNITS+=("model|k_model.hip|${TDMPC2_FLAGS_model:-}")
UNITS+=("ploss|k_policy_loss.hip|${TDMPC2_FLAGS_ploss:-}")
UNITS+=("refresh|k_refresh.hip|${TDMPC2_FLAGS_refresh:-}")
UNITS+=("pixbatch|k_pixel_batch.hip|${TDMPC2_FLAGS_pixbatch:-}")
UNITS+=("buffer|k_buffer.hip|${TDMPC2_FLAGS_buffer:-}")
UNITS+=("lgrad|k_layer_grad.hip|${TDMPC2_FLAGS_lgrad:-}")  # trainable layer: NormedLinear forward / backward, its own C ABI (tdmpc2_layer_*)
# optimiser step: its element math is a chain of separately rounded fp32 operations -- at -O3 hipcc fuses a * b + c into v_fma_f32
# (the _rn intrinsics included) unless contraction is off
UNITS+=("optim|k_optim.hip|-ffp-contract=off ${TDMPC2_FLAGS_optim:-}")
UNITS+=("lossgrad|k_loss_grad.hip|${TDMPC2_FLAGS_lossgrad:-}")  # loss seeds: _update's four losses and their gradients, its own C ABI (tdmpc2_loss_*)
UNITS+=("pigrad|k_pi_grad.hip|${TDMPC2_FLAGS_pigrad:-}")  # policy loss seeds: update_pi between its layers, forward and backward, its own C ABI (tdmpc2_pigrad_*)
UNITS+=("dropout|k_dropout.hip|${TDMPC2_FLAGS_dropout:-}")  # dropout masks: Philox multipliers drawn on the device, its own C ABI (tdmpc2_dropout_*)
UNITS+=("draw|k_draw.hip|${TDMPC2_FLAGS_draw:-}")  # draws of a training step: normals and a pair of Q heads drawn on the device, its own C ABI (tdmpc2_draw_*)
UNITS+=("task|k_task.hip|-ffp-contract=off ${TDMPC2_FLAGS_task:-}")  # task conditioning: renorm, gather and backward, its own C ABI (tdmpc2_task_*); the renorm is separately rounded fp32 operations
UNITS+=("pixgrad|k_pixel_grad.hip|${TDMPC2_FLAGS_pixgrad:-}")  # pixel encoder in training: stateless forward and backward, its own C ABI (tdmpc2_pixgrad_*)
for ap in ${APADS}; do
    UNITS+=("fused${ap}|k_fused.hip|-DTU_APAD=${ap} ${TDMPC2_FLAGS_fused:-}")
    UNITS+=("cluster${ap}|k_cluster.hip|-DTU_APAD=${ap} ${TDMPC2_FLAGS_cluster:-}")
    UNITS+=("model${ap}|k_model.hip|-DTU_APAD=${ap} ${TDMPC2_FLAGS_model:-}")
    UNITS+=("ploss${ap}|k_policy_loss.hip|-DTU_APAD=${ap} ${TDMPC2_FLAGS_ploss:-}")
done

compile_unit() {  # name src flags
    local name="$1" src="$2" flags="$3" obj="${BUILD}/$1.o" stamp="${BUILD}/$1.flags"
    local want="${COMMON} ${flags}"
    local need=0
    [ -f "${obj}" ] || need=1
    [ -f "${stamp}" ] && [ "$(cat "${stamp}")" == "${want}" ] || need=1
    if [ "${need}" == 0 ]; then
        for dep in "${HERE}"/*.hip "${HERE}"/*.cuh "${HERE}"/*.h "${HERE}/../../include/tdmpc2_plan.h" "${HERE}/../../include/tdmpc2_pi_grad.h" "${HERE}/../../include/tdmpc2_dropout.h" "${HERE}/../../include/tdmpc2_draw.h" "${HERE}/../../include/tdmpc2_task.h" "${HERE}/../../include/tdmpc2_pixel_grad.h"; do
            if [ "${dep}" -nt "${obj}" ] && grep -q "$(basename "${dep}")" <(unit_deps "${src}"); then need=1; break; fi
        done
    fi
    if [ "${need}" == 1 ]; then
        "${HIPCC}" ${want} -c -o "${obj}" "${HERE}/${src}"
        echo "${want}" > "${stamp}"
        echo "compiled ${name}"
    fi
}
unit_deps() {  # transitive quoted includes of a source (by name)
    local seen=" $1 " queue="$1" f inc
    while [ -n "${queue}" ]; do
        f="${queue%% *}"; queue="${queue#"${f}"}"; queue="${queue# }"
        for inc in $(grep -ho '#include "[^"]*"' "${HERE}/${f}" 2>/dev/null | sed 's/#include "\(.*\)"/\1/' | xargs -n1 basename 2>/dev/null); do
            case "${seen}" in *" ${inc} "*) ;; *) seen="${seen}${inc} "; queue="${queue} ${inc}";; esac
        done
    done
    echo "${seen}"
}
export -f compile_unit unit_deps
export HERE BUILD HIPCC COMMON

printf '%s\n' "${UNITS[@]}" | xargs -P "${JOBS}" -I{} bash -c 'IFS="|" read -r n s f <<< "{}"; compile_unit "$n" "$s" "$f"'
OBJS=(); HOBJS=()
for u in "${UNITS[@]}"; do
    n="${u%%|*}"
    [ "$n" == "core_hooks" ] && { HOBJS+=("${BUILD}/$n.o"); continue; }
    OBJS+=("${BUILD}/$n.o")
    [ "$n" != "core" ] && HOBJS+=("${BUILD}/$n.o")
done
"${HIPCC}" --offload-arch=gfx950 -shared -fPIC -o "${OUT}" "${OBJS[@]}"
echo "built ${OUT}"
if [ -z "${TDMPC2_NO_HOOKS_LIB:-}" ]; then
    "${HIPCC}" --offload-arch=gfx950 -shared -fPIC -o "${OUT%.so}_hooks.so" "${HOBJS[@]}"
    echo "built ${OUT%.so}_hooks.so"
fi
