"""ctypes binding of the planner's C ABI (include/tdmpc2_plan.h).

The shared library `tdmpc2_amd/libtdmpc2_plan.so` is built in-tree by
`tdmpc2_amd/csrc/build.sh` (hipcc, gfx950).  There is no CPU fallback: if the
library is missing, or a planner is requested on a non-GPU device, this module
raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import torch

# TDMPC2_PLAN_LIB points profiling runs at an ablation build of the same library (tools/ablate.sh)
_LIB_PATH = os.environ.get("TDMPC2_PLAN_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libtdmpc2_plan.so")
_lib = None

ABI_VERSION = 14

NET_DYNAMICS, NET_REWARD, NET_PI, NET_Q, NET_TERMINATION, NET_TARGET_Q = range(6)
PATH_AUTO, PATH_FUSED, PATH_LAYERED = range(3)  # enum tdmpc2_path
PREC_AUTO, PREC_FP32, PREC_SPLIT_F16 = range(3)  # enum tdmpc2_precision


class FaultInfo(C.Structure):  # struct tdmpc2_fault_info
    _fields_ = [("faults_total", C.c_int32), ("rearms", C.c_int32), ("degraded", C.c_int32), ("clean_calls", C.c_int32),
                ("rearm_after", C.c_int32), ("reserved", C.c_int32), ("seconds_since_fault", C.c_double)]


class PlanCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("horizon", "num_samples", "num_elites", "num_pi_trajs", "iterations",
                                          "action_dim", "latent_dim", "mlp_dim", "task_dim", "num_bins", "num_q",
                                          "simnorm_dim")] + \
               [(n, C.c_float) for n in ("vmin", "vmax", "min_std", "max_std", "temperature", "log_std_min",
                                         "log_std_dif")] + \
               [(n, C.c_int32) for n in ("multitask", "episodic", "max_envs", "device", "path", "precision", "num_valid_samples")]


class Noise(C.Structure):
    _fields_ = [("pi_traj_eps", C.c_void_p), ("sample_eps", C.c_void_p), ("pi_eps", C.c_void_p),
                ("qidx", C.c_void_p), ("gumbel_exp", C.c_void_p), ("final_eps", C.c_void_p)]


class TaskTables(C.Structure):
    """struct tdmpc2_task_tables: one task per row of a training batch + the per-task tables."""
    _fields_ = [("task_ids", C.c_void_p), ("task_emb", C.c_void_p), ("act_mask", C.c_void_p), ("discount", C.c_void_p),
                ("n_tasks", C.c_int32)]


class ModelOut(C.Structure):
    """struct tdmpc2_model_out: optional device outputs of the model rollout."""
    _fields_ = [(n, C.c_void_p) for n in ("zs", "reward_logits", "reward", "q_logits", "q", "term_logit")]


class ModelTargets(C.Structure):
    """struct tdmpc2_model_targets: the targets and weights of TDMPC2._update's losses."""
    _fields_ = [(n, C.c_void_p) for n in ("next_z", "reward", "td_target", "terminated")] + \
               [(n, C.c_float) for n in ("rho", "consistency_coef", "reward_coef", "value_coef", "termination_coef")]


MODEL_OUTPUTS = ("zs", "reward_logits", "reward", "q_logits", "q", "term_logit")


class PolicyLossIn(C.Structure):
    """struct tdmpc2_policy_loss_in."""
    _fields_ = [("rho", C.c_float), ("entropy_coef", C.c_float), ("tau", C.c_float), ("update_scale", C.c_int32)]


POLICY_LOSS_OUTPUTS = ("action", "q", "entropy", "scaled_entropy", "step_means", "percentiles")
RUNNING_SCALE_MAX_N = 16384  # tdmpc2_plan_running_scale / the batch of a policy_loss call that updates the scale


class PolicyLossOut(C.Structure):
    """struct tdmpc2_policy_loss_out: optional device outputs of the policy loss."""
    _fields_ = [(n, C.c_void_p) for n in POLICY_LOSS_OUTPUTS]


class WeightEntry(C.Structure):
    """struct tdmpc2_weight_entry: W, b, ln_g, ln_b of one nn.Linear (+ LayerNorm) as device pointers."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "b", "ln_g", "ln_b")]


class WeightTable(C.Structure):
    """struct tdmpc2_weight_table (ABI 14): the model's parameter tensors for tdmpc2_plan_refresh_weights."""
    _fields_ = [("net", WeightEntry * 3 * 6), ("enc", WeightEntry * 6), ("enc_layers", C.c_int32),
                ("enc_out", C.c_int32 * 6), ("enc_in", C.c_int32 * 6)]


NET_PREFIX = {NET_DYNAMICS: "_dynamics", NET_REWARD: "_reward", NET_PI: "_pi", NET_Q: "_Qs.params",
              NET_TERMINATION: "_termination", NET_TARGET_Q: "_target_Qs_params"}
WEIGHT_FIELDS = (("W", "weight"), ("b", "bias"), ("ln_g", "ln.weight"), ("ln_b", "ln.bias"))


class PolicyOut(C.Structure):
    """struct tdmpc2_policy_out: device pointers, all but `action` optional."""
    _fields_ = [("action", C.c_void_p), ("mean", C.c_void_p), ("log_std", C.c_void_p), ("entropy", C.c_void_p),
                ("scaled_entropy", C.c_void_p), ("eps_out", C.c_void_p)]


POLICY_ROUTE_AUTO, POLICY_ROUTE_ROW, POLICY_ROUTE_SPREAD = range(3)  # TDMPC2_TUNE_POLICY_ROUTE values
TUNE_POLICY_ROUTE = 9


BUFFER_MAX_FIELDS = 8


class BufferField(C.Structure):  # struct tdmpc2_buffer_field
    _fields_ = [("row_bytes", C.c_uint32), ("step_first", C.c_int32), ("step_count", C.c_int32)]


class BufferCfg(C.Structure):  # struct tdmpc2_buffer_cfg
    _fields_ = [("capacity", C.c_uint64), ("slice_len", C.c_int32), ("device", C.c_int32), ("n_fields", C.c_int32),
                ("max_batch", C.c_int32), ("field", BufferField * BUFFER_MAX_FIELDS)]


class BufferInfo(C.Structure):  # struct tdmpc2_buffer_info
    _fields_ = [("num_eps", C.c_uint64), ("live_steps", C.c_uint64), ("cursor", C.c_uint64), ("eligible", C.c_uint32),
                ("next_call", C.c_uint32)]


LAYER_LINEAR, LAYER_MISH, LAYER_SIMNORM = range(3)  # enum TDMPC2_LAYER_*


class LayerDesc(C.Structure):  # struct tdmpc2_layer_desc
    _fields_ = [(n, C.c_int32) for n in ("kind", "groups", "rows", "in_dim", "out_dim", "shared_x", "simnorm_dim")] + \
               [("ln_eps", C.c_float)]


class OptimSeg(C.Structure):  # struct tdmpc2_optim_seg
    _fields_ = [("param", C.c_void_p), ("count", C.c_int64), ("group", C.c_int32), ("reserved", C.c_int32)]


class OptimCfg(C.Structure):  # struct tdmpc2_optim_cfg
    _fields_ = [("device", C.c_int32), ("n_segs", C.c_int32), ("n_groups", C.c_int32), ("reserved", C.c_int32),
                ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float),
                ("lr", C.POINTER(C.c_float)), ("segs", C.POINTER(OptimSeg))]


class LossDesc(C.Structure):  # struct tdmpc2_loss_desc
    _fields_ = [(n, C.c_int32) for n in ("steps", "batch", "latent_dim", "num_q", "num_bins", "episodic")] + \
               [(n, C.c_float) for n in ("vmin", "vmax", "bin_size", "rho", "consistency_coef", "reward_coef", "value_coef",
                                         "termination_coef")]


class PiGradDesc(C.Structure):  # struct tdmpc2_pigrad_desc (include/tdmpc2_pi_grad.h)
    _fields_ = [(n, C.c_int32) for n in ("steps", "batch", "action_dim", "num_bins", "multitask")] + \
               [(n, C.c_float) for n in ("vmin", "vmax", "rho", "entropy_coef", "log_std_min", "log_std_dif")]


class DropoutDesc(C.Structure):  # struct tdmpc2_dropout_desc (include/tdmpc2_dropout.h)
    _fields_ = [("n", C.c_int64), ("p", C.c_float), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("call_lo", C.c_uint32),
                ("call_hi", C.c_uint32), ("reserved", C.c_uint32)]


class DrawDesc(C.Structure):  # struct tdmpc2_draw_desc (include/tdmpc2_draw.h)
    _fields_ = [("n", C.c_int64), ("num_q", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("call_lo", C.c_uint32),
                ("call_hi", C.c_uint32), ("reserved", C.c_uint32)]


class TaskDesc(C.Structure):  # struct tdmpc2_task_desc (include/tdmpc2_task.h)
    _fields_ = [(n, C.c_int32) for n in ("steps", "batch", "ids_len", "id_bytes", "num_tasks", "x_dim", "task_dim", "a_dim")] + \
               [("max_norm", C.c_float), ("reserved", C.c_uint32)]


class PixGradDesc(C.Structure):  # struct tdmpc2_pixgrad_desc (include/tdmpc2_pixel_grad.h)
    _fields_ = [(n, C.c_int32) for n in ("n", "cin", "C", "obs_dtype", "seed_is_preact")] + [("reserved", C.c_uint32)]


class Debug(C.Structure):
    _fields_ = [("value", C.c_void_p), ("elite_idx", C.c_void_p), ("score", C.c_void_p), ("mean", C.c_void_p),
                ("std", C.c_void_p), ("actions", C.c_void_p)]


# The prototypes, one ordered table per header: name -> argtypes (restype int), or (argtypes, restype) where it is not int.
# _open declares them all; tests/test_abi_prototypes.py counts each entry against its declaration.
_P, _vp, _i32, _u32, _u64, _f32, _sz = C.POINTER, C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t
_bind = [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp]
_PLAN_H = {  # include/tdmpc2_plan.h
    "tdmpc2_plan_abi_version": [],
    "tdmpc2_last_error": ([], C.c_char_p),
    "tdmpc2_plan_create": [_P(PlanCfg), _P(_vp)],
    "tdmpc2_plan_destroy": ([_vp], None),
    "tdmpc2_plan_device_bytes": ([_vp], _u64),
    "tdmpc2_plan_path": [_vp],
    "tdmpc2_plan_precision": [_vp],
    "tdmpc2_plan_bind_weights": _bind,
    "tdmpc2_plan_run": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _P(Noise), _u64, _vp, _P(Debug), _vp],
    "tdmpc2_plan_estimate_value": [_vp, _i32] + [_vp] * 9,
    "tdmpc2_plan_estimate_value_trace": [_vp, _i32] + [_vp] * 11,
    "tdmpc2_plan_refit": [_vp, _i32] + [_vp] * 8,
    "tdmpc2_plan_set_tuning": [_vp, _i32, _i32],
    "tdmpc2_plan_set_profiling": [_vp, _i32],
    "tdmpc2_plan_profile_read": [_vp, _P(_f32), _P(_i32)],
    "tdmpc2_plan_bind_encoder": _bind,
    "tdmpc2_plan_encode": [_vp, _i32, _vp, _i32, _vp, _vp, _vp],
    "tdmpc2_plan_run_obs": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _P(Noise), _u64, _vp, _vp],
    "tdmpc2_plan_policy_value": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp],
    "tdmpc2_plan_td_target": [_vp, _i32, _vp, _vp, _vp, _f32, _vp, _vp, _u64, _vp, _vp],
    "tdmpc2_plan_policy_value_mt": [_vp, _i32, _vp, _P(TaskTables), _i32, _i32, _vp, _vp, _u64, _vp, _vp, _vp],
    "tdmpc2_plan_td_target_mt": [_vp, _i32, _vp, _vp, _vp, _f32, _P(TaskTables), _vp, _vp, _u64, _vp, _vp],
    "tdmpc2_plan_packed_size": [_vp, _P(_u64)],
    "tdmpc2_plan_export_packed": [_vp, _vp, _u64, _vp],
    "tdmpc2_plan_import_packed": [_vp, _vp, _u64, _vp],
    "tdmpc2_plan_shard_begin": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _P(Noise), _u64, _vp],
    "tdmpc2_plan_shard_values": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _P(Noise), _u64, _vp, _vp],
    "tdmpc2_plan_shard_refit": [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _P(Noise), _u64, _vp, _P(Debug), _vp],
    "tdmpc2_plan_export_noise": [_vp, _i32, _i32, _u64, _u32, _P(Noise), _vp],
    "tdmpc2_plan_call_counter": [_vp, _P(_u32)],
    "tdmpc2_plan_set_call_counter": [_vp, _u32],
    "tdmpc2_plan_take_fault": [_vp, _P(_i32)],
    "tdmpc2_plan_fault_info": [_vp, _P(FaultInfo)],
    "tdmpc2_plan_fault_word": [_vp, _vp, _vp],
    "tdmpc2_plan_bind_pixel_encoder": [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp],
    "tdmpc2_plan_encode_pix": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp],
    "tdmpc2_plan_run_pix": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _P(Noise), _u64, _vp, _vp],
    "tdmpc2_plan_bind_policy": [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp],
    "tdmpc2_plan_pi": [_vp, _i32, _vp, _vp, _vp, _vp, _u64, _P(PolicyOut), _vp],
    "tdmpc2_plan_act_pi": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _u64, _P(PolicyOut), _vp],
    "tdmpc2_plan_act_pi_pix": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _u64, _P(PolicyOut), _vp],
    "tdmpc2_plan_model_rollout": [_vp, _i32, _i32, _vp, _vp, _i32, _P(ModelOut), _vp],
    "tdmpc2_plan_model_rollout_mt": [_vp, _i32, _i32, _vp, _vp, _P(TaskTables), _i32, _P(ModelOut), _vp],
    "tdmpc2_plan_model_losses": [_vp, _i32, _i32, _vp, _vp, _i32, _P(ModelTargets), _P(ModelOut), _vp, _vp, _vp],
    "tdmpc2_plan_model_losses_mt": [_vp, _i32, _i32, _vp, _vp, _P(TaskTables), _i32, _P(ModelTargets), _P(ModelOut), _vp, _vp, _vp],
    "tdmpc2_plan_policy_loss": [_vp, _i32, _i32, _vp, _vp, _vp, _u64, _P(PolicyLossIn), _vp, _P(PolicyLossOut), _vp, _vp],
    "tdmpc2_plan_policy_loss_mt": [_vp, _i32, _i32, _vp, _P(TaskTables), _vp, _vp, _u64, _P(PolicyLossIn), _vp, _P(PolicyLossOut), _vp,
                                   _vp],
    "tdmpc2_plan_running_scale": [_vp, _i32, _vp, _f32, _vp, _vp, _vp],
    "tdmpc2_plan_termination_stats": [_vp, _i32, _vp, _vp, _vp, _vp],
    "tdmpc2_plan_refresh_weights": [_vp, _P(WeightTable), _vp],
    "tdmpc2_plan_soft_update_target": [_vp, _P(WeightTable), _P(_vp * 4), _f32, _vp],
    "tdmpc2_plan_pix_batch_reserve": [_vp, _i32, _vp],
    "tdmpc2_plan_encode_pix_batch": [_vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp],
    "tdmpc2_buffer_create": [_P(BufferCfg), _P(_vp)],
    "tdmpc2_buffer_destroy": ([_vp], None),
    "tdmpc2_buffer_add": [_vp, _u32, _P(_vp), _vp],
    "tdmpc2_buffer_load": [_vp, _u64, _u32, _P(_vp), _vp],
    "tdmpc2_buffer_sample": [_vp, _i32, _P(_vp), _vp, _u64, _vp],
    "tdmpc2_buffer_stats": [_vp, _P(BufferInfo), _vp],
    "tdmpc2_buffer_set_call_counter": [_vp, _u32, _vp],
    "tdmpc2_layer_workspace_bytes": [_P(LayerDesc), _P(_sz)],
    "tdmpc2_layer_forward": [_P(LayerDesc)] + [_vp] * 10,
    "tdmpc2_layer_backward": [_P(LayerDesc)] + [_vp] * 14 + [_sz, _vp],
    "tdmpc2_optim_layout": [_P(OptimCfg), _P(C.c_int64), _P(C.c_int64)],
    "tdmpc2_optim_create": [_P(OptimCfg), _P(_vp)],
    "tdmpc2_optim_destroy": ([_vp], None),
    "tdmpc2_optim_step": [_vp, _vp, _vp, _vp, _i32, _vp, _vp],
    "tdmpc2_optim_get_step": [_vp, _P(C.c_int64), _vp],
    "tdmpc2_optim_set_step": [_vp, C.c_int64, _vp],
    "tdmpc2_loss_workspace_bytes": [_P(LossDesc), _P(_sz)],
    "tdmpc2_loss_forward": [_P(LossDesc)] + [_vp] * 11 + [_sz, _vp],
    "tdmpc2_loss_backward": [_P(LossDesc)] + [_vp] * 14,
}
# include/tdmpc2_pi_grad.h: the policy-loss unit, a header of its own beside ABI 14 (whose version and symbols stay as they are);
# the pointers after the descriptor, the stream included
_PI_GRAD_H = {"tdmpc2_pigrad_" + name: [_P(PiGradDesc)] + [_vp] * nptr for name, nptr in
              (("head_forward", 7), ("head_backward", 7), ("value_forward", 3), ("loss_forward", 7), ("loss_backward", 6))}
# include/tdmpc2_dropout.h: the dropout-mask unit, again a header of its own beside ABI 14
_DROPOUT_H = {"tdmpc2_dropout_mask": [_P(DropoutDesc), _vp, _vp, _vp]}
# include/tdmpc2_draw.h: the draw unit (normals and a pair of Q heads), a header of its own as well
_DRAW_H = {"tdmpc2_draw_noise": [_P(DrawDesc), _vp, _vp, _vp, _vp]}
# include/tdmpc2_task.h: the task unit (embedding renorm, the [x | emb | a] gather and their backward), a header of its own too
_TASK_H = {"tdmpc2_task_forward": [_P(TaskDesc)] + [_vp] * 6, "tdmpc2_task_backward": [_P(TaskDesc)] + [_vp] * 6,
           "tdmpc2_task_renorm": [_P(TaskDesc)] + [_vp] * 3}
# include/tdmpc2_pixel_grad.h: the pixel encoder in training (a forward that keeps its activations, the convolutions' backward)
_PIXEL_GRAD_H = {"tdmpc2_pixgrad_workspace_bytes": [_P(PixGradDesc), _P(_sz), _P(_sz), _P(_sz)],
                 "tdmpc2_pixgrad_shift_table": [_vp],
                 "tdmpc2_pixgrad_forward": [_P(PixGradDesc)] + [_vp] * 8, "tdmpc2_pixgrad_backward": [_P(PixGradDesc)] + [_vp] * 10}
PROTOTYPES = {"tdmpc2_plan.h": _PLAN_H, "tdmpc2_pi_grad.h": _PI_GRAD_H, "tdmpc2_dropout.h": _DROPOUT_H,
              "tdmpc2_draw.h": _DRAW_H, "tdmpc2_task.h": _TASK_H, "tdmpc2_pixel_grad.h": _PIXEL_GRAD_H}  # by header under include/
ABI_SYMBOLS = list(_PLAN_H)  # every symbol include/tdmpc2_plan.h declares (tests check the .so exports all of them)
PI_GRAD_SYMBOLS = tuple(_PI_GRAD_H)
DROPOUT_SYMBOLS = tuple(_DROPOUT_H)
DRAW_SYMBOLS = tuple(_DRAW_H)
TASK_SYMBOLS = tuple(_TASK_H)
PIXEL_GRAD_SYMBOLS = tuple(_PIXEL_GRAD_H)


def signature(sig):
    """(argtypes, restype) of a PROTOTYPES entry."""
    return sig if isinstance(sig, tuple) else (sig, C.c_int)


class NativeError(RuntimeError):
    pass


def lib_path() -> str:
    return _LIB_PATH


# Environment variables that are TEST HOOKS of the bounded-wait / stream-order machinery.  The shipped library does not read them
# (ABI 9); `libtdmpc2_plan_hooks.so` -- the same objects with the C-ABI unit compiled -DTDMPC2_TEST_HOOKS, built beside the product
# library -- does, and a planner created while one of them is set is created on that library (the GPU tests of the fault paths).
TEST_HOOK_ENVS = ("TDMPC2_CLUSTER_FAULT", "TDMPC2_DEBUG_NO_TURN", "TDMPC2_POISON")
_HOOKS_LIB_PATH = os.path.join(os.path.dirname(_LIB_PATH), "libtdmpc2_plan_hooks.so")
_lib_hooks = None


def hooks_lib_path() -> str:
    return _HOOKS_LIB_PATH


def load_library(hooks: bool = False):
    """dlopen the planner library (hooks = True: its test-hooks flavour) and declare its prototypes.  Raises if absent."""
    global _lib, _lib_hooks
    if hooks and "TDMPC2_PLAN_LIB" not in os.environ:
        if _lib_hooks is None:
            _lib_hooks = _open(_HOOKS_LIB_PATH)
        return _lib_hooks
    if _lib is None:
        _lib = _open(_LIB_PATH)
    return _lib


def _open(path):
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: build it with tdmpc2_amd/csrc/build.sh "
                          "(or __graft_entry__.build()); there is no CPU fallback for the planner")
    lib = C.CDLL(path)
    for table in PROTOTYPES.values():
        for name, sig in table.items():
            fn = getattr(lib, name)
            fn.argtypes, fn.restype = signature(sig)
    if lib.tdmpc2_plan_abi_version() != ABI_VERSION:
        raise NativeError(f"ABI version mismatch: library {lib.tdmpc2_plan_abi_version()}, binding {ABI_VERSION}")
    return lib


# include/tdmpc2_plan.h: enum tdmpc2_expert_knob, in order.  TDMPC2_X_<NAME> in the environment OF THE PYTHON PROCESS is applied to every
# planner at creation (the A/B tools: tools/gpu_env_ab.sh); the library itself reads none of these.
EXPERT_KNOBS = ("GEMM_W256_MIN", "GEMM_W_SPLIT_MIN", "GEMM_W_SPLIT_MAX", "GEMM_W_SPLIT_OVH", "KSPLIT_AUTO_LO", "KSPLIT_AUTO_MIN",
                "GEMM_W_XCD_ROWS", "GEMM_NCT1", "GEMM_WIDE_MIN", "GEMM_RT4", "GEMM_FILL_PERMILLE", "GEMM_FILL_HEAD_PERMILLE", "GEMM_SD1",
                "GEMM_XCD_ROWS", "GEMM_COL_PAD", "TWOHOT_UNFUSED", "Z0_SHARED_OFF", "MID_PARTS_MAX", "MID_FUSE_LN", "MID_SPLIT_XCD", "MID_PIFOLD")
TUNE_EXPERT = 100


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk_tensor(name, t, dtype, shape, device):
    if t.device != device:
        raise ValueError(f"{name}: expected device {device}, got {t.device}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def plan_cfg(cfg, iterations: int, max_envs: int = 1, device_index: int = 0, path: int = PATH_AUTO, precision: int = PREC_AUTO,
             log_std_min: Optional[float] = None, log_std_dif: Optional[float] = None) -> PlanCfg:
    """struct tdmpc2_plan_cfg of a handle for `max_envs` plans of `cfg`, as NativePlanner creates it."""
    lsmin = float(cfg.log_std_min) if log_std_min is None else float(log_std_min)
    lsdif = float(cfg.log_std_max) - float(cfg.log_std_min) if log_std_dif is None else float(log_std_dif)
    # cfg.num_samples may be anything (config.yaml:36); the kernels own 64- / 128-row tiles.  The handle is created with the
    # count rounded UP to the tile and told the true one (tdmpc2_plan_cfg::num_valid_samples): the padding rows are rolled out but
    # can never be elites.
    n_true = int(cfg.num_samples)
    # the family create will choose: the rule's home is plan_layout (tdmpc2_amd/csrc/plan_layout.h); repeated here only to round
    # num_samples before create sees it (asking create instead needs an ABI call)
    fused_ok = int(cfg.latent_dim) == 512 and int(cfg.mlp_dim) == 512 and int(path) != PATH_LAYERED
    tile = 64 if fused_ok else 128  # rows a workgroup owns: fused family 64, layered family 128
    npad = (n_true + tile - 1) // tile * tile
    return PlanCfg(horizon=cfg.horizon, num_samples=npad, num_valid_samples=(n_true if npad != n_true else 0),
                   num_elites=cfg.num_elites,
                   num_pi_trajs=cfg.num_pi_trajs, iterations=int(iterations), action_dim=cfg.action_dim,
                   latent_dim=cfg.latent_dim, mlp_dim=cfg.mlp_dim, task_dim=cfg.task_dim, num_bins=cfg.num_bins,
                   num_q=cfg.num_q, simnorm_dim=cfg.simnorm_dim, vmin=cfg.vmin, vmax=cfg.vmax, min_std=cfg.min_std,
                   max_std=cfg.max_std, temperature=cfg.temperature, log_std_min=lsmin, log_std_dif=lsdif,
                   multitask=int(bool(cfg.multitask)), episodic=int(bool(cfg.episodic)), max_envs=int(max_envs),
                   device=device_index, path=int(path), precision=int(precision))


class NativePlanner:
    """Owns one `tdmpc2_plan_t` handle on one GPU.

    Mirrors what the reference keeps as planner state in `TDMPC2.__init__`
    (tdmpc2/tdmpc2.py:17-43): the world-model weights (re-packed on the device)
    and the workspace for `max_envs` concurrent plans.
    """

    def __init__(self, cfg, iterations: int, device: torch.device, max_envs: int = 1,
                 log_std_min: Optional[float] = None, log_std_dif: Optional[float] = None, path: int = PATH_AUTO,
                 precision: int = PREC_AUTO):
        device = torch.device(device)
        if device.type != "cuda":
            raise NativeError(f"the planner runs on an MI355X only (device {device}); there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load_library(hooks=any(k in os.environ for k in TEST_HOOK_ENVS))
        self.cfg = cfg
        self.device = device
        self.iterations = int(iterations)
        self.max_envs = int(max_envs)
        # self.cfg keeps the caller's num_samples; tapes are padded and stages sliced at the handle's (plan_cfg)
        c = plan_cfg(cfg, self.iterations, self.max_envs, device.index, path, precision, log_std_min, log_std_dif)
        self._npad = int(c.num_samples)
        h = C.c_void_p()
        with torch.cuda.device(device):  # the library restores the caller's device itself; this keeps torch's view in step
            self._check(self.lib.tdmpc2_plan_create(C.byref(c), C.byref(h)))
        self._h = h
        self.path = int(self.lib.tdmpc2_plan_path(h))  # PATH_FUSED or PATH_LAYERED
        self.precision = int(self.lib.tdmpc2_plan_precision(h))  # PREC_FP32 or PREC_SPLIT_F16
        for name in EXPERT_KNOBS:  # measurement knobs from THIS process's environment (see EXPERT_KNOBS)
            if f"TDMPC2_X_{name}" in os.environ:
                self.set_expert(name, int(os.environ[f"TDMPC2_X_{name}"]))
        self._seed_calls = 0
        self._shard_noise = None  # struct tdmpc2_noise of the sharded plan in progress (shard_begin .. shard_refit)
        self.encoder_layers = 0
        self.obs_dim = None
        self.policy_bound = False
        self.pix_batch_chunk = 0  # images per pass that reserve_pix_batch has sized the batch route's workspace for (0: nothing reserved)

    # ------------------------------------------------------------------ plumbing
    def _check(self, rc: int):
        if rc != 0:
            raise NativeError(f"tdmpc2_plan error {rc}: {self.lib.tdmpc2_last_error().decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.tdmpc2_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self) -> int:
        return int(self.lib.tdmpc2_plan_device_bytes(self._h))

    # ------------------------------------------------------------------ weights
    def bind_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Bind planner weights from a state dict in the reference's (new-format)
        checkpoint key layout: `_dynamics.{i}.*`, `_reward.{i}.*`, `_pi.{i}.*`,
        `_Qs.params.{i}.*` (stacked over num_q).  tdmpc2/common/layers.py:167-199."""
        nets = [(NET_DYNAMICS, "_dynamics"), (NET_REWARD, "_reward"), (NET_PI, "_pi"), (NET_Q, "_Qs.params")]
        if self.cfg.episodic:
            nets.append((NET_TERMINATION, "_termination"))
        if "_target_Qs_params.0.weight" in sd:
            nets.append((NET_TARGET_Q, "_target_Qs_params"))  # optional: td_target (tdmpc2.py:239-254)
        keep = []
        with torch.cuda.device(self.device):
            for net, prefix in nets:
                for layer in range(3):
                    def get(name, required=True):
                        k = f"{prefix}.{layer}.{name}"
                        if k not in sd:
                            if required:
                                raise KeyError(f"state dict lacks {k}")
                            return None
                        t = sd[k].detach().to(self.device, torch.float32).contiguous()
                        keep.append(t)
                        return t
                    W, b = get("weight"), get("bias")
                    g, beta = get("ln.weight", False), get("ln.bias", False)
                    out_f, in_f = int(W.shape[-2]), int(W.shape[-1])
                    self._check(self.lib.tdmpc2_plan_bind_weights(self._h, net, layer, _ptr(W), _ptr(b), _ptr(g),
                                                                  _ptr(beta), out_f, in_f, self._stream()))
            torch.cuda.current_stream(self.device).synchronize()  # sources may now be freed

    # ------------------------------------------------------------------ weight refresh (ABI 14)
    def _src(self, key, t, shape):
        """Pointer of a tensor the library reads IN PLACE: it must already be what the kernels take (no copy is made)."""
        if not torch.is_tensor(t) or t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise NativeError(f"{key}: the refresh reads the tensor itself -- it must be a contiguous float32 tensor on {self.device}")
        if tuple(t.shape) != tuple(shape):
            raise NativeError(f"{key}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.data_ptr()

    def _net_shapes(self, net, layer):
        """Shapes of `_<net>.{layer}.{weight,bias,ln.weight,ln.bias}` as the handle's cfg gives them (ln entries None without LayerNorm)."""
        c = self.cfg
        is_q = net in (NET_Q, NET_TARGET_Q)
        takes_action = net in (NET_DYNAMICS, NET_REWARD) or is_q
        if layer == 0:
            fin, fout = c.latent_dim + c.task_dim + (c.action_dim if takes_action else 0), c.mlp_dim
        else:
            fin = c.mlp_dim
            fout = c.mlp_dim if layer == 1 else (c.latent_dim if net == NET_DYNAMICS else 2 * c.action_dim if net == NET_PI
                                                 else 1 if net == NET_TERMINATION else max(int(c.num_bins), 1))
        lead = (int(c.num_q),) if is_q else ()
        ln = layer < 2 or net == NET_DYNAMICS
        vec = lead + (fout,)
        return {"weight": lead + (fout, fin), "bias": vec, "ln.weight": vec if ln else None, "ln.bias": vec if ln else None}

    def weight_table(self, sd: Dict[str, torch.Tensor], nets=None, encoder_prefix: str = "_encoder.state") -> WeightTable:
        """struct tdmpc2_weight_table over the tensors of `sd` themselves (checkpoint keys, as `bind_state_dict` / `bind_encoder`
        read them).  `nets`: the NET_* to name (default: every net whose `.0.weight` is in `sd`); the state encoder is named when
        its keys are in `sd`.  NativeError if a tensor is not fp32, not contiguous, not on the handle's device or of another shape."""
        tab = WeightTable()
        for net, prefix in NET_PREFIX.items():
            if (net not in nets) if nets is not None else (f"{prefix}.0.weight" not in sd):
                continue
            for layer in range(3):
                shapes = self._net_shapes(net, layer)
                for field, name in WEIGHT_FIELDS:
                    k = f"{prefix}.{layer}.{name}"
                    if shapes[name] is None:
                        continue
                    if k not in sd:
                        raise KeyError(f"state dict lacks {k}")
                    setattr(tab.net[net][layer], field, self._src(k, sd[k], shapes[name]))
        n = 0
        while nets is None and f"{encoder_prefix}.{n}.weight" in sd:
            n += 1
        if n > 6:
            raise NativeError(f"state encoder of {n} layers (at most 6)")
        for layer in range(n):
            W = sd[f"{encoder_prefix}.{layer}.weight"]
            fout, fin = int(W.shape[0]), int(W.shape[1])
            for field, name in WEIGHT_FIELDS:
                k = f"{encoder_prefix}.{layer}.{name}"
                setattr(tab.enc[layer], field, self._src(k, sd[k], (fout, fin) if field == "W" else (fout,)))
            tab.enc_out[layer], tab.enc_in[layer] = fout, fin
        tab.enc_layers = n
        return tab

    def refresh_state_dict(self, sd: Dict[str, torch.Tensor], nets=None):
        """Re-pack the planner's weights from the tensors of `sd` THEMSELVES in at most four launches (tdmpc2_plan_refresh_weights):
        what `bind_state_dict` + `bind_encoder` (+ `bind_policy` when the policy prior is bound) produce, without copies, without
        a stream synchronisation, capturable.  The tensors are read when the launches run: keep them alive and unchanged until
        the stream has passed the call (a training loop's parameters are both)."""
        tab = self.weight_table(sd, nets)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_refresh_weights(self._h, C.byref(tab), self._stream()))
        if tab.enc_layers:
            self.encoder_layers = int(tab.enc_layers)
            self.obs_dim = int(tab.enc_in[0]) - int(self.cfg.task_dim)

    def soft_update_target(self, sd: Dict[str, torch.Tensor], tau: float):
        """WorldModel.soft_update_target_Q (world_model.py:82-86): `_target_Qs_params.*` of `sd` are lerped IN PLACE towards
        `_Qs.params.*` with weight `tau` and the target ensemble is re-packed from the result (tdmpc2_plan_soft_update_target)."""
        tab = self.weight_table(sd, nets=(NET_Q,))
        tgt = (C.c_void_p * 4 * 3)()
        for layer in range(3):
            shapes = self._net_shapes(NET_TARGET_Q, layer)
            for i, (_, name) in enumerate(WEIGHT_FIELDS):
                if shapes[name] is None:
                    continue
                k = f"_target_Qs_params.{layer}.{name}"
                if k not in sd:
                    raise KeyError(f"state dict lacks {k}")
                tgt[layer][i] = self._src(k, sd[k], shapes[name])
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_soft_update_target(self._h, C.byref(tab), tgt, C.c_float(float(tau)), self._stream()))

    def bind_encoder(self, sd: Dict[str, torch.Tensor], prefix: str = "_encoder.state"):
        """Bind the state encoder (tdmpc2/common/layers.py:153-164) from checkpoint keys
        `_encoder.state.{i}.{weight,bias,ln.weight,ln.bias}`; afterwards `encode` / `plan_obs` run it in HIP."""
        n = 0
        while f"{prefix}.{n}.weight" in sd:
            n += 1
        if n == 0:
            raise KeyError(f"state dict has no {prefix}.0.weight")
        keep = []
        with torch.cuda.device(self.device):
            for layer in range(n):
                ts = []
                for name in ("weight", "bias", "ln.weight", "ln.bias"):
                    t = sd[f"{prefix}.{layer}.{name}"].detach().to(self.device, torch.float32).contiguous()
                    keep.append(t)
                    ts.append(t)
                W = ts[0]
                self._check(self.lib.tdmpc2_plan_bind_encoder(self._h, layer, n, _ptr(W), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]),
                                                              int(W.shape[0]), int(W.shape[1]), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()
        self.encoder_layers = n
        self.obs_dim = int(sd[f"{prefix}.0.weight"].shape[1]) - int(self.cfg.task_dim)

    def encode(self, obs, task_emb=None, out: Optional[torch.Tensor] = None):
        """WorldModel.encode for state observations (world_model.py:103-112): obs [E, obs_dim] -> z [E, L]."""
        cfg, dev = self.cfg, self.device
        E = int(obs.shape[0])
        _chk_tensor("obs", obs, torch.float32, (E, self.obs_dim), dev)
        if cfg.multitask:
            if task_emb is None:
                raise ValueError("multitask encoding needs task_emb")
            _chk_tensor("task_emb", task_emb, torch.float32, (E, cfg.task_dim), dev)
        else:
            task_emb = None
        z = out if out is not None else torch.empty(E, cfg.latent_dim, device=dev, dtype=torch.float32)
        _chk_tensor("z", z, torch.float32, (E, cfg.latent_dim), dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_encode(self._h, E, _ptr(obs), self.obs_dim, _ptr(task_emb), _ptr(z), self._stream()))
        return z

    def plan_obs(self, obs, disc_pow, prev_mean, t0, eval_mode=False, task_emb=None, act_mask=None,
                 tape: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0, out: Optional[torch.Tensor] = None):
        """TDMPC2._plan from the observation on (tdmpc2.py:152-206): encode + plan in one library call."""
        cfg, dev = self.cfg, self.device
        E = int(obs.shape[0])
        H, N, K, P, A, I = cfg.horizon, cfg.num_samples, cfg.num_elites, cfg.num_pi_trajs, cfg.action_dim, self.iterations
        _chk_tensor("obs", obs, torch.float32, (E, self.obs_dim), dev)
        _chk_tensor("disc_pow", disc_pow, torch.float32, (E, H + 1), dev)
        if cfg.multitask:
            if task_emb is None or act_mask is None:
                raise ValueError("multitask planning needs task_emb and act_mask")
            _chk_tensor("task_emb", task_emb, torch.float32, (E, cfg.task_dim), dev)
            _chk_tensor("act_mask", act_mask, torch.float32, (E, A), dev)
        _chk_tensor("prev_mean", prev_mean, torch.float32, (E, H, A), dev)
        _chk_tensor("t0", t0, torch.uint8, (E,), dev)
        action = out if out is not None else torch.empty(E, A, device=dev, dtype=torch.float32)
        _chk_tensor("action", action, torch.float32, (E, A), dev)
        noise_p = None
        if tape is not None:
            noise = self._noise(tape, E)
            noise_p = C.byref(noise)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_run_obs(self._h, E, _ptr(obs), self.obs_dim, _ptr(task_emb), _ptr(act_mask),
                                                     _ptr(disc_pow), _ptr(prev_mean), _ptr(t0), int(bool(eval_mode)), noise_p,
                                                     C.c_uint64(int(seed) & (2**64 - 1)), _ptr(action), self._stream()))
        return action

    # ------------------------------------------------------------------ pixel observations (ABI 10)
    @staticmethod
    def draw_shift(E: int, device) -> torch.Tensor:
        """ShiftAug's draw (tdmpc2/common/layers.py:52, tdmpc2_amd.layers.ShiftAug): the same torch.randint call, so the
        generator advances exactly as the reference's encoder advances it; returned as int32 [E, 2] = (dx, dy)."""
        s = torch.randint(0, 7, size=(int(E), 1, 1, 2), device=device, dtype=torch.float32)
        return s.view(int(E), 2).to(torch.int32)

    def bind_pixel_encoder(self, sd: Dict[str, torch.Tensor], prefix: str = "_encoder.rgb"):
        """Bind the pixel encoder (tdmpc2/common/layers.py:136-150) from checkpoint keys `_encoder.rgb.{2,4,6,8}.{weight,bias}`;
        afterwards `encode_pix` / `plan_pix` run it in HIP.  Not part of the packed blob: bind again after `import_packed`."""
        with torch.cuda.device(self.device):
            keep = []
            for layer, idx in enumerate((2, 4, 6, 8)):
                W = sd[f"{prefix}.{idx}.weight"].detach().to(self.device, torch.float32).contiguous()
                b = sd[f"{prefix}.{idx}.bias"].detach().to(self.device, torch.float32).contiguous()
                keep += [W, b]
                if W.dim() != 4 or W.shape[2] != W.shape[3]:
                    raise ValueError(f"{prefix}.{idx}.weight: expected a square Conv2d kernel, got {tuple(W.shape)}")
                self._check(self.lib.tdmpc2_plan_bind_pixel_encoder(self._h, layer, _ptr(W), _ptr(b), int(W.shape[0]),
                                                                    int(W.shape[1]), int(W.shape[2]), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()  # sources may now be freed
        self.pix_channels = int(sd[f"{prefix}.2.weight"].shape[1])

    def _pix_inputs(self, obs, shift):
        dev = self.device
        if getattr(self, "pix_channels", None) is None:
            raise NativeError("no pixel encoder bound (bind_pixel_encoder)")
        E = int(obs.shape[0])
        if obs.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"obs: expected dtype torch.uint8 or torch.float32, got {obs.dtype}")
        _chk_tensor("obs", obs, obs.dtype, (E, self.pix_channels, 64, 64), dev)
        _chk_tensor("shift", shift, torch.int32, (E, 2), dev)
        return E, 0 if obs.dtype == torch.uint8 else 1

    def encode_pix(self, obs, shift, out: Optional[torch.Tensor] = None):
        """WorldModel.encode for rgb observations: obs [E, Cin, 64, 64] (uint8 or fp32 pixel levels), shift int32 [E, 2]
        (`draw_shift`) -> z [E, L]."""
        E, dt = self._pix_inputs(obs, shift)
        z = out if out is not None else torch.empty(E, self.cfg.latent_dim, device=self.device, dtype=torch.float32)
        _chk_tensor("z", z, torch.float32, (E, self.cfg.latent_dim), self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_encode_pix(self._h, E, _ptr(obs), dt, self.pix_channels, _ptr(shift), _ptr(z),
                                                        self._stream()))
        return z

    def reserve_pix_batch(self, chunk_images: int):
        """Workspace of `encode_pix_batch` for `chunk_images` images per pass (grows, never shrinks; needs a bound pixel encoder).
        The only call of the batch route that allocates."""
        chunk_images = int(chunk_images)
        if chunk_images < 1:
            raise ValueError(f"chunk_images: expected >= 1, got {chunk_images}")
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_pix_batch_reserve(self._h, chunk_images, self._stream()))
        self.pix_batch_chunk = max(self.pix_batch_chunk, chunk_images)

    def encode_pix_batch(self, obs, shift, out: Optional[torch.Tensor] = None):
        """WorldModel.encode on the frame stacks of a training batch: obs [n, Cin, 64, 64] (uint8 or fp32 pixel levels), shift
        int32 [n, 2] (`draw_shift`) -> z [n, L], for any n >= 1 (not bounded by max_envs): passes of the chunk that
        `reserve_pix_batch` sized, on the MFMA batch route."""
        n, dt = self._pix_inputs(obs, shift)
        if n < 1:
            raise ValueError("obs: expected at least one image")
        z = out if out is not None else torch.empty(n, self.cfg.latent_dim, device=self.device, dtype=torch.float32)
        _chk_tensor("z", z, torch.float32, (n, self.cfg.latent_dim), self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_encode_pix_batch(self._h, n, _ptr(obs), dt, self.pix_channels, _ptr(shift), _ptr(z),
                                                              self._stream()))
        return z

    def plan_pix(self, obs, shift, disc_pow, prev_mean, t0, eval_mode=False, tape: Optional[Dict[str, torch.Tensor]] = None,
                 seed: int = 0, out: Optional[torch.Tensor] = None):
        """TDMPC2._plan from the frame stack on: encode_pix + plan in one library call (single-task models)."""
        cfg, dev = self.cfg, self.device
        E, dt = self._pix_inputs(obs, shift)
        H, A = cfg.horizon, cfg.action_dim
        _chk_tensor("disc_pow", disc_pow, torch.float32, (E, H + 1), dev)
        _chk_tensor("prev_mean", prev_mean, torch.float32, (E, H, A), dev)
        _chk_tensor("t0", t0, torch.uint8, (E,), dev)
        action = out if out is not None else torch.empty(E, A, device=dev, dtype=torch.float32)
        _chk_tensor("action", action, torch.float32, (E, A), dev)
        noise_p = None
        if tape is not None:
            noise = self._noise(tape, E)
            noise_p = C.byref(noise)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_run_pix(self._h, E, _ptr(obs), dt, self.pix_channels, _ptr(shift), _ptr(disc_pow),
                                                     _ptr(prev_mean), _ptr(t0), int(bool(eval_mode)), noise_p,
                                                     C.c_uint64(int(seed) & (2**64 - 1)), _ptr(action), self._stream()))
        return action

    # ------------------------------------------------------------------ policy prior (ABI 11)
    def bind_policy(self, sd: Dict[str, torch.Tensor], prefix: str = "_pi"):
        """Bind the policy prior's fp32 copy (`_pi.{0,1,2}.{weight,bias}`, `_pi.{0,1}.ln.{weight,bias}`) for `pi` / `act_pi` /
        `act_pi_pix`.  Separate from `bind_state_dict` (whose policy copy is in the planner's MFMA layouts); not part of the
        packed blob: bind again after `import_packed`."""
        keep = []
        with torch.cuda.device(self.device):
            for layer in range(3):
                ts = []
                for name in ("weight", "bias", "ln.weight", "ln.bias"):
                    k = f"{prefix}.{layer}.{name}"
                    t = sd[k].detach().to(self.device, torch.float32).contiguous() if k in sd else None
                    keep.append(t)
                    ts.append(t)
                W = ts[0]
                self._check(self.lib.tdmpc2_plan_bind_policy(self._h, layer, _ptr(W), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]),
                                                             int(W.shape[0]), int(W.shape[1]), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()  # sources may now be freed
        self.policy_bound = True

    def set_policy_route(self, mode: int):
        """TDMPC2_TUNE_POLICY_ROUTE: 0 auto (default), 1 the row route, 2 the spread route."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, TUNE_POLICY_ROUTE, int(mode)))

    def _policy_io(self, n, task_emb, act_mask, eps, return_eps):
        cfg, dev, A = self.cfg, self.device, self.cfg.action_dim
        if cfg.multitask:
            if task_emb is None or act_mask is None:
                raise ValueError("a multitask policy prior needs task_emb and act_mask")
            _chk_tensor("task_emb", task_emb, torch.float32, (n, cfg.task_dim), dev)
            _chk_tensor("act_mask", act_mask, torch.float32, (n, A), dev)
        else:
            task_emb = act_mask = None
        if eps is not None:
            _chk_tensor("eps", eps, torch.float32, (n, A), dev)
        f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
        info = {"mean": f(n, A), "log_std": f(n, A), "action_prob": 1.0, "entropy": f(n, 1), "scaled_entropy": f(n, 1)}
        if return_eps:
            info["eps"] = f(n, A)
        action = f(n, A)
        out = PolicyOut(action=action.data_ptr(), mean=info["mean"].data_ptr(), log_std=info["log_std"].data_ptr(),
                        entropy=info["entropy"].data_ptr(), scaled_entropy=info["scaled_entropy"].data_ptr(),
                        eps_out=info["eps"].data_ptr() if return_eps else None)
        return task_emb, act_mask, action, info, out

    def pi(self, z, task_emb=None, act_mask=None, eps=None, seed: int = 0, return_eps: bool = False):
        """WorldModel.pi (world_model.py:144-184) on z [n, L] -> (action [n, A], info) with the reference's info keys
        ('mean', 'log_std', 'action_prob', 'entropy' [n, 1], 'scaled_entropy' [n, 1]).  Multitask: per-row task_emb [n, T] and
        act_mask [n, A].  eps [n, A] (torch.randn_like's draws) or None: drawn in the kernel from Philox(seed, call counter);
        return_eps adds info['eps'], the draws used (passed back as eps they replay the call bit for bit)."""
        n = int(z.shape[0])
        _chk_tensor("z", z, torch.float32, (n, self.cfg.latent_dim), self.device)
        emb, mask, action, info, out = self._policy_io(n, task_emb, act_mask, eps, return_eps)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_pi(self._h, n, _ptr(z), _ptr(emb), _ptr(mask), _ptr(eps),
                                                C.c_uint64(int(seed) & (2**64 - 1)), C.byref(out), self._stream()))
        return action, info

    def act_pi(self, obs, task_emb=None, act_mask=None, eps=None, eval_mode: bool = False, seed: int = 0,
               return_eps: bool = False):
        """TDMPC2.act with mpc = False (tdmpc2.py:114-120) for state observations: encode + pi in the library (the 5M model:
        one launch).  eval_mode returns info['mean'] as the action."""
        E = int(obs.shape[0])
        _chk_tensor("obs", obs, torch.float32, (E, self.obs_dim), self.device)
        emb, mask, action, info, out = self._policy_io(E, task_emb, act_mask, eps, return_eps)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_act_pi(self._h, E, _ptr(obs), int(self.obs_dim or 0), _ptr(emb), _ptr(mask), _ptr(eps),
                                                    int(bool(eval_mode)), C.c_uint64(int(seed) & (2**64 - 1)), C.byref(out),
                                                    self._stream()))
        return action, info

    def act_pi_pix(self, obs, shift, eps=None, eval_mode: bool = False, seed: int = 0, return_eps: bool = False):
        """The same for rgb observations: encode_pix (obs, ShiftAug's `shift`: `draw_shift`) + pi (single-task models)."""
        E, dt = self._pix_inputs(obs, shift)
        _, _, action, info, out = self._policy_io(E, None, None, eps, return_eps)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_act_pi_pix(self._h, E, _ptr(obs), dt, self.pix_channels, _ptr(shift), _ptr(eps),
                                                        int(bool(eval_mode)), C.c_uint64(int(seed) & (2**64 - 1)), C.byref(out),
                                                        self._stream()))
        return action, info

    def _noise(self, tape, E):
        shapes = self.noise_shapes(E)
        for k, (shp, dt) in shapes.items():
            _chk_tensor(f"tape[{k}]", tape[k], dt, shp, self.device)
        if self._npad != self.cfg.num_samples:  # pad the sample axis with zeros: the padding rows' draws are irrelevant
            cfg, N, NP, P = self.cfg, self.cfg.num_samples, self._npad, self.cfg.num_pi_trajs
            se = torch.zeros(E, self.iterations, cfg.horizon, NP - P, cfg.action_dim, device=self.device)
            se[:, :, :, :N - P] = tape["sample_eps"]
            pe = torch.zeros(E, self.iterations, NP, cfg.action_dim, device=self.device)
            pe[:, :, :N] = tape["pi_eps"]
            tape = dict(tape, sample_eps=se, pi_eps=pe)
            self._padded_tape = tape  # (kept alive until the next call)
        return Noise(**{k: tape[k].data_ptr() for k in shapes})

    def _whole_tiles_only(self, what):
        if self._npad != self.cfg.num_samples:
            raise NativeError(f"{what} is a stage-wise entry point: it needs num_samples ({self.cfg.num_samples}) to be a multiple of the "
                              f"kernels' row tile; plan() / plan_obs() pad to {self._npad} themselves")

    def noise_shapes(self, E):
        """Shapes / dtypes of the six tensors of a noise tape for E environments (struct tdmpc2_noise)."""
        cfg = self.cfg
        H, N, K, P, A, I = cfg.horizon, cfg.num_samples, cfg.num_elites, cfg.num_pi_trajs, cfg.action_dim, self.iterations
        return {"pi_traj_eps": ((E, H, P, A), torch.float32), "sample_eps": ((E, I, H, N - P, A), torch.float32),
                "pi_eps": ((E, I, N, A), torch.float32), "qidx": ((E, I, 2), torch.int32),
                "gumbel_exp": ((E, K), torch.float32), "final_eps": ((E, A), torch.float32)}

    def call_counter(self) -> int:
        """The handle's call counter: the value the NEXT plan / td_target / policy_value call mixes into its Philox key."""
        n = C.c_uint32()
        self._check(self.lib.tdmpc2_plan_call_counter(self._h, C.byref(n)))
        return int(n.value)

    def set_call_counter(self, value: int):
        self._check(self.lib.tdmpc2_plan_set_call_counter(self._h, C.c_uint32(int(value) & 0xFFFFFFFF)))

    def export_noise(self, seed: int, call: int, n_envs: int, env_first: int = 0, fields=None):
        """The draws a tape = None plan makes under (seed, call = call_counter() read BEFORE that plan) for environments
        [env_first, env_first + n_envs), as a noise-tape dict: feeding it back as `tape` reproduces the plan bit for bit,
        and the same tensors replay through the CPU oracle (tdmpc2_plan_export_noise)."""
        self._whole_tiles_only("export_noise")
        shapes = self.noise_shapes(n_envs)
        out = {k: torch.empty(shp, dtype=dt, device=self.device) for k, (shp, dt) in shapes.items() if fields is None or k in fields}
        noise = Noise(**{k: v.data_ptr() for k, v in out.items()})
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_export_noise(self._h, int(env_first), int(n_envs), C.c_uint64(int(seed) & (2**64 - 1)),
                                                          C.c_uint32(int(call) & 0xFFFFFFFF), C.byref(noise), self._stream()))
        return out

    def take_fault(self) -> int:
        """Number of calls invalidated by a bounded inter-workgroup wait that gave up (cluster path, fused NormedLinear epilogue)
        since the last take_fault; such a plan returned NaN actions and kept its prev_mean, such a td_target / policy_value
        returned NaN.  The handle runs the paths without waits until it re-arms (fault_info, set_rearm_after).  Call after a sync."""
        n = C.c_int()
        self._check(self.lib.tdmpc2_plan_take_fault(self._h, C.byref(n)))
        return int(n.value)

    def fault_word(self, dst):
        """tdmpc2_plan_fault_word: the device-visible verdict word of the calls in flight copied into dst[0] (int32, on this device)
        in stream order -- no host synchronisation (dist.sharded_plan appends it to the slice it all-gathers)."""
        _chk_tensor("dst", dst, torch.int32, (1,), self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_fault_word(self._h, _ptr(dst), self._stream()))

    def fault_info(self) -> dict:
        """The handle's fault history (tdmpc2_plan_fault_info): faults_total, rearms, degraded, clean_calls, rearm_after,
        seconds_since_fault (-1: never).  Nothing is consumed."""
        fi = FaultInfo()
        self._check(self.lib.tdmpc2_plan_fault_info(self._h, C.byref(fi)))
        return {k: getattr(fi, k) for k, _ in FaultInfo._fields_ if k != "reserved"}

    def set_expert(self, name: str, value: Optional[int]):
        """A measurement knob of the layered family's tile choice (TDMPC2_TUNE_EXPERT + tdmpc2_expert_knob); None = the default."""
        v = -2**31 if value is None else int(value)
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, TUNE_EXPERT + EXPERT_KNOBS.index(name), v))

    def set_fewrow(self, on):
        """Layered family (TDMPC2_TUNE_FEWROW): K-part tiles + row kernels for calls with few sample rows (single plans)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 7, int(bool(on))))

    def set_wait_us(self, us):
        """Wall-clock bound of the inter-workgroup waits in microseconds (TDMPC2_TUNE_WAIT_US; default 5000)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 8, int(us)))

    def set_ksplit(self, mode):
        """TDMPC2_TUNE_KSPLIT: layered family -- split 256 x 256 GEMM tiles along K over 2-4 workgroups: 0 never (a plan's bits do
        not depend on the size of the call it is part of), 1 whenever the round arithmetic says so, 2 (default) only for
        launches that leave most of the chip idle (single plans of the 317M model)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 6, int(mode)))

    def plan_safely_once(self, on: bool = True):
        """TDMPC2_TUNE_SAFE_ONCE: the next whole plan (plan(), or shard_begin .. the last shard_refit) runs on the paths without
        inter-workgroup waits; the settings asked for, the downgrade state and the re-arm counter stay as they are."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 5, int(bool(on))))

    def set_rearm_after(self, clean_calls: int):
        """TDMPC2_TUNE_REARM_AFTER: clean calls after which a handle downgraded by a reported wait returns to the fast paths (0: never)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 4, int(clean_calls)))

    # ------------------------------------------------------------------ training-side forward pieces
    def _task_tables(self, R, task_ids, task_emb_table, act_mask_table, discount_table=None):
        """struct tdmpc2_task_tables for a multitask batch (None for single-task handles).  Returns (ctypes pointer | None,
        keep-alive tuple)."""
        cfg, dev = self.cfg, self.device
        if not cfg.multitask:
            if task_ids is not None:
                raise ValueError("task_ids given to a single-task planner")
            return None, ()
        if task_ids is None or task_emb_table is None or act_mask_table is None:
            raise ValueError("multitask policy_value / td_target need task_ids, task_emb_table and act_mask_table")
        n_tasks = int(task_emb_table.shape[0])
        _chk_tensor("task_ids", task_ids, torch.int32, (R,), dev)
        _chk_tensor("task_emb_table", task_emb_table, torch.float32, (n_tasks, cfg.task_dim), dev)
        _chk_tensor("act_mask_table", act_mask_table, torch.float32, (n_tasks, cfg.action_dim), dev)
        if discount_table is not None:
            _chk_tensor("discount_table", discount_table, torch.float32, (n_tasks,), dev)
        tt = TaskTables(task_ids=task_ids.data_ptr(), task_emb=task_emb_table.data_ptr(), act_mask=act_mask_table.data_ptr(),
                        discount=None if discount_table is None else discount_table.data_ptr(), n_tasks=n_tasks)
        return C.byref(tt), (tt, task_ids, task_emb_table, act_mask_table, discount_table)

    def policy_value(self, z, use_target=False, reduce="avg", pi_eps=None, qidx=None, seed: int = 0, return_action=True,
                     task_ids=None, task_emb_table=None, act_mask_table=None):
        """a = pi(z), then two Q heads of the online / target ensemble, 'avg' or 'min' (the forward half of
        TDMPC2.update_pi, tdmpc2.py:208-225).  z [R, L] -> (action [R, A] or None, q [R]).  Multitask models: one task
        per row (`task_ids` int32 [R]) + the model's embedding / action-mask tables (world_model.py:88-101)."""
        cfg, dev = self.cfg, self.device
        R = int(z.shape[0])
        _chk_tensor("z", z, torch.float32, (R, cfg.latent_dim), dev)
        if pi_eps is not None:
            _chk_tensor("pi_eps", pi_eps, torch.float32, (R, cfg.action_dim), dev)
        if qidx is not None:
            _chk_tensor("qidx", qidx, torch.int32, (2,), dev)
        tt, keep = self._task_tables(R, task_ids, task_emb_table, act_mask_table)
        action = torch.empty(R, cfg.action_dim, device=dev) if return_action else None
        q = torch.empty(R, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_policy_value_mt(self._h, R, _ptr(z), tt, int(bool(use_target)), int(reduce == "min"),
                                                             _ptr(pi_eps), _ptr(qidx), C.c_uint64(int(seed) & (2**64 - 1)),
                                                             _ptr(action), _ptr(q), self._stream()))
        return action, q

    def td_target(self, next_z, reward, terminated, discount, pi_eps=None, qidx=None, seed: int = 0,
                  task_ids=None, task_emb_table=None, act_mask_table=None):
        """TDMPC2._td_target (tdmpc2.py:239-254) on flattened rows: next_z [R, L], reward / terminated [R] -> td [R].
        `discount`: python float (single task) or the per-task fp32 tensor TDMPC2.discount (multitask, tdmpc2.py:35-37)."""
        cfg, dev = self.cfg, self.device
        R = int(next_z.shape[0])
        _chk_tensor("next_z", next_z, torch.float32, (R, cfg.latent_dim), dev)
        _chk_tensor("reward", reward, torch.float32, (R,), dev)
        _chk_tensor("terminated", terminated, torch.float32, (R,), dev)
        if pi_eps is not None:
            _chk_tensor("pi_eps", pi_eps, torch.float32, (R, cfg.action_dim), dev)
        if qidx is not None:
            _chk_tensor("qidx", qidx, torch.int32, (2,), dev)
        disc_tab = discount if cfg.multitask else None
        tt, keep = self._task_tables(R, task_ids, task_emb_table, act_mask_table, disc_tab)
        td = torch.empty(R, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_td_target_mt(self._h, R, _ptr(next_z), _ptr(reward), _ptr(terminated),
                                                          C.c_float(0.0 if cfg.multitask else float(discount)), tt,
                                                          _ptr(pi_eps), _ptr(qidx), C.c_uint64(int(seed) & (2**64 - 1)),
                                                          _ptr(td), self._stream()))
        return td

    def _model_out(self, B, H, want):
        """Output tensors of a model rollout, shaped as the reference returns them, and the struct pointing at them."""
        cfg, dev = self.cfg, self.device
        nb = max(cfg.num_bins, 1)
        shapes = {"zs": (H + 1, B, cfg.latent_dim), "reward_logits": (H, B, nb), "reward": (H, B, 1),
                  "q_logits": (cfg.num_q, H, B, nb), "q": (cfg.num_q, H, B, 1), "term_logit": (H + 1, B, 1)}
        for k in want:
            if k not in shapes:
                raise ValueError(f"unknown model output {k!r} (one of {MODEL_OUTPUTS})")
        res = {k: torch.empty(shapes[k], device=dev) for k in want}
        mo = ModelOut(**{k: (res[k].data_ptr() if k in res else None) for k in MODEL_OUTPUTS})
        return res, mo

    def model_rollout(self, z0, actions, use_target=False, want=MODEL_OUTPUTS[:5], task_ids=None, task_emb_table=None,
                      act_mask_table=None):
        """The open-loop latent rollout on recorded actions and the predictions on it (tdmpc2.py:268-283): z0 [B, L], actions
        [H, B, A] -> dict of the outputs named in `want` (tdmpc2_model_out; q_logits [num_q, H, B, bins]).  Multitask models:
        `task_ids` int32 [B], one task per row of the batch."""
        cfg, dev = self.cfg, self.device
        B, H = int(z0.shape[0]), int(actions.shape[0])
        _chk_tensor("z0", z0, torch.float32, (B, cfg.latent_dim), dev)
        _chk_tensor("actions", actions, torch.float32, (H, B, cfg.action_dim), dev)
        tt, keep = self._task_tables(B, task_ids, task_emb_table, act_mask_table)
        res, mo = self._model_out(B, H, tuple(want))
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_model_rollout_mt(self._h, B, H, _ptr(z0), _ptr(actions), tt, int(bool(use_target)),
                                                              C.byref(mo), self._stream()))
        return res

    def model_losses(self, z0, actions, next_z, reward, td_target, terminated=None, rho=0.5, coefs=(20.0, 0.1, 0.1, 1.0),
                     use_target=False, want=(), step_means=False, task_ids=None, task_emb_table=None, act_mask_table=None):
        """The rollout plus the losses of TDMPC2._update (tdmpc2.py:285-304): targets next_z [H, B, L], reward / td_target /
        terminated [H, B] (terminated: episodic models only); coefs = (consistency, reward, value, termination).  Returns a dict:
        "losses" [5] (consistency, reward, value, termination, total), optionally "step_means" [4, H], and the outputs in `want`."""
        cfg, dev = self.cfg, self.device
        B, H = int(z0.shape[0]), int(actions.shape[0])
        _chk_tensor("z0", z0, torch.float32, (B, cfg.latent_dim), dev)
        _chk_tensor("actions", actions, torch.float32, (H, B, cfg.action_dim), dev)
        _chk_tensor("next_z", next_z, torch.float32, (H, B, cfg.latent_dim), dev)
        _chk_tensor("reward", reward, torch.float32, (H, B), dev)
        _chk_tensor("td_target", td_target, torch.float32, (H, B), dev)
        if terminated is not None:
            _chk_tensor("terminated", terminated, torch.float32, (H, B), dev)
        tt, keep = self._task_tables(B, task_ids, task_emb_table, act_mask_table)
        res, mo = self._model_out(B, H, tuple(want))
        tg = ModelTargets(next_z=next_z.data_ptr(), reward=reward.data_ptr(), td_target=td_target.data_ptr(),
                          terminated=None if terminated is None else terminated.data_ptr(), rho=float(rho),
                          consistency_coef=float(coefs[0]), reward_coef=float(coefs[1]), value_coef=float(coefs[2]),
                          termination_coef=float(coefs[3]))
        res["losses"] = torch.empty(5, device=dev)
        if step_means:
            res["step_means"] = torch.empty(4, H, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_model_losses_mt(self._h, B, H, _ptr(z0), _ptr(actions), tt, int(bool(use_target)),
                                                             C.byref(tg), C.byref(mo), _ptr(res["losses"]),
                                                             _ptr(res.get("step_means")), self._stream()))
        return res

    def policy_loss(self, zs, scale, rho=0.5, entropy_coef=1e-4, tau=0.01, update_scale=True, pi_eps=None, qidx=None, seed: int = 0,
                    want=(), task_ids=None, task_emb_table=None, act_mask_table=None):
        """The forward of TDMPC2.update_pi (tdmpc2.py:208-239): zs [T, B, L], `scale` the fp32 [1] device tensor RunningScale.value
        (updated in place from q[0] before the division when `update_scale`).  Returns a dict: "loss" [4] (pi_loss, mean entropy,
        mean scaled_entropy, the scale after the call) and the outputs named in `want` (tdmpc2_policy_loss_out: action [T, B, A],
        q / entropy / scaled_entropy [T, B, 1], step_means [3, T], percentiles [2]).  Multitask models: `task_ids` int32 [B]."""
        cfg, dev = self.cfg, self.device
        T, B = int(zs.shape[0]), int(zs.shape[1])
        _chk_tensor("zs", zs, torch.float32, (T, B, cfg.latent_dim), dev)
        _chk_tensor("scale", scale, torch.float32, (1,), dev)
        if pi_eps is not None:
            _chk_tensor("pi_eps", pi_eps, torch.float32, (T, B, cfg.action_dim), dev)
        if qidx is not None:
            _chk_tensor("qidx", qidx, torch.int32, (2,), dev)
        tt, keep = self._task_tables(B, task_ids, task_emb_table, act_mask_table)
        shapes = {"action": (T, B, cfg.action_dim), "q": (T, B, 1), "entropy": (T, B, 1), "scaled_entropy": (T, B, 1),
                  "step_means": (3, T), "percentiles": (2,)}
        for k in want:
            if k not in shapes:
                raise ValueError(f"unknown policy_loss output {k!r} (one of {POLICY_LOSS_OUTPUTS})")
        res = {k: torch.empty(shapes[k], device=dev) for k in want}
        po = PolicyLossOut(**{k: (res[k].data_ptr() if k in res else None) for k in POLICY_LOSS_OUTPUTS})
        pin = PolicyLossIn(rho=float(rho), entropy_coef=float(entropy_coef), tau=float(tau), update_scale=int(bool(update_scale)))
        res["loss"] = torch.empty(4, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_policy_loss_mt(self._h, B, T - 1, _ptr(zs), tt, _ptr(pi_eps), _ptr(qidx),
                                                            C.c_uint64(int(seed) & (2**64 - 1)), C.byref(pin), _ptr(scale),
                                                            C.byref(po), _ptr(res["loss"]), self._stream()))
        return res

    def running_scale(self, x, scale, tau=0.01, percentiles=None):
        """RunningScale.update (common/scale.py:39-42): x (any shape, n values) lerps the fp32 [1] device tensor `scale` in place;
        `percentiles` (fp32 [2] device tensor, optional) receives the 5th / 95th percentile."""
        dev = self.device
        n = int(x.numel())
        _chk_tensor("x", x, torch.float32, tuple(x.shape), dev)
        _chk_tensor("scale", scale, torch.float32, (1,), dev)
        if percentiles is not None:
            _chk_tensor("percentiles", percentiles, torch.float32, (2,), dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_running_scale(self._h, n, _ptr(x), C.c_float(float(tau)), _ptr(scale), _ptr(percentiles),
                                                           self._stream()))
        return scale

    def termination_stats(self, term_logit, terminated):
        """math.termination_statistics(sigmoid(term_logit), terminated) (common/math.py:97-109): n rows each -> fp32 [2] = rate, f1."""
        dev = self.device
        n = int(term_logit.numel())
        _chk_tensor("term_logit", term_logit, torch.float32, tuple(term_logit.shape), dev)
        _chk_tensor("terminated", terminated, torch.float32, tuple(terminated.shape), dev)
        if int(terminated.numel()) != n:
            raise ValueError(f"term_logit has {n} rows, terminated {int(terminated.numel())}")
        stats = torch.empty(2, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_termination_stats(self._h, n, _ptr(term_logit), _ptr(terminated), _ptr(stats),
                                                               self._stream()))
        return stats

    # ------------------------------------------------------------------ packed weight file
    def export_packed(self) -> bytes:
        """Everything the binds produced (fragment-ordered weights, scales, LayerNorm parameters, encoder, target ensemble when
        bound) as one blob; specific to this handle's kernel family and arithmetic (tdmpc2_plan_export_packed)."""
        n = C.c_uint64()
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_packed_size(self._h, C.byref(n)))
            buf = (C.c_char * n.value)()
            self._check(self.lib.tdmpc2_plan_export_packed(self._h, C.cast(buf, C.c_void_p), n, self._stream()))
        return bytes(buf)

    def import_packed(self, blob: bytes, obs_dim: Optional[int] = None):
        """Restore the weights from `export_packed` output: host-to-device copies only (no packing kernels)."""
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_plan_import_packed(self._h, C.cast(buf, C.c_void_p), C.c_uint64(len(blob)), self._stream()))
        if obs_dim is not None:
            self.obs_dim = int(obs_dim)

    def save_packed(self, path: str):
        with open(path, "wb") as f:
            f.write(self.export_packed())

    def load_packed(self, path: str, obs_dim: Optional[int] = None):
        with open(path, "rb") as f:
            self.import_packed(f.read(), obs_dim)

    # ------------------------------------------------------------------ planning
    def _common_inputs(self, E, z0, task_emb, act_mask, disc_pow):
        cfg, dev = self.cfg, self.device
        _chk_tensor("z0", z0, torch.float32, (E, cfg.latent_dim), dev)
        _chk_tensor("disc_pow", disc_pow, torch.float32, (E, cfg.horizon + 1), dev)
        if cfg.multitask:
            if task_emb is None or act_mask is None:
                raise ValueError("multitask planning needs task_emb and act_mask")
            _chk_tensor("task_emb", task_emb, torch.float32, (E, cfg.task_dim), dev)
            _chk_tensor("act_mask", act_mask, torch.float32, (E, cfg.action_dim), dev)

    def plan(self, z0, disc_pow, prev_mean, t0, eval_mode=False, task_emb=None, act_mask=None,
             tape: Optional[Dict[str, torch.Tensor]] = None, seed: int = 0, debug: bool = False,
             out: Optional[torch.Tensor] = None):
        """E plans in one call.  `prev_mean` [E,H,A] is updated in place.
        Returns action [E,A] (device), or (action, stages) when `debug`."""
        cfg, dev = self.cfg, self.device
        E = int(z0.shape[0])
        H, N, K, P, A, I = cfg.horizon, cfg.num_samples, cfg.num_elites, cfg.num_pi_trajs, cfg.action_dim, self.iterations
        self._common_inputs(E, z0, task_emb, act_mask, disc_pow)
        _chk_tensor("prev_mean", prev_mean, torch.float32, (E, H, A), dev)
        _chk_tensor("t0", t0, torch.uint8, (E,), dev)
        action = out if out is not None else torch.empty(E, A, device=dev, dtype=torch.float32)
        _chk_tensor("action", action, torch.float32, (E, A), dev)
        noise_p = None
        if tape is not None:
            noise = self._noise(tape, E)
            noise_p = C.byref(noise)
        dbg_p, stages = None, None
        if debug:
            NP = self._npad  # (stages come back sliced to the caller's num_samples)
            stages = {"value": torch.empty(E, I, NP, device=dev), "elite_idx": torch.empty(E, I, K, device=dev, dtype=torch.int32),
                      "score": torch.empty(E, I, K, device=dev), "mean": torch.empty(E, I, H, A, device=dev),
                      "std": torch.empty(E, I, H, A, device=dev), "actions": torch.empty(E, I, H, NP, A, device=dev)}
            dbg = Debug(**{k: v.data_ptr() for k, v in stages.items()})
            dbg_p = C.byref(dbg)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_run(self._h, E, _ptr(z0), _ptr(task_emb), _ptr(act_mask), _ptr(disc_pow),
                                                 _ptr(prev_mean), _ptr(t0), int(bool(eval_mode)), noise_p,
                                                 C.c_uint64(int(seed) & (2**64 - 1)), _ptr(action), dbg_p, self._stream()))
        if debug and self._npad != N:
            stages["value"] = stages["value"][:, :, :N].contiguous()
            stages["actions"] = stages["actions"][:, :, :, :N].contiguous()
        return (action, stages) if debug else action

    def estimate_value(self, z0, disc_pow, actions, pi_eps, qidx, task_emb=None, act_mask=None, trace=False):
        """TDMPC2._estimate_value (tdmpc2/tdmpc2.py:122-136) on given action sequences -> value [E,N].
        With `trace`, also returns (tiles [E*N/64, 5H+7, 64, L], scalars [E, N, H+2+A])."""
        cfg, dev = self.cfg, self.device
        self._whole_tiles_only("estimate_value")
        E = int(z0.shape[0])
        self._common_inputs(E, z0, task_emb, act_mask, disc_pow)
        _chk_tensor("actions", actions, torch.float32, (E, cfg.horizon, cfg.num_samples, cfg.action_dim), dev)
        _chk_tensor("pi_eps", pi_eps, torch.float32, (E, cfg.num_samples, cfg.action_dim), dev)
        _chk_tensor("qidx", qidx, torch.int32, (E, 2), dev)
        value = torch.empty(E, cfg.num_samples, device=dev, dtype=torch.float32)
        tiles = scalars = None
        if trace:
            if self.path == PATH_FUSED:  # the layered path dumps the per-row scalars only
                tiles = torch.zeros(E * cfg.num_samples // 64, 5 * cfg.horizon + 7, 64, cfg.latent_dim, device=dev)
            scalars = torch.zeros(E, cfg.num_samples, cfg.horizon + 2 + cfg.action_dim, device=dev)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_estimate_value_trace(
                self._h, E, _ptr(z0), _ptr(task_emb), _ptr(act_mask), _ptr(disc_pow), _ptr(actions), _ptr(pi_eps),
                _ptr(qidx), _ptr(value), _ptr(tiles), _ptr(scalars), self._stream()))
        return (value, tiles, scalars) if trace else value

    def refit(self, value, actions, act_mask=None):
        """Elite select + refit (tdmpc2/tdmpc2.py:184-197).  `value` [E,N] gets nan_to_num in place.
        Returns (mean, std, score, elite_idx)."""
        self._whole_tiles_only("refit")
        cfg, dev = self.cfg, self.device
        E = int(value.shape[0])
        H, N, K, A = cfg.horizon, cfg.num_samples, cfg.num_elites, cfg.action_dim
        _chk_tensor("value", value, torch.float32, (E, N), dev)
        _chk_tensor("actions", actions, torch.float32, (E, H, N, A), dev)
        mean = torch.empty(E, H, A, device=dev)
        std = torch.empty(E, H, A, device=dev)
        score = torch.empty(E, K, device=dev)
        idx = torch.empty(E, K, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_refit(self._h, E, _ptr(value), _ptr(actions), _ptr(act_mask), _ptr(mean),
                                                   _ptr(std), _ptr(score), _ptr(idx), self._stream()))
        return mean, std, score, idx

    # ------------------------------------------------------------------ one plan sharded over ranks (tdmpc2_amd/dist.py)
    @property
    def shard_granularity(self) -> int:
        """Row ranges of shard_values are multiples of this many sample rows."""
        return 64 if self.path == PATH_FUSED else 128

    def shard_begin(self, z0, prev_mean, t0, task_emb=None, act_mask=None, tape=None, seed: int = 0):
        """Prologue of a plan whose sample rows are split over ranks: warm start + policy-prior trajectories
        (tdmpc2.py:154-170), replicated on every rank."""
        self._whole_tiles_only("shard_begin")
        cfg, dev = self.cfg, self.device
        E = int(z0.shape[0])
        _chk_tensor("z0", z0, torch.float32, (E, cfg.latent_dim), dev)
        _chk_tensor("prev_mean", prev_mean, torch.float32, (E, cfg.horizon, cfg.action_dim), dev)
        _chk_tensor("t0", t0, torch.uint8, (E,), dev)
        self._shard_noise = self._noise(tape, E) if tape is not None else None
        noise_p = C.byref(self._shard_noise) if self._shard_noise is not None else None
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_shard_begin(self._h, E, _ptr(z0), _ptr(task_emb), _ptr(act_mask), _ptr(prev_mean),
                                                         _ptr(t0), noise_p, C.c_uint64(int(seed) & (2**64 - 1)), self._stream()))

    def shard_values(self, it: int, row_begin: int, row_end: int, z0, disc_pow, value, act_mask=None, seed: int = 0):
        """Sample the iteration's actions (all rows, replicated) and evaluate rows [row_begin, row_end) of every plan into
        value[E, N] (other columns untouched)."""
        cfg, dev = self.cfg, self.device
        E = int(z0.shape[0])
        _chk_tensor("value", value, torch.float32, (E, cfg.num_samples), dev)
        _chk_tensor("disc_pow", disc_pow, torch.float32, (E, cfg.horizon + 1), dev)
        noise_p = C.byref(self._shard_noise) if self._shard_noise is not None else None
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_shard_values(self._h, E, int(it), int(row_begin), int(row_end), _ptr(z0), _ptr(act_mask),
                                                          _ptr(disc_pow), noise_p, C.c_uint64(int(seed) & (2**64 - 1)), _ptr(value),
                                                          self._stream()))

    def shard_refit(self, it: int, value, prev_mean, action, act_mask=None, eval_mode=False, seed: int = 0, stages=None):
        """Elite selection + refit on the complete value[E, N] (identical on every rank); the last iteration also picks the
        action and writes the new prev_mean."""
        cfg, dev = self.cfg, self.device
        E = int(value.shape[0])
        _chk_tensor("value", value, torch.float32, (E, cfg.num_samples), dev)
        _chk_tensor("action", action, torch.float32, (E, cfg.action_dim), dev)
        noise_p = C.byref(self._shard_noise) if self._shard_noise is not None else None
        dbg_p = None
        if stages is not None:
            dbg = Debug(**{k: v.data_ptr() for k, v in stages.items()})
            dbg_p = C.byref(dbg)
        with torch.cuda.device(dev):
            self._check(self.lib.tdmpc2_plan_shard_refit(self._h, E, int(it), _ptr(value), _ptr(act_mask), _ptr(prev_mean),
                                                         int(bool(eval_mode)), noise_p, C.c_uint64(int(seed) & (2**64 - 1)),
                                                         _ptr(action), dbg_p, self._stream()))

    def debug_buffers(self, E: int):
        """Stage buffers for the stage-wise entry points (shard_refit): sized to the handle's sample count, so whole tiles only."""
        self._whole_tiles_only("debug_buffers")
        cfg, dev, I = self.cfg, self.device, self.iterations
        H, N, K, A = cfg.horizon, cfg.num_samples, cfg.num_elites, cfg.action_dim
        return {"value": torch.empty(E, I, N, device=dev), "elite_idx": torch.empty(E, I, K, device=dev, dtype=torch.int32),
                "score": torch.empty(E, I, K, device=dev), "mean": torch.empty(E, I, H, A, device=dev),
                "std": torch.empty(E, I, H, A, device=dev), "actions": torch.empty(E, I, H, N, A, device=dev)}

    # ------------------------------------------------------------------ tuning / profiling
    def set_rows_per_workgroup(self, rows: int):
        """0 = automatic (32-row workgroups for calls with few plans: latency), or force 32 / 64 sample rows."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 0, int(rows)))

    def set_fold_refit(self, mode):
        """Fused family: elite selection + refit inside the rollout launch (True / 1), as a launch of its own (False / 0),
        or chosen per call (2, the default: inside when the call fits the chip in one round of workgroups)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 1, int(mode)))

    def set_cluster(self, mode):
        """Fused family, split arithmetic: the single-plan latency path (8 workgroups per 32-row tile, cluster_kernels.cuh):
        0 never, 1 whenever all of a call's clusters fit the chip at once, 2 (default) = 1 plus, for a single non-episodic plan,
        a second cluster per tile that runs the reward chain beside the dynamics chain (cluster2_kernels.cuh)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 2, int(mode)))

    def set_fuse_ln(self, on):
        """Layered family, split arithmetic: LayerNorm + Mish / SimNorm + operand split inside the GEMM epilogue (1, default)
        or as a row kernel over fp32 pre-activations (0)."""
        self._check(self.lib.tdmpc2_plan_set_tuning(self._h, 3, int(bool(on))))

    def set_profiling(self, max_launches: int):
        """Bracket up to `max_launches` rollout-kernel launches with HIP events (0 = off)."""
        self._check(self.lib.tdmpc2_plan_set_profiling(self._h, int(max_launches)))

    def profile_read(self):
        ms, n = C.c_float(), C.c_int()
        self._check(self.lib.tdmpc2_plan_profile_read(self._h, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)


def buffer_cfg(capacity: int, slice_len: int, fields, device_index: int = 0, max_batch: int = 0) -> BufferCfg:
    """struct tdmpc2_buffer_cfg; fields: (row_bytes, step_first, step_count) per field."""
    c = BufferCfg(capacity=int(capacity), slice_len=int(slice_len), device=int(device_index), n_fields=len(fields),
                  max_batch=int(max_batch))
    for i, (rb, s0, sc) in enumerate(fields[:BUFFER_MAX_FIELDS]):
        c.field[i] = BufferField(int(rb), int(s0), int(sc))
    return c


class NativeBuffer:
    """Owns one `tdmpc2_buffer_t`: an episode ring of opaque byte rows on one GPU with the reference Buffer's slice sampling
    (tdmpc2/common/buffer.py:13-115).  fields: (row_bytes, step_first, step_count) per field; tensors passed to add / load are
    [T, ...] / [N, T, ...] with row_bytes bytes per step, outputs of sample are [step_count, batch, row_bytes] bytes."""

    def __init__(self, capacity: int, slice_len: int, fields, device: torch.device, max_batch: int = 0):
        device = torch.device(device)
        if device.type != "cuda":
            raise NativeError(f"the replay buffer keeps its storage on an MI355X only (device {device}); there is no host storage")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load_library()
        self.device = device
        self.fields = [tuple(int(v) for v in f) for f in fields]
        self.capacity, self.slice_len = int(capacity), int(slice_len)
        h = C.c_void_p()
        self._h = C.c_void_p()
        self._check(self.lib.tdmpc2_buffer_create(C.byref(buffer_cfg(capacity, slice_len, self.fields, device.index, max_batch)),
                                                  C.byref(h)))
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            raise NativeError(f"tdmpc2_buffer error {rc}: {self.lib.tdmpc2_last_error().decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.tdmpc2_buffer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, tensors, lead):
        if len(tensors) != len(self.fields):
            raise ValueError(f"expected {len(self.fields)} field tensors, got {len(tensors)}")
        n = 1
        for d in lead:
            n *= int(d)
        ptrs = (C.c_void_p * len(self.fields))()
        keep = []
        for i, (t, (rb, _, _)) in enumerate(zip(tensors, self.fields)):
            if t.device != self.device:
                raise ValueError(f"field {i}: expected device {self.device}, got {t.device}")
            if tuple(t.shape[:len(lead)]) != tuple(lead) or t.numel() * t.element_size() != n * rb:
                raise ValueError(f"field {i}: expected {tuple(lead)} steps of {rb} bytes, got {tuple(t.shape)} {t.dtype}")
            t = t.contiguous()
            keep.append(t)
            ptrs[i] = t.data_ptr()
        return ptrs, keep

    def add(self, tensors):
        """One episode: tensors[f] is [T, ...]."""
        T = int(tensors[0].shape[0])
        ptrs, keep = self._rows(tensors, (T,))
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_buffer_add(self._h, T, ptrs, self._stream()))
        for t in keep:  # the copies are stream-ordered: the caching allocator must not hand the sources out before they ran
            t.record_stream(torch.cuda.current_stream(self.device))

    def load(self, tensors):
        """N episodes of equal length: tensors[f] is [N, T, ...]."""
        N, T = int(tensors[0].shape[0]), int(tensors[0].shape[1])
        ptrs, keep = self._rows(tensors, (N, T))
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_buffer_load(self._h, N, T, ptrs, self._stream()))
        for t in keep:
            t.record_stream(torch.cuda.current_stream(self.device))

    def sample(self, outs, seed: int = 0, index_out: Optional[torch.Tensor] = None):
        """outs[f]: a contiguous tensor of step_count x batch x row_bytes bytes on the device, or None (field not wanted)."""
        batch = None
        ptrs = (C.c_void_p * len(self.fields))()
        for i, (t, (rb, _, sc)) in enumerate(zip(outs, self.fields)):
            if t is None:
                continue
            if t.device != self.device or not t.is_contiguous():
                raise ValueError(f"output {i}: must be contiguous on {self.device}")
            nb = t.numel() * t.element_size()
            if nb % (rb * sc):
                raise ValueError(f"output {i}: {nb} bytes is not [{sc}, batch, {rb} bytes]")
            if batch is None:
                batch = nb // (rb * sc)
            if nb != batch * rb * sc:
                raise ValueError(f"output {i}: expected [{sc}, {batch}, {rb} bytes], got {tuple(t.shape)} {t.dtype}")
            ptrs[i] = t.data_ptr()
        if index_out is not None:
            _chk_tensor("index_out", index_out, torch.int64, (index_out.shape[0],), self.device)
            batch = int(index_out.shape[0]) if batch is None else batch
            if int(index_out.shape[0]) != batch:
                raise ValueError(f"index_out: expected [{batch}], got {tuple(index_out.shape)}")
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_buffer_sample(self._h, int(batch or 0), ptrs, _ptr(index_out), int(seed) & (2 ** 64 - 1),
                                                      self._stream()))

    def stats(self) -> dict:
        info = BufferInfo()
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_buffer_stats(self._h, C.byref(info), self._stream()))
        return {k: int(getattr(info, k)) for k, _ in BufferInfo._fields_}

    def set_call_counter(self, value: int):
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_buffer_set_call_counter(self._h, int(value) & 0xFFFFFFFF, self._stream()))


# ---------------------------------------------------------------- trainable layer (tdmpc2_layer_*)
LAYER_CALLS = 0  # library layer calls made through the wrappers below (forward + backward): what the tests of the flag count


def layer_desc(kind: int, groups: int, rows: int, in_dim: int, out_dim: int, shared_x: bool = False, simnorm_dim: int = 0,
               ln_eps: float = 1e-5) -> LayerDesc:
    return LayerDesc(kind=int(kind), groups=int(groups), rows=int(rows), in_dim=int(in_dim), out_dim=int(out_dim),
                     shared_x=int(bool(shared_x)), simnorm_dim=int(simnorm_dim), ln_eps=float(ln_eps))


_UNIT_COUNTER = dict(layer="LAYER_CALLS", loss="LOSS_CALLS", pigrad="PI_GRAD_CALLS", dropout="DROPOUT_CALLS",
                     draw="DRAW_CALLS", task="TASK_CALLS", pixgrad="PIXEL_GRAD_CALLS")


def _unit_check(tag: str, rc: int):
    if rc != 0:
        raise NativeError(f"tdmpc2_{tag} error {rc}: {load_library().tdmpc2_last_error().decode()}")


def _unit_call(tag: str, symbol: str, desc, first, want, tail, **ts):
    """The one call path of the stateless units (layer, loss, pigrad, dropout, draw, task, pixgrad): `first` names the device; every tensor of `ts` (the
    C order after the descriptor; None = absent, a c_void_p = a pointer its caller has checked) is contiguous fp32 on it and holds
    what `want` (name -> element count, or None: the library sees pointers only) asks for; then the unit's counter, the call on the
    current stream with `tail` between the tensors and the stream, and the library's error."""
    what, device = symbol[len("tdmpc2_"):], first.device
    if device.type != "cuda":
        raise NativeError(f"{what} runs on an MI355X only (device {device}); there is no CPU fallback")
    for name, t in ts.items():
        if t is None or type(t) is C.c_void_p:
            continue
        if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
            raise NativeError(f"{what}: {name} must be a contiguous fp32 tensor on {device} (got {t.dtype}, {t.device}, "
                              f"contiguous={t.is_contiguous()})")
    for name, t in ts.items() if want else ():
        if t is not None and type(t) is not C.c_void_p and t.numel() != want[name]:
            raise NativeError(f"{what}: {name} holds {t.numel()} floats, the descriptor asks for {want[name]}")
    globals()[_UNIT_COUNTER[tag]] += 1
    with torch.cuda.device(device):
        ptrs = [t if t is None or type(t) is C.c_void_p else t.data_ptr() for t in ts.values()]
        rc = getattr(load_library(), symbol)(C.byref(desc), *ptrs, *tail, torch.cuda.current_stream(device).cuda_stream)
    _unit_check(tag, rc)


def _nbytes(t) -> int:
    return 0 if t is None else t.numel() * t.element_size()


def layer_workspace_bytes(desc: LayerDesc) -> int:
    n = C.c_size_t()
    _unit_check("layer", load_library().tdmpc2_layer_workspace_bytes(C.byref(desc), C.byref(n)))
    return int(n.value)


def layer_forward(desc: LayerDesc, x, w, b, ln_w=None, ln_b=None, mask=None, y=None, pre=None, stat=None):
    """tdmpc2_layer_forward on the current stream; tensors are contiguous fp32 on one GPU (checked), outputs are written in place."""
    _unit_call("layer", "tdmpc2_layer_forward", desc, x, None, (), x=x, w=w, b=b, ln_w=ln_w, ln_b=ln_b, mask=mask, y=y, pre=pre,
               stat=stat)


def layer_backward(desc: LayerDesc, x, w, ln_w, ln_b, pre, stat, mask, dy, dx=None, dw=None, db=None, dln_w=None, dln_b=None, ws=None):
    """tdmpc2_layer_backward on the current stream; `ws` is a uint8 tensor of at least layer_workspace_bytes(desc) bytes."""
    _unit_call("layer", "tdmpc2_layer_backward", desc, dy, None, (_ptr(ws), _nbytes(ws)), x=x, w=w, ln_w=ln_w, ln_b=ln_b, pre=pre,
               stat=stat, mask=mask, dy=dy, dx=dx, dw=dw, db=db, dln_w=dln_w, dln_b=dln_b)


# ---------------------------------------------------------------- optimiser step (tdmpc2_optim_*)
def optim_cfg(segs, lrs, beta1: float, beta2: float, eps: float, max_norm: float, device_index: int = 0):
    """struct tdmpc2_optim_cfg; segs: (device pointer, count, group) per segment, lrs: one per group.  Returns (cfg, keep): the
    arrays the cfg points to live as long as `keep` does."""
    seg_arr = (OptimSeg * max(len(segs), 1))()
    for i, (ptr, count, group) in enumerate(segs):
        seg_arr[i] = OptimSeg(int(ptr) if ptr else None, int(count), int(group), 0)
    lr_arr = (C.c_float * max(len(lrs), 1))(*[float(v) for v in lrs])
    cfg = OptimCfg(device=int(device_index), n_segs=len(segs), n_groups=len(lrs), reserved=0, beta1=float(beta1), beta2=float(beta2),
                   eps=float(eps), max_norm=float(max_norm), lr=lr_arr, segs=seg_arr)
    return cfg, (seg_arr, lr_arr)


def optim_layout(cfg: OptimCfg):
    """tdmpc2_optim_layout -> (offsets per segment, floats per arena).  Host only."""
    lib = load_library()
    offs, total = (C.c_int64 * max(int(cfg.n_segs), 1))(), C.c_int64()
    rc = lib.tdmpc2_optim_layout(C.byref(cfg), offs, C.byref(total))
    if rc != 0:
        raise NativeError(f"tdmpc2_optim error {rc}: {lib.tdmpc2_last_error().decode()}")
    return [int(v) for v in offs[:cfg.n_segs]], int(total.value)


class NativeOptim:
    """Owns one `tdmpc2_optim_t`: gradient clip + Adam over three caller-owned flat fp32 arenas, three launches per step."""

    def __init__(self, segs, lrs, beta1, beta2, eps, max_norm, device: torch.device):
        device = torch.device(device)
        if device.type != "cuda":
            raise NativeError(f"the optimiser step runs on an MI355X only (device {device}); there is no CPU fallback")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.lib = load_library()
        self.device = device
        self._h = C.c_void_p()
        cfg, keep = optim_cfg(segs, lrs, beta1, beta2, eps, max_norm, device.index)
        self.offsets, self.arena_floats = optim_layout(cfg)
        h = C.c_void_p()
        self._check(self.lib.tdmpc2_optim_create(C.byref(cfg), C.byref(h)))
        del keep
        self._h = h

    def _check(self, rc: int):
        if rc != 0:
            raise NativeError(f"tdmpc2_optim error {rc}: {self.lib.tdmpc2_last_error().decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.tdmpc2_optim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _arena(self, name, t):
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.arena_floats:
            raise NativeError(f"optim step: {name} must be a contiguous fp32 tensor of {self.arena_floats} floats on {self.device}")
        return _ptr(t)

    def step(self, grad, exp_avg, exp_avg_sq, zero_grad: bool = True, norm_out: Optional[torch.Tensor] = None):
        """tdmpc2_optim_step on the current stream; norm_out: a one-element fp32 tensor on the device, or None."""
        if norm_out is not None:
            _chk_tensor("norm_out", norm_out, torch.float32, tuple(norm_out.shape), self.device)
            if norm_out.numel() != 1:
                raise NativeError("optim step: norm_out holds one float")
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_optim_step(self._h, self._arena("grad", grad), self._arena("exp_avg", exp_avg),
                                                   self._arena("exp_avg_sq", exp_avg_sq), int(bool(zero_grad)), _ptr(norm_out),
                                                   self._stream()))

    def get_step(self) -> int:
        n = C.c_int64()
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_optim_get_step(self._h, C.byref(n), self._stream()))
        return int(n.value)

    def set_step(self, step: int):
        with torch.cuda.device(self.device):
            self._check(self.lib.tdmpc2_optim_set_step(self._h, int(step), self._stream()))


# ---------------------------------------------------------------- loss seeds (tdmpc2_loss_*)
LOSS_CALLS = 0  # library loss calls made through the wrappers below (forward + backward), kept like LAYER_CALLS


def loss_desc(steps: int, batch: int, latent_dim: int, num_q: int, num_bins: int, episodic: bool, vmin: float, vmax: float,
              bin_size: float, rho: float, consistency_coef: float, reward_coef: float, value_coef: float,
              termination_coef: float) -> LossDesc:
    return LossDesc(steps=int(steps), batch=int(batch), latent_dim=int(latent_dim), num_q=int(num_q), num_bins=int(num_bins),
                    episodic=int(bool(episodic)), vmin=float(vmin), vmax=float(vmax), bin_size=float(bin_size), rho=float(rho),
                    consistency_coef=float(consistency_coef), reward_coef=float(reward_coef), value_coef=float(value_coef),
                    termination_coef=float(termination_coef))


def loss_workspace_bytes(desc: LossDesc) -> int:
    n = C.c_size_t()
    _unit_check("loss", load_library().tdmpc2_loss_workspace_bytes(C.byref(desc), C.byref(n)))
    return int(n.value)


def _loss_want(desc: LossDesc) -> dict:
    """Element counts of the layouts of include/tdmpc2_plan.h (the library sees pointers only)."""
    T, B, L, Q, NB = desc.steps, desc.batch, desc.latent_dim, desc.num_q, desc.num_bins
    return dict(z_pred=T * B * L, next_z=T * B * L, reward_logits=T * B * NB, reward=T * B, q_logits=Q * T * B * NB, td_target=T * B,
                term_logit=T * B, terminated=T * B, d_z_pred=T * B * L, d_reward_logits=T * B * NB, d_q_logits=Q * T * B * NB,
                d_term_logit=T * B, losses=5, step_means=4 * T, grad_total=1)


def loss_forward(desc: LossDesc, z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit=None, terminated=None,
                 losses=None, step_means=None, ws=None):
    """tdmpc2_loss_forward on the current stream; tensors are contiguous fp32 on one GPU (checked); `losses` [5] and `step_means`
    [4, steps] (optional) are written in place; `ws` is a uint8 tensor of at least loss_workspace_bytes(desc) bytes."""
    _unit_call("loss", "tdmpc2_loss_forward", desc, z_pred, _loss_want(desc), (_ptr(ws), _nbytes(ws)), z_pred=z_pred, next_z=next_z,
               reward_logits=reward_logits, reward=reward, q_logits=q_logits, td_target=td_target, term_logit=term_logit,
               terminated=terminated, losses=losses, step_means=step_means)


def loss_backward(desc: LossDesc, z_pred, next_z, reward_logits, reward, q_logits, td_target, term_logit=None, terminated=None,
                  grad_total=None, d_z_pred=None, d_reward_logits=None, d_q_logits=None, d_term_logit=None):
    """tdmpc2_loss_backward on the current stream; `grad_total` is a one-element fp32 tensor on the device or None (= 1); the
    outputs that are not None are overwritten."""
    _unit_call("loss", "tdmpc2_loss_backward", desc, z_pred, _loss_want(desc), (), z_pred=z_pred, next_z=next_z,
               reward_logits=reward_logits, reward=reward, q_logits=q_logits, td_target=td_target, term_logit=term_logit,
               terminated=terminated, grad_total=grad_total, d_z_pred=d_z_pred, d_reward_logits=d_reward_logits, d_q_logits=d_q_logits,
               d_term_logit=d_term_logit)


# ---------------------------------------------------------------- policy loss seeds (tdmpc2_pigrad_*, include/tdmpc2_pi_grad.h)
PI_GRAD_CALLS = 0  # library calls made through the wrappers below (forward + backward), kept like LOSS_CALLS


def pigrad_desc(steps: int, batch: int, action_dim: int, num_bins: int, multitask: bool, vmin: float, vmax: float, rho: float,
                entropy_coef: float, log_std_min: float, log_std_dif: float) -> PiGradDesc:
    return PiGradDesc(steps=int(steps), batch=int(batch), action_dim=int(action_dim), num_bins=int(num_bins),
                      multitask=int(bool(multitask)), vmin=float(vmin), vmax=float(vmax), rho=float(rho),
                      entropy_coef=float(entropy_coef), log_std_min=float(log_std_min), log_std_dif=float(log_std_dif))


def _pigrad_want(desc: PiGradDesc) -> dict:
    """Element counts of the layouts of include/tdmpc2_pi_grad.h (the library sees pointers only)."""
    T, B, A, NB = desc.steps, desc.batch, desc.action_dim, desc.num_bins
    return dict(pi_out=T * B * 2 * A, eps=T * B * A, action_mask=B * A, action=T * B * A, entropy=T * B, scaled_entropy=T * B,
                d_action=T * B * A, d_scaled_entropy=T * B, d_pi_out=T * B * 2 * A, q_logits=2 * T * B * NB, q=T * B, scale=1,
                losses=3, step_means=T, grad_total=1, d_q_logits=2 * T * B * NB)


def pigrad_head_forward(desc: PiGradDesc, pi_out, eps, action_mask=None, action=None, entropy=None, scaled_entropy=None):
    """tdmpc2_pigrad_head_forward: pi_out [T, B, 2A], eps [T, B, A], action_mask [B, A] (multitask) -> action [T, B, A], entropy and
    scaled_entropy [T, B], written in place."""
    _unit_call("pigrad", "tdmpc2_pigrad_head_forward", desc, pi_out, _pigrad_want(desc), (), pi_out=pi_out, eps=eps,
               action_mask=action_mask, action=action, entropy=entropy, scaled_entropy=scaled_entropy)


def pigrad_head_backward(desc: PiGradDesc, pi_out, eps, action_mask=None, d_action=None, d_scaled_entropy=None, d_pi_out=None):
    """tdmpc2_pigrad_head_backward: the incoming gradients (None = zero, not both) -> d_pi_out [T, B, 2A], overwritten."""
    _unit_call("pigrad", "tdmpc2_pigrad_head_backward", desc, pi_out, _pigrad_want(desc), (), pi_out=pi_out, eps=eps,
               action_mask=action_mask, d_action=d_action, d_scaled_entropy=d_scaled_entropy, d_pi_out=d_pi_out)


def pigrad_value_forward(desc: PiGradDesc, q_logits, q):
    """tdmpc2_pigrad_value_forward: q_logits [2, T, B, NB] -> q [T, B] = the average of two_hot_inv of the two heads."""
    _unit_call("pigrad", "tdmpc2_pigrad_value_forward", desc, q_logits, _pigrad_want(desc), (), q_logits=q_logits, q=q)


def pigrad_loss_forward(desc: PiGradDesc, q, entropy, scaled_entropy, scale, losses, step_means=None):
    """tdmpc2_pigrad_loss_forward: -> losses [3] (pi_loss, mean entropy, mean scaled_entropy) and step_means [T] (optional); `scale`
    is a one-element fp32 tensor on the device (RunningScale.value)."""
    _unit_call("pigrad", "tdmpc2_pigrad_loss_forward", desc, q, _pigrad_want(desc), (), q=q, entropy=entropy,
               scaled_entropy=scaled_entropy, scale=scale, losses=losses, step_means=step_means)


def pigrad_loss_backward(desc: PiGradDesc, q_logits, scale, grad_total=None, d_q_logits=None, d_scaled_entropy=None):
    """tdmpc2_pigrad_loss_backward: `grad_total` is a one-element fp32 tensor on the device or None (= 1); the outputs that are not
    None are overwritten."""
    _unit_call("pigrad", "tdmpc2_pigrad_loss_backward", desc, q_logits, _pigrad_want(desc), (), q_logits=q_logits, scale=scale,
               grad_total=grad_total, d_q_logits=d_q_logits, d_scaled_entropy=d_scaled_entropy)


# ---------------------------------------------------------------- dropout masks (tdmpc2_dropout_mask, include/tdmpc2_dropout.h)
DROPOUT_CALLS = 0  # library calls made through the wrapper below, kept like PI_GRAD_CALLS


def dropout_desc(n: int, p: float, seed: int = 0, call: int = 0) -> DropoutDesc:
    """n elements at drop probability p; `seed` is the 64-bit Philox key, `call` the 64-bit call counter (read only when the call is
    given no device counter)."""
    seed, call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
    return DropoutDesc(n=int(n), p=float(p), seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, call_lo=call & 0xFFFFFFFF,
                       call_hi=call >> 32, reserved=0)


def dropout_mask(desc: DropoutDesc, state, out):
    """tdmpc2_dropout_mask on the current stream: `out` (contiguous fp32 on the GPU, at least desc.n elements, 16-byte aligned) is
    overwritten with dropout's multipliers.  `state`: None (the descriptor's call counter is used) or two int32 words on the same
    device holding the counter, which the call advances by one in stream order.  No host read, no synchronisation."""
    if out.numel() < desc.n:
        raise NativeError(f"dropout_mask: mask holds {out.numel()} floats, the descriptor asks for {desc.n}")
    if state is not None and (state.device != out.device or state.dtype != torch.int32 or state.numel() != 2
                              or not state.is_contiguous()):
        raise NativeError(f"dropout_mask: state must be two contiguous int32 words on {out.device} (got {state.dtype}, {state.device}, "
                          f"{state.numel()} elements)")
    _unit_call("dropout", "tdmpc2_dropout_mask", desc, out, None, (), state=_ptr(state), mask=out)


# ---------------------------------------------------------------- draws of a training step (tdmpc2_draw_noise, include/tdmpc2_draw.h)
DRAW_CALLS = 0  # library calls made through the wrapper below, kept like DROPOUT_CALLS
DRAW_KEY_HI = 0x44524157  # "DRAW": the high key word of autograd.Draws, which keeps its stream apart from DropoutMasks' (seed, 0)


def draw_desc(n: int, num_q: int = 0, seed: int = 0, call: int = 0) -> DrawDesc:
    """n normals and (where the call is given a pair buffer) a pair out of num_q heads; `seed` is the 64-bit Philox key, `call` the
    64-bit call counter (read only when the call is given no device counter)."""
    seed, call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
    return DrawDesc(n=int(n), num_q=int(num_q), seed_lo=seed & 0xFFFFFFFF, seed_hi=seed >> 32, call_lo=call & 0xFFFFFFFF,
                    call_hi=call >> 32, reserved=0)


def draw_noise(desc: DrawDesc, state, normal=None, pair=None):
    """tdmpc2_draw_noise on the current stream: `normal` (contiguous fp32 on the GPU, at least desc.n elements, 16-byte aligned; None
    with desc.n == 0) is overwritten with standard normals and `pair` (two contiguous int32 words on the same device, or None) with
    an ordered pair of distinct heads out of desc.num_q.  `state`: None (the descriptor's call counter is used) or two int32 words
    on the same device holding the counter, which the call advances by one in stream order.  No host read, no synchronisation."""
    first = normal if normal is not None else pair
    if first is None:
        raise NativeError("draw_noise: both outputs are None")
    if normal is not None and normal.numel() < desc.n:
        raise NativeError(f"draw_noise: normal holds {normal.numel()} floats, the descriptor asks for {desc.n}")
    for name, t in (("state", state), ("pair", pair)):
        if t is not None and (t.device != first.device or t.dtype != torch.int32 or t.numel() != 2 or not t.is_contiguous()):
            raise NativeError(f"draw_noise: {name} must be two contiguous int32 words on {first.device} (got {t.dtype}, {t.device}, "
                              f"{t.numel()} elements)")
    # (the call path checks fp32 tensors; state and pair go as pointers the checks above cover)
    _unit_call("draw", "tdmpc2_draw_noise", desc, first, None, (), state=_ptr(state), normal=normal, pair=_ptr(pair))


# ---------------------------------------------------------------- task conditioning (tdmpc2_task_*, include/tdmpc2_task.h)
TASK_CALLS = 0  # library calls made through the wrappers below (forward + backward + renorm), kept like DRAW_CALLS


def task_desc(steps: int, batch: int, ids_len: int, id_bytes: int, num_tasks: int, x_dim: int, task_dim: int, a_dim: int = 0,
              max_norm: float = 1.0) -> TaskDesc:
    """R = steps * batch rows [x_dim | task_dim | a_dim]; row t * batch + b reads ids[0] (ids_len 1) or ids[b] (ids_len batch);
    max_norm <= 0: the forward does not renorm."""
    return TaskDesc(steps=int(steps), batch=int(batch), ids_len=int(ids_len), id_bytes=int(id_bytes), num_tasks=int(num_tasks),
                    x_dim=int(x_dim), task_dim=int(task_dim), a_dim=int(a_dim), max_norm=float(max_norm), reserved=0)


def _task_ids(what: str, desc: TaskDesc, ids, device):
    """The id list as a checked pointer: contiguous int32 or int64 (as desc.id_bytes says) on `device`, desc.ids_len elements."""
    if device.type != "cuda":
        raise NativeError(f"{what} runs on an MI355X only (device {device}); there is no CPU fallback")
    want = {4: torch.int32, 8: torch.int64}.get(desc.id_bytes)
    if ids.device != device or ids.dtype != want or ids.numel() != desc.ids_len or not ids.is_contiguous():
        raise NativeError(f"{what}: ids must be {desc.ids_len} contiguous {want} words on {device} (got {ids.dtype}, {ids.device}, "
                          f"{ids.numel()} elements)")
    return _ptr(ids)


def _task_want(desc: TaskDesc) -> dict:
    """Element counts of the layouts of include/tdmpc2_task.h (the library sees pointers only)."""
    R, D, T, A = desc.steps * desc.batch, desc.x_dim, desc.task_dim, desc.a_dim
    W = D + T + A
    return dict(table=desc.num_tasks * T, x=R * D, a=R * A, out=R * W, dout=R * W, dx=R * D, da=R * A, dtable=desc.num_tasks * T)


def task_forward(desc: TaskDesc, table, ids, x, a=None, out=None):
    """tdmpc2_task_forward on the current stream: `table` [num_tasks, T] is renormalised in place (the rows `ids` names, when
    desc.max_norm > 0), then out [R, D + T + A] = [x | table[id] | a] is written.  Tensors are contiguous fp32 on one GPU."""
    _unit_call("task", "tdmpc2_task_forward", desc, table, _task_want(desc), (), table=table,
               ids=_task_ids("task_forward", desc, ids, table.device), x=x, a=a, out=out)


def task_backward(desc: TaskDesc, ids, dout, dx=None, da=None, dtable=None):
    """tdmpc2_task_backward on the current stream: dx [R, D] and da [R, A] are copies of dout's blocks, dtable [num_tasks, T] the
    sum of dout's embedding block per task in the header's fixed order (zeros for a task no row names).  The outputs that are not
    None are overwritten."""
    if dx is None and da is None and dtable is None:
        raise NativeError("task_backward: all three outputs are None")
    _unit_call("task", "tdmpc2_task_backward", desc, dout, _task_want(desc), (),
               ids=_task_ids("task_backward", desc, ids, dout.device), dout=dout, dx=dx,
               da=da, dtable=dtable)


def task_renorm(desc: TaskDesc, table, ids):
    """tdmpc2_task_renorm on the current stream: the forward's renorm alone."""
    _unit_call("task", "tdmpc2_task_renorm", desc, table, _task_want(desc), (), table=table,
               ids=_task_ids("task_renorm", desc, ids, table.device))


# ---------------------------------------------------------------- pixel encoder in training (tdmpc2_pixgrad_*, include/tdmpc2_pixel_grad.h)
PIXEL_GRAD_CALLS = 0  # library calls made through the wrappers below (forward + backward), kept like TASK_CALLS
PIX_HW = (841, 169, 36, 16)      # output pixels of layers 0..3
PIX_KERNEL = (7, 5, 3, 3)
_PIX_TABLES = {}                 # device -> the uploaded ShiftAug tap table


def pixgrad_desc(n: int, cin: int, channels: int, obs_dtype: int = 0, seed_is_preact: bool = False) -> PixGradDesc:
    """n images [cin, 64, 64] (obs_dtype 0 uint8, 1 fp32) through the encoder of `channels` channels; seed_is_preact: the backward
    takes dz as the gradient of layer 3's pre-activation and skips the SimNorm backward."""
    return PixGradDesc(n=int(n), cin=int(cin), C=int(channels), obs_dtype=int(obs_dtype), seed_is_preact=int(bool(seed_is_preact)),
                       reserved=0)


def pixgrad_workspace_bytes(desc: PixGradDesc):
    """-> (acts_bytes, fwd_ws_bytes, bwd_ws_bytes) of tdmpc2_pixgrad_workspace_bytes."""
    a, f, b = C.c_size_t(), C.c_size_t(), C.c_size_t()
    _unit_check("pixgrad", load_library().tdmpc2_pixgrad_workspace_bytes(C.byref(desc), C.byref(a), C.byref(f), C.byref(b)))
    return int(a.value), int(f.value), int(b.value)


def pixgrad_shift_table(device) -> torch.Tensor:
    """ShiftAug's 7 x 64 tap table (tdmpc2_pixgrad_shift_table) on `device` as int32 [7, 64, 4] (two indices and the bit patterns of
    two fp32 weights per entry): filled on the host, uploaded once per device and cached."""
    device = torch.device(device)
    if device.type != "cuda":
        raise NativeError(f"pixgrad_shift_table: the table lives on an MI355X (device {device}); there is no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _PIX_TABLES:
        host = torch.empty((7, 64, 4), dtype=torch.int32)
        _unit_check("pixgrad", load_library().tdmpc2_pixgrad_shift_table(C.c_void_p(host.data_ptr())))
        _PIX_TABLES[device] = host.to(device)
    return _PIX_TABLES[device]


def _pixgrad_obs(what: str, desc: PixGradDesc, obs, shift, tab):
    dev = obs.device
    want = torch.uint8 if desc.obs_dtype == 0 else torch.float32
    if obs.dtype != want or tuple(obs.shape) != (desc.n, desc.cin, 64, 64) or not obs.is_contiguous():
        raise NativeError(f"{what}: obs must be a contiguous {want} [{desc.n}, {desc.cin}, 64, 64] tensor (got {obs.dtype}, "
                          f"{tuple(obs.shape)})")
    if shift.dtype != torch.int32 or tuple(shift.shape) != (desc.n, 2) or not shift.is_contiguous() or shift.device != dev:
        raise NativeError(f"{what}: shift must be a contiguous int32 [{desc.n}, 2] tensor on {dev}")
    if tab.dtype != torch.int32 or tab.numel() != 7 * 64 * 4 or not tab.is_contiguous() or tab.device != dev:
        raise NativeError(f"{what}: tab must be pixgrad_shift_table({dev})")
    return _ptr(obs), _ptr(shift), _ptr(tab)


def _pixgrad_four(what: str, desc: PixGradDesc, ts, weights: bool, device, optional: bool = False):
    """Four per-layer tensors as a host array of device pointers -> (c_void_p of the array, the array to keep alive)."""
    arr = (C.c_void_p * 4)()
    for l, t in enumerate(ts):
        if t is None and optional:
            continue
        cin_l = desc.cin if l == 0 else desc.C
        count = desc.C * cin_l * PIX_KERNEL[l] ** 2 if weights else desc.C
        if t is None or t.device != device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != count:
            raise NativeError(f"{what}: layer {l} needs a contiguous fp32 tensor of {count} floats on {device}")
        arr[l] = t.data_ptr()
    return C.cast(arr, C.c_void_p), arr


def pixgrad_forward(desc: PixGradDesc, obs, shift, tab, W, b, fwd_ws, acts):
    """tdmpc2_pixgrad_forward on the current stream: W / b the four Conv2d weights and biases, fwd_ws and acts fp32 tensors of at least
    the sizes of pixgrad_workspace_bytes; acts is written (the outputs of layers 0..2 per image, then z [n, 16 C])."""
    what, dev = "pixgrad_forward", acts.device
    ab, fb, _ = pixgrad_workspace_bytes(desc)
    if _nbytes(acts) < ab or _nbytes(fwd_ws) < fb:
        raise NativeError(f"{what}: acts / fwd_ws hold {_nbytes(acts)} / {_nbytes(fwd_ws)} bytes, {ab} / {fb} needed")
    po, ps, pt = _pixgrad_obs(what, desc, obs, shift, tab) if dev.type == "cuda" else (None, None, None)
    Wp, keep_w = _pixgrad_four(what, desc, W, True, dev)
    bp, keep_b = _pixgrad_four(what, desc, b, False, dev)
    _unit_call("pixgrad", "tdmpc2_pixgrad_forward", desc, acts, None, (), obs=po, shift=ps, tab=pt, W=Wp, b=bp, fwd_ws=fwd_ws, acts=acts)
    del keep_w, keep_b


def pixgrad_backward(desc: PixGradDesc, obs, shift, tab, W, acts, dz, bwd_ws, dW, db):
    """tdmpc2_pixgrad_backward on the current stream: dW / db are lists of four tensors or None (a layer's pair is given or None
    together); bwd_ws an fp32 tensor of at least pixgrad_workspace_bytes(desc)[2] bytes."""
    what, dev = "pixgrad_backward", acts.device
    ab, _, bb = pixgrad_workspace_bytes(desc)
    if _nbytes(acts) < ab or _nbytes(bwd_ws) < bb:
        raise NativeError(f"{what}: acts / bwd_ws hold {_nbytes(acts)} / {_nbytes(bwd_ws)} bytes, {ab} / {bb} needed")
    if dz.numel() != desc.n * 16 * desc.C:
        raise NativeError(f"{what}: dz holds {dz.numel()} floats, the descriptor asks for {desc.n * 16 * desc.C}")
    po, ps, pt = _pixgrad_obs(what, desc, obs, shift, tab) if dev.type == "cuda" else (None, None, None)
    Wp, keep_w = _pixgrad_four(what, desc, W, True, dev)
    dWp, keep_dw = _pixgrad_four(what, desc, dW, True, dev, optional=True)
    dbp, keep_db = _pixgrad_four(what, desc, db, False, dev, optional=True)
    _unit_call("pixgrad", "tdmpc2_pixgrad_backward", desc, acts, None, (), obs=po, shift=ps, tab=pt, W=Wp, acts=acts, dz=dz,
               bwd_ws=bwd_ws, dW=dWp, db=dbp)
    del keep_w, keep_dw, keep_db
