"""ctypes binding of libnsd_hip.so (C ABI: include/nsd.h).

The library is the product: there is NO CPU or eager-PyTorch fallback.  If the shared object is
missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("NSD_LIB", "libnsd_hip.so"))   # NSD_LIB=libnsd_hip_prof.so: diagnostic build
CSRC = os.path.join(_HERE, "csrc")

NSD_FLAG_RESIDUAL = 1
NSD_FLAG_TRAIN = 2
NSD_FLAG_BF16 = 4
NSD_FLAG_BIDIR = 8
NSD_FLAG_MODEL_P = 16     # nsd_multi_train_fwd / _fwd_soft / _bwd only: rng[m].p_lstm / p_head per model (hyper-parameter grids)
# honoured by the DIAGNOSTIC build only (csrc/nsd_diag.h, libnsd_hip_diag.so); the product library rejects them
NSD_DIAG_FLAG_NO_L2_EXCHANGE = 16
NSD_DIAG_FLAG_SPREAD_GROUPS = 32
NSD_DIAG_FLAG_NO_FUSED_LAYERS = 64
NSD_DIAG_FLAG_LOSE_MEMBER = 128


class Rng(C.Structure):
    """nsd_rng of include/nsd.h"""
    _fields_ = [("seed", C.c_uint64), ("base_stream", C.c_uint32), ("p_lstm", C.c_float), ("p_head", C.c_float)]


class Aug(C.Structure):
    """nsd_aug of include/nsd.h"""
    _fields_ = [("max_shift", C.c_int32), ("scale_range", C.c_float), ("p_channel", C.c_float), ("noise_std", C.c_float)]


NSD_AUG_ZSCORE = 1


class Mix(C.Structure):
    """nsd_mix of include/nsd.h"""
    _fields_ = [("mix", C.c_float), ("smoothing", C.c_float)]


class CropCfg(C.Structure):
    """nsd_crop_cfg of include/nsd.h: window W, crops per trial R, hop (0: drawn offsets), in samples"""
    _fields_ = [("window", C.c_int32), ("crops", C.c_int32), ("hop", C.c_int32)]


NSD_CROP_MAX = 64


class Opt(C.Structure):
    """nsd_opt of include/nsd.h"""
    _fields_ = ([(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale", "max_norm")]
                + [(n, C.c_int32) for n in ("sched", "warmup_steps", "total_steps", "step_size")]
                + [("min_ratio", C.c_float), ("gamma", C.c_float)])


class OptRecord(C.Structure):
    """nsd_opt_record of include/nsd.h"""
    _fields_ = [("norm", C.c_float), ("coef", C.c_float), ("lr", C.c_float), ("skipped", C.c_uint32)]


NSD_SCHED = {"constant": 0, "cosine": 1, "step": 2}


class Avg(C.Structure):
    """nsd_avg of include/nsd.h"""
    _fields_ = [("mode", C.c_int32), ("decay", C.c_float), ("start_step", C.c_int32), ("every", C.c_int32)]


NSD_AVG = {"ema": 1, "swa": 2}


class Sam(C.Structure):
    """nsd_sam of include/nsd.h"""
    _fields_ = [("rho", C.c_float)]


class SamRecord(C.Structure):
    """nsd_sam_record of include/nsd.h"""
    _fields_ = [("norm", C.c_float), ("scale", C.c_float), ("nonfinite", C.c_uint32), ("pad", C.c_uint32)]


class NsdError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "T", "C", "H", "L", "K", "F")]


class StreamLayout(C.Structure):
    """nsd_stream_layout of include/nsd.h: float offsets inside one slot of a stream state"""
    _fields_ = ([("h", C.c_int64 * 8), ("c", C.c_int64 * 8)]
                + [(n, C.c_int64) for n in ("pool_max", "pool_den", "pool_acc", "steps", "stride")])


class Window(C.Structure):
    """nsd_window of include/nsd.h: window and hop of a sliding-window decoder, in samples"""
    _fields_ = [("window", C.c_int32), ("hop", C.c_int32)]


class WindowLayout(C.Structure):
    """nsd_window_layout of include/nsd.h: float offsets inside one stream of a window state"""
    _fields_ = [(n, C.c_int64) for n in ("phases", "phase_stride", "window", "hop", "count", "stream_stride")]


NSD_WINDOW_MAX_PHASES = 128


class Fit(C.Structure):
    """nsd_fit of include/nsd.h: the settings of one nsd_head_fit call"""
    _fields_ = ([("epochs", C.c_int32), ("train", C.c_uint32)]
                + [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "scale")])


class FitLayout(C.Structure):
    """nsd_fit_layout of include/nsd.h: float offsets inside one model's fit state"""
    _fields_ = [(n, C.c_int64) for n in ("m", "v", "epochs", "status", "stride")]


NSD_FIT_MAX_TRIALS, NSD_FIT_MAX_EPOCHS = 256, 65536
NSD_FIT_LN, NSD_FIT_FC0, NSD_FIT_FC3 = 1, 2, 4


class Select(C.Structure):
    """nsd_select of include/nsd.h: the early-stopping rule of one nsd_multi_eval call"""
    _fields_ = [("metric", C.c_int32), ("patience", C.c_int32), ("min_delta", C.c_float)]


class EvalRecord(C.Structure):
    """nsd_eval_record of include/nsd.h: one model's held-out metrics"""
    _fields_ = ([("loss_sum", C.c_double)] + [(n, C.c_int32) for n in ("n", "correct", "nonfinite", "pad")]
                + [("confusion", (C.c_int32 * 8) * 8)])


class SelectRecord(C.Structure):
    """nsd_select_record of include/nsd.h: one model's best evaluation, patience count and stop flag"""
    _fields_ = ([("best_loss", C.c_double)] + [(n, C.c_int32) for n in ("best_correct", "best_n", "best_eval", "evals", "bad")]
                + [(n, C.c_uint32) for n in ("stopped", "status", "pad")])


NSD_SELECT_LOSS, NSD_SELECT_ACC, NSD_EVAL_MAX_K = 0, 1, 8
NSD_SELECT = {"loss": NSD_SELECT_LOSS, "acc": NSD_SELECT_ACC}


class Prep(C.Structure):
    """nsd_prep of include/nsd.h"""
    _fields_ = [("flags", C.c_uint32), ("n_sections", C.c_int32), ("sos", (C.c_float * 5) * 4), ("alpha", C.c_float), ("var0", C.c_float)]


class PrepLayout(C.Structure):
    """nsd_prep_layout of include/nsd.h: float offsets inside one slot of a prep state"""
    _fields_ = [(n, C.c_int64) for n in ("x0", "z", "mu", "var", "steps", "stride")]


NSD_PREP_MAX_SECTIONS, NSD_PREP_BASELINE, NSD_PREP_CAR = 4, 1, 2


class Resample(C.Structure):
    """nsd_resample of include/nsd.h: out / in rate = L / M, P taps per phase"""
    _fields_ = [("L", C.c_int32), ("M", C.c_int32), ("P", C.c_int32)]


class ResampleLayout(C.Structure):
    """nsd_resample_layout of include/nsd.h: offsets inside one slot of a resample state, in 4-byte words"""
    _fields_ = [(n, C.c_int64) for n in ("hist", "n_in", "stride")]


class Gate(C.Structure):
    """nsd_gate of include/nsd.h"""
    _fields_ = [("rail", C.c_float), ("jump", C.c_float), ("flat_eps", C.c_float), ("flat_samples", C.c_int32), ("pp", C.c_float),
                ("pp_samples", C.c_int32), ("hold_samples", C.c_int32), ("max_bad", C.c_int32), ("flags", C.c_uint32)]


class GateLayout(C.Structure):
    """nsd_gate_layout of include/nsd.h: offsets inside one slot of a gate state, in 4-byte words"""
    _fields_ = [(n, C.c_int64) for n in ("prev", "held", "run", "hang", "ring", "bad", "rejected", "steps", "stride")]


NSD_GATE_MAX_SPAN, NSD_GATE_ZERO = 64, 1


class Whiten(C.Structure):
    """nsd_whiten of include/nsd.h"""
    _fields_ = [("shrinkage", C.c_float), ("floor", C.c_float), ("min_steps", C.c_int32)]


class WhitenRecord(C.Structure):
    """nsd_whiten_record of include/nsd.h: one group's fit (64 bytes)"""
    _fields_ = [("steps", C.c_int64), ("skipped", C.c_int64), ("trace_mean", C.c_double), ("eig_min", C.c_double), ("eig_max", C.c_double),
                ("sweeps", C.c_int32), ("status", C.c_uint32), ("accumulators", C.c_int32), ("ignored", C.c_int32), ("reserved", C.c_int64)]


class CovLayout(C.Structure):
    """nsd_cov_layout of include/nsd.h: offsets inside one slot of a cov state, in 8-byte words"""
    _fields_ = [(n, C.c_int64) for n in ("sum", "count", "skipped", "stride")]


class SpatialFitCfg(C.Structure):
    """nsd_spatial_fit of include/nsd.h"""
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "decay")]


class SpatialFitLayout(C.Structure):
    """nsd_spatial_fit_layout of include/nsd.h: offsets inside one matrix's slot of a fit state, in bytes"""
    _fields_ = [(n, C.c_int64) for n in ("m", "v", "step", "skipped", "status", "stride")]


NSD_SPATIAL_FIT_NONFINITE = 1
NSD_WHITEN_MAX_SWEEPS = 40
NSD_WHITEN_FEW, NSD_WHITEN_NONFINITE, NSD_WHITEN_CLIPPED, NSD_WHITEN_NOT_CONVERGED = 1, 2, 4, 8


class WsLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("hseq", "cseq", "gact", "inseq", "top", "alpha", "pooled", "fc0_pre",
                                          "dscore", "dpooled", "loss", "adpack", "slabs", "n_slabs", "hslabs", "da_seq", "din", "total")]


# every symbol include/nsd.h declares: name -> (restype, argtypes)
_fp, _vp, _ip = C.c_void_p, C.c_void_p, C.c_void_p   # device pointers travel as integers
_dp = C.POINTER(Dims)
SYMBOLS = {
    "nsd_version": (C.c_int, []),
    "nsd_last_error": (C.c_char_p, []),
    "nsd_param_count": (C.c_int64, [C.c_int32] * 5),
    "nsd_param_layout": (C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_int64)]),
    "nsd_workspace_bytes": (C.c_int64, [_dp, C.POINTER(WsLayout)]),
    "nsd_fast_path": (C.c_int, [_dp]),
    "nsd_zscore_fwd": (C.c_int, [_fp, _fp, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "nsd_infer_scratch_bytes": (C.c_int64, [_dp]),
    "nsd_infer": (C.c_int, [_dp, _fp, _fp, C.c_uint32, _fp, _fp, _vp, _vp]),
    "nsd_lstm_fwd": (C.c_int, [_dp, _fp, _fp, _fp, C.c_uint32, _fp, C.c_int64, _vp]),
    "nsd_head_fwd": (C.c_int, [_dp, _fp, _fp, _fp, _fp, C.c_int64, _fp, _fp, _vp]),
    "nsd_head_bwd": (C.c_int, [_dp, _fp, _fp, _fp, _fp, _fp, _ip, C.c_float, _fp, C.c_int64, _vp]),
    "nsd_head_train": (C.c_int, [_dp, _fp, _fp, _fp, _ip, C.c_float, _fp, C.c_int64, _fp, _vp]),
    "nsd_lstm_head_train": (C.c_int, [_dp, _fp, _fp, _fp, _fp, _fp, _ip, C.c_float, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_rng_path": (C.c_int, [_dp]),
    "nsd_lstm_head_train_rng": (C.c_int, [_dp, _fp, _fp, _vp, _ip, C.c_float, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_lstm_bwd_rng": (C.c_int, [_dp, _fp, _fp, _vp, C.c_uint32, _fp, C.c_int64, _vp]),
    "nsd_dx_path": (C.c_int, [_dp]),
    "nsd_lstm_bwd": (C.c_int, [_dp, _fp, _fp, _fp, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_grad_reduce": (C.c_int, [_dp, _fp, C.c_int64, _fp, C.c_int32, _vp]),
    "nsd_grad_reduce_adam": (C.c_int, [_dp, _fp, C.c_int64, _fp, _fp, _fp, _fp] + [C.c_float] * 6 + [C.c_int32, _vp]),
    "nsd_loss_sum": (C.c_int, [_dp, _fp, C.c_int64, _fp, _vp]),
    "nsd_adam_step": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp] + [C.c_float] * 6 + [C.c_int32, _vp]),
    "nsd_adam_step_guarded": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp] + [C.c_float] * 6 + [C.c_int32, _fp, _vp]),
    "nsd_dropout_mask": (C.c_int, [C.c_uint64, C.c_uint32, C.c_float, C.c_int64, _fp, _vp]),
    "nsd_rrelu_noise": (C.c_int, [C.c_uint64, C.c_uint32, C.c_int64, _fp, _vp]),
    "nsd_step_counter_inc": (C.c_int, [_vp, _vp]),
    "nsd_train_masks_dev": (C.c_int, [C.c_uint64, _vp, C.c_float, C.c_float, C.c_int64, _fp, C.c_int64, _fp, _fp, _vp]),
    "nsd_adam_step_dev": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp] + [C.c_float] * 6 + [_vp, _vp]),
    "nsd_gemm_bf16": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp, C.c_int64, C.c_int32, C.c_int64, _vp, C.c_int64, C.c_int32, _fp,
                                C.c_int32, C.c_int32, C.c_int64, C.c_int32, _vp]),
    "nsd_seq_param_count": (C.c_int64, [C.c_int32] * 6),
    "nsd_seq_param_layout": (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int64)]),
    "nsd_seq_supported": (C.c_int, [_dp, C.c_uint32]),
    "nsd_seq_workspace_bytes": (C.c_int64, [_dp, C.c_uint32]),
    "nsd_seq_infer": (C.c_int, [_dp, _fp, _fp, C.c_uint32, _fp, _fp, _vp, C.c_int64, _vp]),
    "nsd_seq_train_fwd": (C.c_int, [_dp, _fp, _fp, _vp, _ip, C.c_float, C.c_uint32, _vp, C.c_int64, _fp, _vp]),
    "nsd_seq_train_bwd": (C.c_int, [_dp, _fp, _vp, C.c_uint32, _vp, C.c_int64, _fp, _vp]),
    "nsd_seq_loss_sum": (C.c_int, [_dp, C.c_uint32, _vp, C.c_int64, _fp, _vp]),
    "nsd_seq_train_fwd_logits": (C.c_int, [_dp, _fp, _fp, _vp, C.c_uint32, _vp, C.c_int64, _fp, _vp]),
    "nsd_seq_head_bwd": (C.c_int, [_dp, _fp, _vp, _fp, C.c_uint32, _vp, C.c_int64, _vp]),
    "nsd_seq_train_bwd_dx": (C.c_int, [_dp, _fp, _vp, C.c_uint32, _vp, C.c_int64, _fp, _fp, _vp]),
    "nsd_seq_workspace_init": (C.c_int, [_vp, C.c_int64, _vp]),
    "nsd_seq_status": (C.c_int, [_vp, C.POINTER(C.c_int32), _vp]),
    "nsd_seq_guard": (C.c_int, [_vp, _fp, _vp]),
    "nsd_train_masks": (C.c_int, [C.c_uint64, C.c_uint32, C.c_float, C.c_float, C.c_int64, _fp, C.c_int64, _fp, _fp, _vp]),
    # trial augmentation for the trainers
    "nsd_augment_path": (C.c_int, [_dp]),
    "nsd_augment": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _vp, _vp, _vp, C.c_uint32, _fp, _vp]),
    # soft targets (label smoothing, class weights, mixup, distillation)
    "nsd_mixup": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _ip, _fp, _vp, _vp, _vp, _fp, _fp, _vp]),
    "nsd_head_train_soft": (C.c_int, [_dp, _fp, _fp, _fp, _fp, C.c_float, _fp, C.c_int64, _fp, _vp]),
    "nsd_lstm_head_train_soft": (C.c_int, [_dp, _fp, _fp, _fp, _fp, _fp, _vp, _fp, C.c_float, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_multi_train_fwd_soft": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, _vp, _fp, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_seq_train_fwd_soft": (C.c_int, [_dp, _fp, _fp, _vp, _fp, C.c_float, C.c_uint32, _vp, C.c_int64, _fp, _vp]),
    # cropped training: windows cut from the trials of a step, the trial's decision pooled from its windows'
    "nsd_crop_path": (C.c_int, [_dp, C.POINTER(CropCfg)]),
    "nsd_crop": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, C.POINTER(CropCfg), _vp, _vp, _ip, _fp, _fp, _ip, _fp, _ip, _vp]),
    "nsd_crop_pool": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, _ip, _fp, _fp, _vp]),
    # the step's batch gathered on the device from the resident trials and the run's index schedule
    "nsd_gather_path": (C.c_int, [_dp, C.c_int32, C.c_int32, C.c_int32]),
    "nsd_gather": (C.c_int, [_dp, C.c_int32, C.c_int32, _fp, _ip, _fp, _ip, C.c_int32, C.c_int64, _vp, C.c_int64, _fp, _ip, _fp, _ip, _vp]),
    # model-batched H = 48 path (several models per launch)
    "nsd_multi_path": (C.c_int, [_dp, C.c_int32]),
    "nsd_multi_workspace_bytes": (C.c_int64, [_dp, C.c_int32, C.POINTER(WsLayout)]),
    "nsd_multi_train_fwd": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, _vp, _ip, C.c_uint32, _fp, C.c_int64, _fp, _vp]),
    "nsd_multi_train_bwd": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, _vp, C.c_uint32, _fp, C.c_int64, _vp]),
    "nsd_multi_grad_reduce": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _vp]),
    "nsd_multi_grad_reduce_adam": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp, _fp] + [C.c_float] * 6 + [C.c_int32, _vp]),
    # global-norm clipping and learning-rate schedules in the step tail
    "nsd_lr_factor": (C.c_double, [_vp, C.c_int64]),
    "nsd_opt_state_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "nsd_opt_state_init": (C.c_int, [_vp, C.c_int64, _vp]),
    "nsd_grad_reduce_clip_adam": (C.c_int, [_dp, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp]),
    "nsd_grad_norm": (C.c_int, [C.c_int64, _fp, C.c_float, _vp, C.c_int64, _vp]),
    "nsd_adam_step_clip": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _fp, _vp, C.c_int64, _vp]),
    "nsd_multi_grad_reduce_clip_adam": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp]),
    "nsd_multi_loss_sum": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _vp]),
    # input gradients of M frozen models (ensemble saliency, the shared spatial fit)
    "nsd_multi_dx_path": (C.c_int, [_dp, C.c_int32]),
    "nsd_multi_train_bwd_dx": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, C.c_uint32, _fp, C.c_int64, _fp, C.c_int32, _vp]),
    "nsd_multi_loss_mean": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _vp]),
    # per-model step settings (hyper-parameter grids): the `_each` twins take M entries of nsd_aug / nsd_mix / nsd_opt
    "nsd_multi_hyper_path": (C.c_int, [_dp, C.c_int32]),
    "nsd_augment_each": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _vp, _vp, _vp, C.c_uint32, _fp, _vp]),
    "nsd_mixup_each": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _ip, _fp, _vp, _vp, _vp, _fp, _fp, _vp]),
    "nsd_multi_grad_reduce_clip_adam_each": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp]),
    # weight averaging in the update launch: each `_avg` twin takes its twin's arguments, then avg, avg_state, avg_state_bytes
    "nsd_avg_state_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "nsd_avg_state_init": (C.c_int, [_vp, C.c_int64, C.c_int32, _vp]),
    "nsd_grad_reduce_clip_adam_avg": (C.c_int, [_dp, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int64]),
    "nsd_adam_step_clip_avg": (C.c_int, [C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _fp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int64]),
    "nsd_multi_grad_reduce_clip_adam_avg": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp,
                                                      _vp, _vp, C.c_int64]),
    "nsd_multi_grad_reduce_clip_adam_avg_each": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp,
                                                           _vp, _vp, C.c_int64]),
    # sharpness-aware minimisation: the ascent between the two passes of a step (the tail's first launch, then sam_ascend_kernel)
    "nsd_sam_state_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "nsd_sam_state_init": (C.c_int, [_vp, C.c_int64, _vp]),
    "nsd_sam_ascend": (C.c_int, [_dp, _fp, C.c_int64, _fp, _fp, _vp, C.c_float, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "nsd_multi_sam_ascend": (C.c_int, [_dp, C.c_int32, _fp, C.c_int64, _fp, _fp, _vp, C.c_int32, _vp, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "nsd_sam_ascend_flat": (C.c_int, [C.c_int64, _fp, _fp, _vp, C.c_float, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "nsd_multi_infer_scratch_bytes": (C.c_int64, [_dp, C.c_int32]),
    "nsd_multi_infer": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, C.c_uint32, _fp, _fp, _vp, _vp]),
    # early stopping for model batches: metrics, the best-evaluation decision and the snapshot in one launch
    "nsd_multi_eval_path": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64]),
    "nsd_select_state_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "nsd_select_state_init": (C.c_int, [_vp, C.c_int64, C.c_int32, C.c_int64, _vp]),
    "nsd_multi_eval": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _fp, _ip, C.POINTER(C.c_int32), _vp, C.POINTER(Select), _fp, C.c_int64,
                                 _vp, C.c_int64, _vp]),
    # resumable H = 48 inference (streams decoded chunk by chunk)
    "nsd_stream_path": (C.c_int, [_dp]),
    "nsd_stream_state_bytes": (C.c_int64, [_dp, C.c_int32]),
    "nsd_stream_state_layout": (C.c_int, [_dp, C.POINTER(StreamLayout)]),
    "nsd_stream_reset": (C.c_int, [_dp, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_stream_step": (C.c_int, [_dp, _fp, _fp, _ip, C.c_uint32, _vp, C.c_int64, C.c_int32, _fp, _fp, _vp]),
    # resumable inference of M models per launch (an ensemble decoding live streams)
    "nsd_multi_stream_path": (C.c_int, [_dp, C.c_int32]),
    "nsd_multi_stream_state_bytes": (C.c_int64, [_dp, C.c_int32, C.c_int32]),
    "nsd_multi_stream_step": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, _ip, C.c_uint32, _vp, C.c_int64, C.c_int32, _fp, _fp, _fp, _vp]),
    # session calibration: the pooled vector of stream slots, the read-out refitted on frozen features in one launch
    "nsd_stream_features": (C.c_int, [_dp, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _fp, _vp]),
    "nsd_head_fit_path": (C.c_int, [_dp, C.c_int32]),
    "nsd_head_fit_state_bytes": (C.c_int64, [_dp, C.c_int32]),
    "nsd_head_fit_state_layout": (C.c_int, [_dp, C.POINTER(FitLayout)]),
    "nsd_head_fit": (C.c_int, [_dp, C.c_int32, _fp, _fp, C.c_int64, _fp, C.POINTER(Fit), _vp, _vp, C.c_int64, _fp, _vp]),
    # sliding-window decisions for continuous streams
    "nsd_window_path": (C.c_int, [_dp, C.POINTER(Window)]),
    "nsd_window_rows": (C.c_int32, [C.c_int32, C.POINTER(Window)]),
    "nsd_window_state_bytes": (C.c_int64, [_dp, C.POINTER(Window), C.c_int32]),
    "nsd_window_state_layout": (C.c_int, [_dp, C.POINTER(Window), C.POINTER(WindowLayout)]),
    "nsd_window_reset": (C.c_int, [_dp, C.POINTER(Window), _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_window_step": (C.c_int, [_dp, C.POINTER(Window), _fp, _fp, _ip, C.c_uint32, _vp, C.c_int64, C.c_int32, _fp, _fp, _vp, _ip, _vp]),
    # sliding-window decisions of M models per launch (an ensemble on continuous streams)
    "nsd_multi_window_path": (C.c_int, [_dp, C.POINTER(Window), C.c_int32]),
    "nsd_multi_window_state_bytes": (C.c_int64, [_dp, C.POINTER(Window), C.c_int32, C.c_int32]),
    "nsd_multi_window_step": (C.c_int, [_dp, C.POINTER(Window), C.c_int32, _fp, _fp, C.c_int64, _ip, C.c_uint32, _vp, C.c_int64, C.c_int32,
                                        _fp, _fp, _fp, _vp, _ip, _vp]),
    # causal front end for live streams and their training
    "nsd_prep_path": (C.c_int, [C.c_int32, _vp]),
    "nsd_prep_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "nsd_prep_state_layout": (C.c_int, [C.c_int32, C.POINTER(PrepLayout)]),
    "nsd_prep_reset": (C.c_int, [C.c_int32, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_prep_step": (C.c_int, [_dp, _vp, _fp, _ip, _vp, C.c_int64, C.c_int32, _fp, _vp]),
    # rate conversion: stage 0 of the front end
    "nsd_resample_path": (C.c_int, [C.c_int32, _vp]),
    "nsd_resample_out_steps": (C.c_int64, [_vp, C.c_int64, C.c_int64]),
    "nsd_resample_state_bytes": (C.c_int64, [C.c_int32, _vp, C.c_int32]),
    "nsd_resample_state_layout": (C.c_int, [C.c_int32, _vp, C.POINTER(ResampleLayout)]),
    "nsd_resample_reset": (C.c_int, [C.c_int32, _vp, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_resample_step": (C.c_int, [_dp, _vp, _fp, _fp, _ip, _vp, C.c_int64, C.c_int32, _fp, C.c_int64, _ip, _vp]),
    # signal-quality gate around the front end
    "nsd_gate_path": (C.c_int, [C.c_int32, _vp]),
    "nsd_gate_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "nsd_gate_state_layout": (C.c_int, [C.c_int32, C.POINTER(GateLayout)]),
    "nsd_gate_reset": (C.c_int, [C.c_int32, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_gate_step": (C.c_int, [_dp, _vp, _fp, _ip, _vp, C.c_int64, C.c_int32, _fp, _vp, _vp]),
    "nsd_gate_apply": (C.c_int, [_dp, _vp, _fp, _vp, _fp, _vp]),
    # session alignment: channel covariance, whitening fit, spatial apply
    "nsd_cov_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "nsd_cov_state_layout": (C.c_int, [C.c_int32, C.POINTER(CovLayout)]),
    "nsd_cov_reset": (C.c_int, [C.c_int32, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _vp]),
    "nsd_cov_step": (C.c_int, [_dp, _fp, _vp, _ip, _vp, C.c_int64, C.c_int32, _vp, _vp, _vp]),
    "nsd_whiten_fit": (C.c_int, [C.c_int32, C.POINTER(Whiten), _vp, C.c_int64, _vp, C.c_int64, C.c_int32, _ip, C.c_int32, _fp, _vp, _vp]),
    "nsd_spatial_apply": (C.c_int, [_dp, _fp, _fp, C.c_int32, _ip, _fp, _vp]),
    # supervised session alignment: the apply's backward and the Adam step on the matrix
    "nsd_spatial_bwd_scratch_bytes": (C.c_int64, [_dp]),
    "nsd_spatial_bwd": (C.c_int, [_dp, _fp, _fp, _fp, C.c_int32, _ip, _fp, _fp, _vp, _vp, C.c_int64, _vp]),
    "nsd_spatial_fit_state_bytes": (C.c_int64, [C.c_int32, C.c_int32]),
    "nsd_spatial_fit_state_layout": (C.c_int, [C.c_int32, C.POINTER(SpatialFitLayout)]),
    "nsd_spatial_fit_step": (C.c_int, [C.c_int32, C.c_int32, _fp, _fp, _fp, C.POINTER(SpatialFitCfg), _vp, C.c_int64, _fp, _fp, C.c_int32, _vp]),
}
NSD_MAX_MODELS = 32
NSD_DX_PER_MODEL, NSD_DX_MEAN = 0, 1     # nsd_multi_train_bwd_dx's reduce


class DiagGemm(C.Structure):
    """nsd_diag_gemm of csrc/nsd_diag.h: every field of the bf16 GEMM's arguments and the kernel selector"""
    _fields_ = [("A", _vp), ("B", _vp), ("lda", C.c_int64), ("ldb", C.c_int64), ("a_kmajor", C.c_int32), ("b_kmajor", C.c_int32),
                ("b_shift", C.c_int64), ("b_period", C.c_int64), ("B2", _vp), ("ldb2", C.c_int64), ("b2_shift", C.c_int64),
                ("n_split", C.c_int32), ("epilogue", C.c_int32), ("C", _vp), ("ldc", C.c_int64), ("bias", _fp), ("add", _fp),
                ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int64), ("splits", C.c_int32), ("kernel", C.c_int32)]


# entry points of the diagnostic build only (csrc/nsd_diag.h)
DIAG_SYMBOLS = {
    "nsd_diag_gemm_bf16": (C.c_int, [C.POINTER(DiagGemm), _vp]),
    "nsd_diag_reduce_dw": (C.c_int, [_fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _fp, _vp]),
    "nsd_diag_reduce_db": (C.c_int, [_fp, C.c_int32, C.c_int32, _fp, _fp, _vp]),
    "nsd_seq_profile": (C.c_int, [C.c_int32]),
    "nsd_seq_profile_read": (C.c_int, [C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "nsd_diag_force_fwd48": (C.c_int, [C.c_int32]),
    "nsd_diag_force_bwd48": (C.c_int, [C.c_int32]),
    "nsd_diag_dx": (C.c_int, [_fp, _fp, C.c_int64, _fp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp]),
}
DIAG_LIB_PATH = os.path.join(_HERE, "libnsd_hip_diag.so")


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 with hipcc into libnsd_hip.so (in-tree)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(os.path.dirname(_HERE), "include", "nsd.h"))
    outs = [LIB_PATH] + ([DIAG_LIB_PATH] if os.path.basename(LIB_PATH) == "libnsd_hip.so" else [])
    stale = any((not os.path.exists(o)) or any(os.path.getmtime(s) > os.path.getmtime(o) for s in srcs) for o in outs)
    if force or stale:
        subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load libnsd_hip.so; raise loudly when it is absent (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NsdError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        diag = os.path.basename(LIB_PATH) != "libnsd_hip.so"     # NSD_LIB: profiling / A-B builds, possibly of an older ABI
        for name, (res, args) in SYMBOLS.items():
            if diag and not hasattr(L, name):
                continue
            fn = getattr(L, name)        # AttributeError if the ABI and the header ever diverge
            fn.restype, fn.argtypes = res, args
        if diag and hasattr(L, "nsd_debug_profile_buffer"):      # diagnostic build only; not part of include/nsd.h
            L.nsd_debug_profile_buffer.restype, L.nsd_debug_profile_buffer.argtypes = C.c_int, [_vp]
        if L.nsd_version() < 301 and not diag:
            raise NsdError(f"{LIB_PATH} is ABI v{L.nsd_version()}, this binding needs >= 301: rebuild it")
        _lib = L
    return _lib


_diag = None
_diag_active = False


def diag_lib() -> C.CDLL:
    """libnsd_hip_diag.so: the same kernels, with the diagnostic flag bits and the per-kernel timing entry points of
    csrc/nsd_diag.h.  Test / bench / tools infrastructure -- the product modules never ask for it."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_LIB_PATH):
            raise NsdError(f"{DIAG_LIB_PATH} is missing: `make -C {CSRC}` builds it next to the product library")
        L = C.CDLL(DIAG_LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(DIAG_SYMBOLS.items()):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _diag = L
    return _diag


class diagnostic_library:
    """`with diagnostic_library():` -- every C-ABI call of the block goes to libnsd_hip_diag.so instead of the product
    library (same sources; both can be loaded at once).  Not re-entrant, not for product code."""

    def __enter__(self):
        global _lib, _diag_active
        if _diag_active:
            raise NsdError("diagnostic_library() is not re-entrant")
        lib()
        self._saved, _lib, _diag_active = _lib, diag_lib(), True
        return _lib

    def __exit__(self, *exc):
        global _lib, _diag_active
        _lib, _diag_active = self._saved, False
        return False


def diag_active() -> bool:
    return _diag_active


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise NsdError(f"{what} failed (rc={rc}): {lib().nsd_last_error().decode(errors='replace')}")
