"""ctypes binding of libs5fxp.so (the C ABI in include/s5fxp.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).  There is no CPU
fallback: if the shared object is missing this module raises, and every op in the package
fails with it.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch-ROCm ships its own libamdhip64; libs5fxp.so links the same SONAME.  Whichever is loaded first is the HIP
# runtime of the process, and the streams / device pointers handed to the C ABI are torch's: torch must come first,
# or the library binds /opt/rocm's runtime and every launch fails with an invalid-handle error.
import torch  # noqa: F401  (load order matters, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
# S5FXP_LIB: developer override to load an experimental build of the same library (tools/build_variant.sh)
LIB_PATH = os.environ.get("S5FXP_LIB") or os.path.join(_HERE, "libs5fxp.so")

I32P = C.POINTER(C.c_int32)
VOIDP = C.c_void_p

S5FXP_OK, S5FXP_EBADARG, S5FXP_ENEGSHIFT, S5FXP_EUNSUPPORTED, S5FXP_EHIP, S5FXP_EWORKSPACE = 0, -1, -2, -3, -4, -5
ST_NEGSHIFT, ST_NEGEXP, ST_WIDE_STATE, ST_WIDE_INPUT, ST_REDO = 1, 2, 4, 8, 16
FWD_DEFER_REDO, FWD_EXACT, FWD_NO_PAIR = 1, 2, 4
STATUS_WORDS = 128
PATH_GENERIC, PATH_FUSED, PATH_STEP, PATH_CLIP = 1, 2, 3, 4   # status[2]
STEP_MAX_ROWS = 32
STREAM_MAX_HOPS = 32
PUSH_FRESH, PUSH_ZEROS, PUSH_FINAL = 1, 2, 4   # s5fxp_push_desc.flags
MODEL_DEFAULT, MODEL_FORCE_DENSE, MODEL_FORCE_CSR, MODEL_FORCE_GENERIC, MODEL_NO_RESID_FOLD, MODEL_NO_RESID_LAZY = 0, 1, 2, 4, 8, 16
MODEL_NO_GATE_EXT = 32


class DenseDesc(C.Structure):
    _fields_ = [("K", C.c_int32), ("M", C.c_int32), ("weight", I32P), ("bias", I32P)] + [
        (n, C.c_int32) for n in ("w_bits", "w_exp", "b_bits", "b_exp", "inp_bits", "inp_exp", "out_bits", "out_exp")]


class SSMDesc(C.Structure):
    _fields_ = [("H", C.c_int32), ("P", C.c_int32)] + [
        (n, I32P) for n in ("A_re", "A_im", "B_re", "B_im", "C_re", "C_im", "D")] + [
        (n, C.c_int32) for n in (
            "A_re_bits", "A_re_exp", "A_im_bits", "A_im_exp", "B_re_bits", "B_re_exp", "B_im_bits", "B_im_exp",
            "C_re_bits", "C_re_exp", "C_im_bits", "C_im_exp", "D_bits", "D_exp",
            "u_bits", "u_exp", "Bu_re_bits", "Bu_re_exp", "Bu_im_bits", "Bu_im_exp",
            "x_re_bits", "x_re_exp", "x_im_bits", "x_im_exp", "y_bits", "y_exp")]


class NormDesc(C.Structure):
    _fields_ = [(n, I32P) for n in ("minus_mean", "invsq_var", "scale", "bias")] + [
        (n, C.c_int32) for n in ("mean_bits", "mean_exp", "invsq_var_bits", "invsq_var_exp", "scale_bits",
                                 "scale_exp", "bias_bits", "bias_exp")]


class LayerDesc(C.Structure):
    _fields_ = [("norm", NormDesc), ("ssm", SSMDesc), ("out2", DenseDesc)] + [
        (n, C.c_int32) for n in ("l_bits", "l_exp", "r_bits", "r_exp", "res_bits", "res_exp", "sig_x_exp",
                                 "sig_y_exp")] + [("lut", C.c_int32 * 8)]


class ModelDesc(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("encoder", DenseDesc), ("layers", C.POINTER(LayerDesc)),
                ("decoder", DenseDesc)]


TRACE_FIELDS = ("pre_s5", "u", "Bu_re", "Bu_im", "xs_re", "xs_im", "ys", "out2", "out2_sigmoid", "post_GLU",
                "residadd")


class LayerTrace(C.Structure):
    _fields_ = [(n, VOIDP) for n in TRACE_FIELDS]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, VOIDP, VOIDP, C.c_int, VOIDP)


class ForwardOpts(C.Structure):
    _fields_ = [("allreduce", ALLREDUCE_FN), ("allreduce_ctx", VOIDP), ("scan_events", C.POINTER(VOIDP)),
                ("flags", C.c_int32), ("state_in", VOIDP), ("state_out", VOIDP), ("groups", C.c_int32),
                ("gate_events", C.POINTER(VOIDP))]


class PushDesc(C.Structure):
    """s5fxp_push_desc: one entry of a ragged push (32 bytes)."""
    _fields_ = [(n, C.c_int32) for n in ("slot", "rows", "flags", "hops", "h4")] + [("reserved", C.c_int32 * 3)]


F32P = C.POINTER(C.c_float)


class FloatFqSite(C.Structure):
    """s5fxp_float_fq_site: one site of a fake-quantised float forward (4 bytes; bits 0: off)."""
    _fields_ = [("bits", C.c_int8), ("exp", C.c_int8), ("mode", C.c_uint8), ("saturate", C.c_uint8)]


class FloatLayerDesc(C.Structure):
    """s5fxp_float_layer_desc: host pointers to one layer's float parameters."""
    _fields_ = [(n, F32P) for n in ("mean", "var", "scale", "bias", "lambda_bar", "B_bar", "C", "D", "w2", "b2")]


class FloatModelDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "d_in", "H", "P", "d_out")] + [
        ("enc_w", F32P), ("enc_b", F32P), ("layers", C.POINTER(FloatLayerDesc)), ("dec_w", F32P), ("dec_b", F32P)]


STAGE_I32, STAGE_F32 = 0, 1   # s5fxp_stage_pair.a_kind
STAGE_RELU_A = 1              # s5fxp_stage_pair.flags
STAGE_MAX_PAIRS = 4096
CLIPS_TRACED_MAX_LAYERS = 8   # s5fxp_model_clips_traced: the kernel-argument table of trace pointers


class StagePair(C.Structure):
    """s5fxp_stage_pair: one pair of strided (nb, rows, cols) boxes (88 bytes)."""
    _fields_ = [("a", VOIDP), ("a_kind", C.c_int32), ("a_exp", C.c_int32), ("b", VOIDP), ("a_stride", C.c_int64 * 3),
                ("b_stride", C.c_int64 * 3), ("nb", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("flags", C.c_int32)]


class StageErrRec(C.Structure):
    """s5fxp_stage_err_rec: the sums of one pair (1104 bytes, 138 8-byte words)."""
    _fields_ = [(n, C.c_uint64) for n in ("n", "n_nonfinite", "n_equal", "n_ref_nonzero")] + [
        (n, C.c_double) for n in ("sum_abs", "sum_sq", "max_abs", "sum_ref_sq", "sum_rel", "max_rel")] + [
        ("hist_abs", C.c_uint64 * 64), ("hist_rel", C.c_uint64 * 64)]


class S5FxpError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP extension has not been built.  Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    i, i64, p = C.c_int, C.c_int64, VOIDP
    sig = {
        "s5fxp_version": (i, []),
        "s5fxp_strerror": (C.c_char_p, [i]),
        "s5fxp_from_fp": (i, [p, p, i64, i, i, i, p]),
        "s5fxp_to_float": (i, [p, p, i64, i, p]),
        "s5fxp_change_cfg": (i, [p, p, i64, i, i, i, i, p]),
        "s5fxp_dense": (i, [p, p, p, p, i64, i, i, i, i, i, i, i, i, i, p]),
        "s5fxp_dense_csr": (i, [p, p, p, p, p, p, i64, i, i, i, i, i, i, i, i, i, p]),
        "s5fxp_add": (i, [p, p, p, i64, i64, i, i, i, i, i, i, i, p]),
        "s5fxp_mul": (i, [p, p, p, i64, i64, i, i, i, i, p]),
        "s5fxp_add_cb": (i, [p, p, p, i64, i64, i, i, i, i, i, p, p, p]),
        "s5fxp_mul_cb": (i, [p, p, p, i64, i64, i, i, i, p, p, p]),
        "s5fxp_relu": (i, [p, p, p, p, i64, p]),
        "s5fxp_sigmoid": (i, [p, p, i64, i, i, i, i, I32P, p]),
        "s5fxp_scan": (i, [p, p, p, p, p, p, i, i, i, i, i, i, i, i, i, i, p]),
        "s5fxp_assoc_scan_c64": (i, [p, p, p, p, p, i, i, i, i, p]),
        "s5fxp_fq_scan_c64": (i, [p, p, p, p, p, p, i, i, i, i, i, p]),
        "s5fxp_stft_frames": (i64, [i64]),
        "s5fxp_stft_mag": (i, [p, i, i64, C.c_float, p, p, p]),
        "s5fxp_mask_istft": (i, [p, p, i, i64, p, p, p]),
        "s5fxp_stft_mag_i16": (i, [p, i, i64, C.c_float, i, i, p, p, p]),
        "s5fxp_mask_istft_i16": (i, [p, p, i, i, i64, p, p, p]),
        "s5fxp_stft_mag_clips": (i, [p, i, i64, p, C.c_float, p, p, p, p]),
        "s5fxp_mask_istft_clips": (i, [p, p, i, i64, p, p, p, p]),
        "s5fxp_score_workspace_bytes": (C.c_size_t, [i, i64]),
        "s5fxp_mask_istft_score": (i, [p, p, p, i, i64, C.c_float, p, p, p, C.c_size_t, p, p, p, p]),
        "s5fxp_mask_istft_score_i16": (i, [p, p, p, i, i, i64, C.c_float, p, p, p, C.c_size_t, p, p, p, p]),
        "s5fxp_score_clips_workspace_bytes": (C.c_size_t, [i, i64]),
        "s5fxp_mask_istft_score_clips": (i, [p, p, p, i, i64, p, C.c_float, p, p, p, C.c_size_t, p, p, p, p]),
        "s5fxp_stream_audio_state_bytes": (C.c_size_t, []),
        "s5fxp_stream_frames": (i64, [i64, i]),
        "s5fxp_stream_out_hops": (i64, [i64, i, i]),
        "s5fxp_stream_stft": (i, [p, i, i, i64, C.c_float, p, p, p]),
        "s5fxp_stream_mask_istft": (i, [p, i, i, i64, i, p, p, p, p]),
        "s5fxp_model_blob_bytes": (C.c_size_t, [C.POINTER(ModelDesc)]),
        "s5fxp_model_create": (i, [C.POINTER(ModelDesc), p, C.c_size_t, i, p, C.POINTER(p)]),
        "s5fxp_model_destroy": (None, [p]),
        "s5fxp_workspace_bytes": (C.c_size_t, [p, i, i]),
        "s5fxp_model_forward": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p]),
        "s5fxp_model_forward_f32": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p]),
        "s5fxp_workspace_bytes_f32": (C.c_size_t, [p, i, i]),
        "s5fxp_model_forward_i16": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p]),
        "s5fxp_workspace_bytes_i16": (C.c_size_t, [p, i, i]),
        "s5fxp_layer_forward": (i, [p, i, p, i, i, i, i, p, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p]),
        "s5fxp_model_layer_out_bits": (i, [p, i]),
        "s5fxp_model_live_states": (i, [p, i]),
        "s5fxp_model_out_exp": (i, [p]),
        "s5fxp_model_out_bits": (i, [p]),
        "s5fxp_model_is_fast": (i, [p]),
        "s5fxp_model_recurrence_kernel": (i, [p, i]),
        "s5fxp_model_recurrence_xmax": (i, [p, i]),
        "s5fxp_model_step_ok": (i, [p, i, i]),
        "s5fxp_model_step": (i, [p, p, i, i, i, i, i, p, p, p, p, p]),
        "s5fxp_model_step_f32": (i, [p, p, i, i, i, i, i, p, p, p, p, p]),
        "s5fxp_push_desc_check": (i, [p, i, i, i, i, i]),
        "s5fxp_model_step_ragged": (i, [p, p, i, i, i, i, i, p, p, p, i, p, p]),
        "s5fxp_model_step_ragged_f32": (i, [p, p, i, i, i, i, i, p, p, p, i, p, p]),
        "s5fxp_clips_workspace_bytes": (C.c_size_t, [p, i, i]),
        "s5fxp_model_clips_ok": (i, [p, i]),
        "s5fxp_model_clips": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, p]),
        "s5fxp_model_clips_f32": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, p]),
        "s5fxp_stream_stft_ragged": (i, [p, i, i, p, C.c_float, p, i, p, p]),
        "s5fxp_stream_mask_istft_ragged": (i, [p, i, i, p, p, i, p, p, p]),
        "s5fxp_float_model_blob_bytes": (C.c_size_t, [C.POINTER(FloatModelDesc)]),
        "s5fxp_float_model_pack": (i, [C.POINTER(FloatModelDesc), p, C.c_size_t]),
        "s5fxp_float_model_create": (i, [C.POINTER(FloatModelDesc), p, C.c_size_t, p, C.POINTER(p)]),
        "s5fxp_float_model_destroy": (None, [p]),
        "s5fxp_float_workspace_bytes": (C.c_size_t, [p, i, i, i]),
        "s5fxp_float_trace_bytes": (C.c_size_t, [p, i, i]),
        "s5fxp_float_model_forward": (i, [p, p, i, i, p, p, p, p, C.c_size_t, p]),
        "s5fxp_float_model_forward_hist": (i, [p, p, i, i, p, p, p, p, p, C.c_size_t, p]),
        "s5fxp_float_model_clips": (i, [p, p, i, i, p, p, p, p, p, C.c_size_t, p]),
        "s5fxp_float_model_forward_fq": (i, [p, p, i, i, p, p, p, p, p, C.c_size_t, p]),
        "s5fxp_float_model_clips_fq": (i, [p, p, i, i, p, p, p, p, p, C.c_size_t, p]),
        "s5fxp_stage_err_workspace_bytes": (C.c_size_t, [i]),
        "s5fxp_stage_err": (i, [C.POINTER(StagePair), i, p, p, C.c_size_t, p]),
        "s5fxp_model_clips_traced": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, C.POINTER(LayerTrace), p]),
        "s5fxp_model_clips_traced_f32": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, C.POINTER(LayerTrace), p]),
        "s5fxp_float_model_clips_traced": (i, [p, p, i, i, p, p, p, p, p, p, C.c_size_t, p]),
        "s5fxp_stage_err_clips_workspace_bytes": (C.c_size_t, [i]),
        # pairs_host: an array of verify.StagePairClips (s5fxp_stage_pair_clips, 120 bytes)
        "s5fxp_stage_err_clips": (i, [p, i, p, p, C.c_size_t, p]),
        # stated exponents: the namesake's arguments with exps (host int32 array, 5 * n_layers) in front of the stream
        "s5fxp_model_exp_max": (i, [p, i, i]),
        "s5fxp_model_exps_check": (i, [p, p]),
        "s5fxp_model_step_at": (i, [p, p, i, i, i, i, i, p, p, p, p, p, p]),
        "s5fxp_model_step_at_f32": (i, [p, p, i, i, i, i, i, p, p, p, p, p, p]),
        "s5fxp_model_step_ragged_at": (i, [p, p, i, i, i, i, i, p, p, p, i, p, p, p]),
        "s5fxp_model_step_ragged_at_f32": (i, [p, p, i, i, i, i, i, p, p, p, i, p, p, p]),
        "s5fxp_model_clips_at": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, p, p]),
        "s5fxp_model_clips_at_f32": (i, [p, p, i, i, i, i, p, p, p, p, p, C.c_size_t, p, p, p]),
        "s5fxp_model_forward_at": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p, p]),
        "s5fxp_model_forward_at_f32": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p, p]),
        "s5fxp_model_forward_at_i16": (i, [p, p, i, i, i, i, p, p, C.c_size_t, p, C.POINTER(LayerTrace), C.POINTER(ForwardOpts), p, p]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here means the .so is stale: rebuild
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()
EXPORTED_SYMBOLS = ("s5fxp_version s5fxp_strerror s5fxp_from_fp s5fxp_to_float s5fxp_change_cfg s5fxp_dense s5fxp_dense_csr s5fxp_add "
                    "s5fxp_mul s5fxp_add_cb s5fxp_mul_cb s5fxp_relu s5fxp_sigmoid s5fxp_scan s5fxp_assoc_scan_c64 s5fxp_fq_scan_c64 s5fxp_model_blob_bytes "
                    "s5fxp_model_create s5fxp_model_destroy s5fxp_workspace_bytes s5fxp_model_forward s5fxp_model_forward_f32 s5fxp_workspace_bytes_f32 s5fxp_model_forward_i16 s5fxp_workspace_bytes_i16 s5fxp_layer_forward s5fxp_model_layer_out_bits s5fxp_model_live_states "
                    "s5fxp_model_out_exp s5fxp_model_out_bits s5fxp_model_is_fast s5fxp_model_recurrence_kernel s5fxp_model_recurrence_xmax "
                    "s5fxp_model_step_ok s5fxp_model_step s5fxp_model_step_f32 "
                    "s5fxp_stft_frames s5fxp_stft_mag s5fxp_mask_istft s5fxp_stft_mag_i16 s5fxp_mask_istft_i16 s5fxp_score_workspace_bytes s5fxp_mask_istft_score "
                    "s5fxp_mask_istft_score_i16 s5fxp_stream_audio_state_bytes s5fxp_stream_frames "
                    "s5fxp_stream_out_hops s5fxp_stream_stft s5fxp_stream_mask_istft "
                    "s5fxp_push_desc_check s5fxp_model_step_ragged s5fxp_model_step_ragged_f32 s5fxp_stream_stft_ragged "
                    "s5fxp_stream_mask_istft_ragged "
                    "s5fxp_clips_workspace_bytes s5fxp_model_clips_ok s5fxp_model_clips s5fxp_model_clips_f32 "
                    "s5fxp_stft_mag_clips s5fxp_mask_istft_clips s5fxp_score_clips_workspace_bytes s5fxp_mask_istft_score_clips "
                    "s5fxp_float_model_blob_bytes s5fxp_float_model_pack s5fxp_float_model_create s5fxp_float_model_destroy "
                    "s5fxp_float_workspace_bytes s5fxp_float_trace_bytes s5fxp_float_model_forward "
                    "s5fxp_float_model_forward_hist s5fxp_float_model_clips "
                    "s5fxp_float_model_forward_fq s5fxp_float_model_clips_fq "
                    "s5fxp_stage_err_workspace_bytes s5fxp_stage_err "
                    "s5fxp_model_clips_traced s5fxp_model_clips_traced_f32 s5fxp_float_model_clips_traced "
                    "s5fxp_stage_err_clips_workspace_bytes s5fxp_stage_err_clips "
                    "s5fxp_model_exp_max s5fxp_model_exps_check s5fxp_model_step_at s5fxp_model_step_at_f32 "
                    "s5fxp_model_step_ragged_at s5fxp_model_step_ragged_at_f32 s5fxp_model_clips_at s5fxp_model_clips_at_f32 "
                    "s5fxp_model_forward_at s5fxp_model_forward_at_f32 s5fxp_model_forward_at_i16").split()


def check(rc: int, what: str = "") -> None:
    """Maps C-ABI error codes onto the exceptions the reference raises for the same condition."""
    if rc == S5FXP_OK:
        return
    msg = f"{what}: {lib.s5fxp_strerror(rc).decode()}" if what else lib.s5fxp_strerror(rc).decode()
    if rc == S5FXP_ENEGSHIFT:
        raise ValueError(msg)  # fxparray.py:619-621
    if rc == S5FXP_EUNSUPPORTED:
        raise NotImplementedError(msg)
    raise S5FxpError(msg)
