"""ctypes binding of libdgtta_hip.so (the C ABI declared in include/dgtta.h).

There is NO CPU fallback: if the library cannot be loaded every op raises.  The library is built in-tree by
`python dg_tta_amd/build.py` (hipcc, gfx950) so that it travels with the repository snapshot.
"""
import ctypes as C
import os
from pathlib import Path

LIB_PATH = Path(__file__).resolve().parent / "libdgtta_hip.so"

_c_float_p = C.POINTER(C.c_float)
P, I, I64, U64, F, SZ = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/dgtta.h one to one
SIGNATURES = {
    "dgtta_version": (I, []),
    "dgtta_last_error": (C.c_char_p, []),
    "dgtta_reload_env": (I, []),
    "dgtta_mind3d_ws_bytes": (SZ, [I, I, I, I]),
    "dgtta_mind3d_fwd": (I, [P, P, F, I, C.POINTER(F), I, P, I, I, I, P, SZ, I, I, I, I, P]),
    "dgtta_mind3d_noise_fill": (I, [P, U64, U64, I, I, I, I, I, P]),
    "dgtta_mind3d_fwd_seeded": (I, [P, U64, U64, I, F, I, C.POINTER(F), I, P, I, I, I, P, SZ, I, I, I, I, P]),
    "dgtta_gin_ws_bytes": (SZ, [I, I, I, I]),
    "dgtta_gin_chain_fwd": (I, [P, P, C.POINTER(I), C.POINTER(P), C.POINTER(P), P, P, SZ, I, I, I, I, P]),
    "dgtta_affine_warp3d_fwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P, P]),
    "dgtta_affine_warp3d_bwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_rf_field_ws_bytes": (SZ, [I, I, I, I]),
    "dgtta_rf_field_fwd": (I, [P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_diffeo_fields_ws_bytes": (SZ, [I, I, I, I]),
    "dgtta_diffeo_fields": (I, [P, F, P, P, P, SZ, I, I, I, I, I, P]),
    "dgtta_dense_warp3d_fwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_dense_warp3d_bwd": (I, [P, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_softdice_ws_bytes": (SZ, [I, I, I64]),
    "dgtta_softdice_fwd": (I, [P, P, P, P, P, SZ, I, I, I64, I, I, I, P]),
    "dgtta_softdice_bwd": (I, [P, P, P, P, P, F, P, I, I, I64, I, I, P]),
    "dgtta_softdice_bwd_t": (I, [P, P, P, P, P, F, P, I, I, I64, I, I, I, P]),
    "dgtta_softdice_probs_fwd": (I, [P, P, P, P, SZ, I, I, I64, I64, I64, I64, P]),
    "dgtta_softdice_probs_bwd": (I, [P, P, P, P, P, P, I, I, I64, I64, I64, I64, P]),
    "dgtta_dice_ce_ws_bytes": (SZ, [I, I, I64]),
    "dgtta_dice_ce_fwd": (I, [P, I, P, P, P, P, SZ, I, I, I64, F, I, P]),
    "dgtta_dice_ce_bwd": (I, [P, I, P, P, F, P, P, I, I, I, I64, P]),
    "dgtta_dice_ce_ds_ws_bytes": (SZ, [I, I, I, I, I]),
    "dgtta_dice_ce_ds_fwd": (I, [P, I, P, P, P, P, SZ, I, I, I, I, I, I, I, I, F, I, P]),
    "dgtta_dice_ce_ds_bwd": (I, [P, I, P, P, F, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_dice_ce_batch_fwd": (I, [P, I, P, P, P, P, SZ, I, I, I64, F, I, I, P]),
    "dgtta_dice_ce_ds_batch_fwd": (I, [P, I, P, P, P, P, SZ, I, I, I, I, I, I, I, I, F, I, I, P]),
    "dgtta_region_loss_ws_bytes": (SZ, [I, I, I64]),
    "dgtta_region_loss_fwd": (I, [P, I, P, P, I, P, P, P, SZ, I, I, I64, F, P]),
    "dgtta_region_loss_batch_fwd": (I, [P, I, P, P, I, P, P, P, SZ, I, I, I64, F, I, P]),
    "dgtta_region_loss_bwd": (I, [P, I, P, P, I, P, F, P, P, I, I, I, I64, P]),
    "dgtta_region_loss_ds_ws_bytes": (SZ, [I, I, I, I, I]),
    "dgtta_region_loss_ds_fwd": (I, [P, I, P, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, F, P]),
    "dgtta_region_loss_ds_batch_fwd": (I, [P, I, P, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, F, I, P]),
    "dgtta_region_loss_ds_bwd": (I, [P, I, P, P, I, P, F, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_region_counts": (I, [P, I, I, P, P, I, P, I64, P]),
    "dgtta_logits_regions": (I, [P, I, I, I64, C.POINTER(I), P, P]),
    "dgtta_feature_head_regions": (I, [P, I64, P, P, P, I, I, I, I64, C.POINTER(I), P, P]),
    "dgtta_adamw_step": (I, [C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(I64), I, F, F, F, F, F,
                             I, F, P, P]),
    "dgtta_grads_nonfinite": (I, [C.POINTER(P), C.POINTER(I64), I, P, P]),
    "dgtta_grad_sumsq_ws_bytes": (SZ, [I64, I]),
    "dgtta_grad_sumsq": (I, [C.POINTER(P), C.POINTER(I64), I, P, P, SZ, P]),
    "dgtta_sgd_step": (I, [C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(I64), I, F, F, F, I, I, F, P, F, P, P]),
    "dgtta_conv3d_packed_bytes": (SZ, [I, I, I]),
    "dgtta_conv3d_pack_weights": (I, [P, P, I, I, I, I, I, P]),
    "dgtta_conv3d_stats_bytes": (SZ, [I, I, I, I, I]),
    "dgtta_conv3d_k3_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_k3_dgrad": (I, [P, I, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_wgrad_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "dgtta_conv3d_wgrad_split_ws_bytes": (SZ, [I, I, I, I, I, I, I]),
    "dgtta_conv3d_k3_wgrad": (I, [P, I, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_k3_blocked_supported": (I, [I, I, I, I, I, I, I]),
    "dgtta_conv3d_k3_fwd_blocked": (I, [P, I64, P, P, P, I, P, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_k3_wgrad_blocked": (I, [P, I64, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_instnorm_ws_bytes": (SZ, [I, I, I64]),
    "dgtta_instnorm_lrelu_fwd": (I, [P, I, P, P, P, P, P, I, P, SZ, I, I, I64, F, F, I, P]),
    "dgtta_instnorm_lrelu_bwd": (I, [P, I, P, I, P, P, P, P, I, P, P, P, SZ, I, I, I64, F, I, I, P]),
    "dgtta_conv3d_k3_dgrad_gstats": (I, [P, I, P, P, I, I, I, I, I, I, I, I, I, P, I, P, P, P, F, P, SZ, C.POINTER(I), I, I, P]),
    "dgtta_instnorm_lrelu_bwd_gstats": (I, [P, I, P, I, P, P, P, P, I, P, P, P, P, SZ, I, I, I64, F, I, I, P]),
    "dgtta_convT3d_fwd_ws_bytes": (SZ, [I, I, I]),
    "dgtta_convT3d_k2s2_fwd": (I, [P, I, P, P, P, I, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_convT3d_bwd_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "dgtta_convT3d_bwd_split_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "dgtta_convT3d_k2s2_bwd": (I, [P, I, P, I, P, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_kpacked_bytes": (SZ, [I, I, I, I]),
    "dgtta_conv3d_kpack_weights": (I, [P, P, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_dgrad": (I, [P, I, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_conv3d_kwgrad_ws_bytes": (SZ, [I, I, I, I, I, I, I, I, I, I]),
    "dgtta_conv3d_wgrad": (I, [P, I, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_convT3d_s_fwd_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "dgtta_convT3d_s_fwd": (I, [P, I, P, P, P, I, P, SZ, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_convT3d_s_bwd_ws_bytes": (SZ, [I, I, I, I, I, I, I, I, I]),
    "dgtta_convT3d_s_bwd": (I, [P, I, P, I, P, P, I, P, P, P, SZ, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_fwd": (I, [P, I, P, P, P, I, P, I, I, I, I, I64, I, P]),
    "dgtta_seghead_bwd_ws_bytes": (SZ, [I, I, I, I64]),
    "dgtta_seghead_bwd": (I, [P, I, P, I, P, P, I, P, I, P, P, P, SZ, I, I, I64, I, I, P]),
    "dgtta_seghead_bwd_acc": (I, [P, I, P, I, P, P, I, P, I, P, P, P, SZ, I, I, I64, I, I, I, P]),
    "dgtta_seghead_warp_supported": (I, [P, I, I, I, I, I, I, I]),
    "dgtta_seghead_warp_bwd_ws_bytes": (SZ, [I, I, I, I, I, I]),
    "dgtta_seghead_warp_fwd": (I, [P, P, P, P, I, P, P, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_warp_bwd": (I, [P, P, P, P, P, P, I, P, P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_warp_bwd_g16": (I, [P, P, P, P, P, P, I, P, P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_warp_bwd_g16_d16": (I, [P, P, P, P, I, P, P, P, P, SZ, I, I, I, I, I, I, I, I, P]),
    "dgtta_instnorm_lrelu_bwd_head": (I, [P, P, P, I, P, I, P, P, P, P, I, P, P, P, SZ, I, I, I64, F, I, I, P]),
    "dgtta_ncdhw_to_ndhwc": (I, [P, P, I, I, I64, I, I, P]),
    "dgtta_ndhwc_to_ncdhw": (I, [P, P, I, I, I64, I, I, P]),
    "dgtta_argmax_dice": (I, [P, I, I, P, P, P, I, I64, P]),
    "dgtta_resample_axis_ws_bytes": (SZ, [I64, I, I64, I]),
    "dgtta_resample_axis": (I, [P, P, P, SZ, I64, I, I, I64, I, P]),
    "dgtta_window_accumulate": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_window_accumulate": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_logits_chunk_f64": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_window_accumulate_t": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_window_accumulate_t": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_argmax_rows": (I, [P, I, I, I64, P, P]),
    "dgtta_feature_window_accumulate": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_feature_window_accumulate_norm": (I, [P, P, P, P, F, P, P, P, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_feature_window_accumulate_multi": (I, [P, P, P, I, P, P, F, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_feature_head_argmax": (I, [P, I64, P, P, P, I, I, I, I64, P, P]),
    "dgtta_feature_logits_chunk_f64": (I, [P, I64, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_logits_chunk_f64_t": (I, [P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_argmax_merge_f64": (I, [P, I64, I, I, P, P, I, P]),
    "dgtta_regions_merge_f64": (I, [P, I64, I, I, C.c_double, C.POINTER(I), I, P, P, I, I, P]),
    "dgtta_feature_head_softmax": (I, [P, I64, P, P, P, I, I, I, I64, C.POINTER(I), I, I, P, P, P, P, P]),
    "dgtta_softmax_merge_f64": (I, [P, I64, I, I, C.c_double, P, P, P, C.POINTER(I), I, P, I, P]),
    "dgtta_softmax_finalize_f64": (I, [P, P, P, P, I64, I, I, P, P, P, P]),
    "dgtta_label_bboxes": (I, [P, P, I, I, I, I, P, P]),
    "dgtta_label_surface": (I, [P, I, I, I, I64, I, I, I, I, I, I, P, P]),
    "dgtta_edt_ws_bytes": (SZ, [I, I, I]),
    "dgtta_edt_sq": (I, [P, P, P, SZ, I, I, I, F, F, F, P]),
    "dgtta_cc_ws_bytes": (SZ, [I, I, I]),
    "dgtta_cc_label": (I, [P, P, I, I, I, I, I, P, P, SZ, P]),
    "dgtta_cc_sizes": (I, [P, I64, P, P]),
    "dgtta_cc_filter": (I, [P, P, I, P, P, I64, I, I, I64, P, P, P, SZ, P]),
    "dgtta_holes_ws_bytes": (SZ, [I, I, I]),
    "dgtta_holes_fill": (I, [P, I, I, I, I, P, P, P, P, SZ, P]),
    "dgtta_holes_member": (I, [P, I, I, I, P, I, I, I, I, I, I, I, P, P]),
    "dgtta_holes_apply": (I, [P, I, I, I, P, P, I, I, I, I, I, I, I64, I64, P, P]),
    "dgtta_nonzero_mask": (I, [P, I, I64, P, P]),
    "dgtta_bspline3_prefilter": (I, [P, P, I, I, I, P]),
    "dgtta_patch_sample_aug": (I, [P, I, I, I, I, I, P, P, P]),
    "dgtta_intensity_stats_ws_bytes": (SZ, [I, I64]),
    "dgtta_intensity_stats": (I, [P, I, I64, C.POINTER(I), I, P, P, SZ, P]),
    "dgtta_intensity_map": (I, [P, P, I, I64, P, I, P, P, P]),
    "dgtta_gauss_blur3": (I, [P, P, P, I, I, I, I, P, I, P]),
    "dgtta_mirror_batch": (I, [P, P, P, P, C.POINTER(I), I, I, I, I, I, P]),
    "dgtta_window_gather": (I, [P, P, C.POINTER(I), C.POINTER(I), I, I, I, I, I, I, I, I, P]),
    "dgtta_feature_window_accumulate_mirror": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_feature_window_accumulate_norm_mirror": (I, [P, P, P, P, F, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_seghead_window_accumulate_mirror_t": (I, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_window_accumulate_mirror_t": (I, [P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, P]),
    "dgtta_fingerprint_ws_bytes": (SZ, [I64, I]),
    "dgtta_fingerprint_sweep": (I, [P, P, I, I64, I, C.c_double, I64, I, I, C.POINTER(C.c_uint32), I, P, P, P, SZ, P]),
}

FP_BINS, FP_MAX_PREFIXES = 2048, 6
SEG_U8, SEG_I16, SEG_I32 = 0, 1, 2


class PatchItem(C.Structure):
    """DgttaPatchItem of include/dgtta.h."""
    _fields_ = [("image", P), ("label", P), ("D", I), ("H", I), ("W", I), ("map", F * 12)]


PATCH_MAX_ITEMS = 16


class IntensityItem(C.Structure):
    """DgttaIntensityItem of include/dgtta.h."""
    _fields_ = [("item", I), ("mode", I), ("negate", I), ("noise_b", I), ("a", F), ("s", F), ("seed_lo", C.c_uint32),
                ("seed_hi", C.c_uint32), ("off_lo", C.c_uint32), ("off_hi", C.c_uint32)]


class BlurItem(C.Structure):
    """DgttaBlurItem of include/dgtta.h."""
    _fields_ = [("item", I), ("radius", I), ("taps", F * 9)]


INTENSITY_MAX_ITEMS = 16
IMAP_LINEAR, IMAP_CONTRAST, IMAP_GAMMA, IMAP_RESTORE = 0, 1, 2, 3

_lib = None
_load_error = None


class DgttaError(RuntimeError):
    pass


def load():
    """Loads the shared library once; raises DgttaError (never falls back) when it is missing."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise DgttaError(_load_error)
    path = os.environ.get("DGTTA_LIB", str(LIB_PATH))
    # PyTorch-ROCm ships its own libamdhip64.so.7; import it first so that this library binds to the SAME HIP runtime
    # instance (same streams / allocations) instead of pulling in /opt/rocm's copy as a second runtime.
    import torch  # noqa: F401
    try:
        lib = C.CDLL(path)
    except OSError as e:
        _load_error = (f"libdgtta_hip.so could not be loaded from {path} ({e}). Build it with "
                       f"`python dg_tta_amd/build.py`; dg_tta_amd has no CPU fallback.")
        raise DgttaError(_load_error) from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().dgtta_last_error().decode(errors="replace")
        raise DgttaError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """Device pointer of a tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream_of(device=None):
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise DgttaError("dg_tta_amd ops run on the MI355X only: got a CPU tensor (there is no CPU fallback)")
