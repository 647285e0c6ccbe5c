"""ctypes binding of csrc/libmaua_hip.so — the C ABI declared in include/maua_hip.h.

The product path has NO CPU or PyTorch fallback: if the library is missing, or a launcher returns non-zero,
this raises.  torch is used only for device memory (``tensor.data_ptr()``) and the current HIP stream.
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmaua_hip.so")
ABI_VERSION = 8


class MauaHipError(RuntimeError):
    pass


class StyleLayer(ctypes.Structure):
    """maua_style_layer_t (include/maua_hip.h)."""

    _fields_ = [
        ("mod_w", c_void_p),
        ("mod_b", c_void_p),
        ("wsq", c_void_p),
        ("cin", c_int),
        ("cout", c_int),
        ("lat_idx", c_int),
        ("s_off", c_int),
        ("d_off", c_int64),
        ("wscale", c_float),
        ("pad_", c_int),
    ]


MAX_NOISE_SLOTS = 32


class FrameSource(ctypes.Structure):
    """maua_frame_source_t (include/maua_hip.h): per-frame sequences resident in HBM + the frame a launch starts at."""

    _fields_ = [
        ("frame0", ctypes.c_int32),
        ("pad_", ctypes.c_int32),
        ("latents", c_void_p),
        ("trunc", c_void_p),
        ("noise", c_void_p * MAX_NOISE_SLOTS),
        ("noise_stride", c_int64 * MAX_NOISE_SLOTS),
    ]


class RandnSlot(ctypes.Structure):
    """maua_randn_slot_t (include/maua_hip.h): one generated noise map sequence of a maua_randn_frames_f32 launch."""

    _fields_ = [("dst", c_void_p), ("hw", ctypes.c_int32), ("slot", ctypes.c_int32)]


NOISE_SYNTH_MAX_TERMS = 4


class NoiseTerm(ctypes.Structure):
    """maua_noise_term_t (include/maua_hip.h): one term of a synthesised noise slot."""

    _fields_ = [("bank", c_void_p), ("envelope", c_void_p), ("mask", c_void_p), ("period", ctypes.c_int32), ("phase", ctypes.c_int32)]


class NoiseSynthSlot(ctypes.Structure):
    """maua_noise_synth_slot_t (include/maua_hip.h): the recipe of one noise slot of a maua_noise_synth_f32 launch."""

    _fields_ = [("dst", c_void_p), ("hw", ctypes.c_int32), ("slot", ctypes.c_int32), ("n_terms", ctypes.c_int32), ("gain", c_float),
                ("seed", ctypes.c_uint64), ("term", NoiseTerm * NOISE_SYNTH_MAX_TERMS)]


_P = c_void_p
_SIGNATURES = {
    "maua_abi_version": (c_int, []),
    "maua_device_info": (c_int, [POINTER(c_int), POINTER(c_int), c_char_p, c_int]),
    "maua_upfirdn2d_f32": (c_int, [_P, _P, _P] + [c_int] * 14 + [_P]),
    "maua_upfirdn2d_plan_instance": (c_int, [c_int] * 14 + [c_char_p, c_int]),
    "maua_fused_bias_act_f32": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, _P]),
    "maua_fused_bias_act_f16": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, _P]),
    "maua_fused_bias_act_f64": (c_int, [_P, _P, _P, _P, c_int64, c_int, c_int, c_int, c_int, c_float, c_float, _P]),
    "maua_upfirdn2d_f16": (c_int, [_P, _P, _P] + [c_int] * 14 + [_P]),
    "maua_upfirdn2d_f64": (c_int, [_P, _P, _P] + [c_int] * 14 + [_P]),
    "maua_frame_source_seek": (c_int, [_P, c_int, _P]),
    "maua_randn_frames_f32": (c_int, [_P, c_int, c_int, ctypes.c_uint64, c_int, _P, _P]),
    "maua_noise_synth_f32": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "maua_blur_noise_act_f32": (c_int, [_P, _P, _P] + [c_int] * 8 + [_P, _P, c_int64, _P, _P, _P, c_int, _P, c_int, _P]),
    "maua_upconv_blur_ok": (c_int, [c_int] * 4),
    "maua_upconv_blur_ws_floats": (c_int64, [c_int] * 5),
    "maua_upconv_blur_f32": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, c_int] + [c_int] * 5 + [c_float, _P, _P]),
    "maua_lowres_ok": (c_int, [c_int] * 5),
    "maua_lowres_ws_floats": (c_int64, [c_int] * 6),
    "maua_upconv_blur_lowres_f32": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, c_int] + [c_int] * 6 + [c_float, _P, _P]),
    "maua_styledconv_rgbpart_lowres_f32": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, _P, c_int]
                                           + [c_int] * 6 + [c_float, _P]),
    "maua_const_conv_ok": (c_int, [c_int] * 4),
    "maua_pack_const_conv_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "maua_const_styledconv_f32": (c_int, [_P, _P, c_int, _P, _P, _P, c_int64, _P, _P, _P, _P, c_float, _P, _P, c_int] + [c_int] * 5 + [c_float, _P]),
    "maua_style_affine_f32": (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, c_int, c_int, _P, c_int, _P, _P]),
    "maua_demod_f32": (c_int, [_P, c_int, c_int, _P, c_int, _P, c_int, _P]),
    "maua_pack_weight_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P]),
    "maua_pack_weight_wino_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_pack_weight_wino43_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_pack_weight_upwino_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_pack_weight_wino2d_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_pack_weight_up2d_floats": (c_int64, [c_int] * 2),
    "maua_pack_weight_up2d_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_modconv_up2d_ok": (c_int, [c_int] * 4),
    "maua_pack_weight_sbf16_bytes": (c_int64, [c_int] * 2),
    "maua_pack_weight_sbf16_f32": (c_int, [_P, _P, c_int, c_int, _P]),
    "maua_modconv_sbf16_ok": (c_int, [c_int] * 4),
    "maua_modconv_sbf16_up_ok": (c_int, [c_int] * 4),
    "maua_modconv_w2d_ok": (c_int, [c_int] * 4),
    "maua_modconv_w2d_mtiles": (c_int, [c_int] * 4),
    "maua_modconv_ws_floats": (c_int64, [c_int] * 6),
    "maua_modconv_last_instance": (c_int, [c_char_p, c_int]),
    "maua_modconv_plan_instance": (c_int, [c_int] * 6 + [c_char_p, c_int]),
    "maua_modconv3x3_f32": (c_int, [_P, _P, _P, c_int, _P, _P] + [c_int] * 6 + [c_float, c_int, _P, c_int64, _P, _P, _P, _P, c_int, _P]),
    "maua_styledconv_torgb_f32": (c_int, [_P, _P, _P, c_int, _P, _P] + [c_int] * 6 + [c_float, _P, c_int64, _P, _P, _P, _P, c_float,
                                          _P, _P, _P, _P, c_int, _P, _P, c_int, _P, _P]),
    "maua_styledconv_torgb_partial_f32": (c_int, [_P, _P, _P, c_int, _P, _P] + [c_int] * 6 + [c_float, _P, c_int64, _P, _P, _P, _P, c_float,
                                                  _P, _P, c_int, _P, _P]),
    "maua_torgb_f32": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "maua_frames_to_u8": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "maua_crop_resize_u8": (c_int, [_P, _P] + [c_int] * 9 + [_P]),
    "maua_rgb_to_yuv420p_u8": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "maua_jpeg_header": (c_int, [c_int] * 4 + [_P, c_int]),
    "maua_jpeg_ws_bytes": (c_int64, [c_int] * 4),
    "maua_jpeg_encode_u8": (c_int, [_P] + [c_int] * 5 + [_P, c_int, _P, c_int64, _P, _P]),
    "maua_temporal_fold_u8": (c_int, [_P, _P, c_int, c_int, c_int64, _P, _P, _P, _P]),
    "maua_frames_to_u16": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "maua_crop_resize_u16": (c_int, [_P, _P] + [c_int] * 9 + [_P]),
    "maua_rgb48_to_yuv_p10": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "maua_frames_to_yuv_p10_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "maua_grade_f32": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P]),
    "maua_grade_to_u8": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, _P]),
    "maua_lens_extract_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, c_int, _P]),
    "maua_lens_blur_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P]),
    "maua_lens_blur_plan": (c_int, [c_int, c_int, c_int, _P, _P]),
    "maua_lens_apply_f32": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_int, _P, c_int, c_int, c_int, _P, _P]),
    "maua_feedback_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P]),
    "maua_feedback_plan": (c_int, [c_int, c_int, c_int, _P, c_int, _P, _P]),
    "maua_feedback_test_grid_cap": (c_int, [c_int]),
    "maua_resample_coeffs": (c_int, [c_int] * 5 + [_P, _P, c_int]),
    "maua_resample_u8": (c_int, [_P, _P] + [c_int] * 9 + [_P, _P, c_int, _P, _P, c_int, _P, _P]),
    "maua_resample_u16": (c_int, [_P, _P] + [c_int] * 9 + [_P, _P, c_int, _P, _P, c_int, _P, _P]),
    "maua_resample_ws_bytes": (c_int64, [c_int] * 8),
    "maua_resample_plan": (c_int, [c_int] * 13 + [c_char_p, c_int]),
    "maua_sg1_epilogue_f32":(c_int, [_P, _P, _P, c_int64, _P, _P, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "maua_temporal_fir_f32": (c_int, [_P, _P, _P, c_int, c_int64, c_int, _P]),
    "maua_stft_power_f32": (c_int, [_P, c_int64, _P, c_int, c_int, _P, c_int, _P]),
    "maua_stft_complex_f32": (c_int, [_P, c_int64, _P, c_int, c_int, _P, _P, c_int, _P]),
    "maua_istft_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, c_int64, _P]),
    "maua_median_filter_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "maua_softmask_apply_f32": (c_int, [_P, _P, _P, _P, c_float, c_float, c_int, _P, _P, c_int64, _P]),
    "maua_resample_f64": (c_int, [_P, c_int, c_int64, _P, c_int, _P]),
    "maua_cqt_mag_f32": (c_int, [_P, c_int64, _P, _P, c_int, c_int, c_float, _P, c_int, _P]),
    "maua_chroma_cens_f32": (c_int, [_P, _P, c_int, c_int, c_int, _P]),
    "maua_nn_median_ws_doubles": (c_int64, [c_int] * 3),
    "maua_nn_median_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "maua_yin_f32": (c_int, [_P, c_int64, c_int, c_int, c_int, c_int, c_float, _P, _P, _P, _P, c_int, _P]),
    "maua_pyin_candidates_f32": (c_int, [_P, c_int, c_int, c_int, _P, c_int, c_float, _P, c_int, _P, _P, _P, _P]),
    "maua_pyin_viterbi_f64": (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_double, c_double, c_double, _P, _P, _P, _P]),
    "maua_tempogram_peak_f32": (c_int, [_P, c_int, _P, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "maua_pulse_synth_f32": (c_int, [_P, _P, c_int, _P, c_int, _P, c_int, _P, _P]),
    "maua_hmm_viterbi_f64": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    "maua_hmm_posterior_f64": (c_int, [_P, _P, _P, c_int, c_int, _P, _P, _P]),
    "maua_bar_lds_bytes": (c_int64, [c_int] * 3),
    "maua_bar_ws_bytes": (c_int64, [c_int] * 4),
    "maua_bar_viterbi_f64": (c_int, [_P, c_int, POINTER(ctypes.c_int32), POINTER(ctypes.c_int32), _P, c_int, POINTER(ctypes.c_int32), c_int,
                                     _P, _P, _P, _P]),
    "maua_sosfilt_default_chunk": (c_int, [c_int]),
    "maua_sosfilt_ws_doubles": (c_int64, [c_int] * 4),
    "maua_sosfilt_plan": (c_int, [c_int] * 4 + [POINTER(ctypes.c_int32)]),
    "maua_sosfilt_f64": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "maua_env_follow_f32": (c_int, [_P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "maua_nmf_kl_f32": (c_int, [_P, _P, _P] + [c_int] * 6 + [c_float, _P]),
    "maua_nmf_kl_div_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_float, _P, _P]),
    "maua_nmf_separate_f32": (c_int, [_P, _P, _P, _P, POINTER(ctypes.c_int32)] + [c_int] * 7 + [_P, _P, _P]),
    "maua_filterbank_f32": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "maua_tempogram_ws_doubles": (c_int64, [c_int] * 2),
    "maua_tempogram_f32": (c_int, [_P, c_int, c_int, _P, _P, _P]),
    "maua_beat_track_f64": (c_int, [_P, c_int, c_int, _P, _P, _P, _P]),
    "maua_beat_sync_f32": (c_int, [_P, c_int, c_int, _P, c_int, c_int, _P, _P]),
    "maua_knn_links_f32": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P]),
    "maua_rec_affinity_f32": (c_int, [_P, c_int, c_float, _P, _P, _P]),
    "maua_perlin3d_f32": (c_int, [_P, _P] + [c_int] * 6 + [_P]),
    "maua_keyframe_blend_f32": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P] + [c_int] * 4 + [_P]),
    "maua_affine_reflect_warp_f32": (c_int, [_P, _P, _P] + [c_int] * 8 + [_P, _P]),
    "maua_affine_reflect_warp_mapped_f32": (c_int, [_P, _P, _P] + [c_int] * 8 + [_P, _P, _P, _P, _P]),
    "maua_bend_point_f32": (c_int, [_P, _P, c_int, c_int, c_int64, c_int, _P, c_int, _P, _P, _P]),
    "maua_bend_morph_f32": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P]),
    "maua_bend_pad_f32": (c_int, [_P, _P] + [c_int] * 9 + [c_float, _P, c_int, _P]),
    "maua_bend_remap_f32": (c_int, [_P, _P] + [c_int] * 6 + [_P, c_int, _P] + [c_int] * 3 + [_P, _P, _P]),
    "maua_graph_begin_capture": (c_int, [_P]),
    "maua_graph_end_capture": (c_int, [_P, POINTER(c_void_p)]),
    "maua_graph_launch": (c_int, [_P, _P]),
    "maua_graph_destroy": (c_int, [_P]),
    "maua_event_create": (c_int, [POINTER(c_void_p)]),
    "maua_event_record": (c_int, [_P, _P]),
    "maua_event_elapsed_ms": (c_int, [_P, _P, POINTER(c_float)]),
    "maua_event_destroy": (c_int, [_P]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGNATURES)


def load():
    """dlopen the library (once) and type every entry point; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MauaHipError(
            f"{LIB_PATH} is missing: build it with `python -m maua_stylegan2_amd.build` "
            "(there is deliberately no CPU / PyTorch fallback for the native ops)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    ver = lib.maua_abi_version()
    if ver != ABI_VERSION:
        raise MauaHipError(f"libmaua_hip.so ABI {ver} != binding ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise MauaHipError(f"{what} failed with code {rc}" + (" (hipError)" if rc > 0 else " (rejected arguments)"))


def stream_ptr(device=None):
    return torch.cuda.current_stream(device).cuda_stream


_I32P = POINTER(ctypes.c_int32)


def call(name, *args, device=None):
    """Launch the native entry ``name`` on the current stream of its tensors' device: the one way the audio modules reach the library.

    ``args`` are the entry's arguments WITHOUT the trailing ``void* stream``; each is converted by its slot in ``_SIGNATURES[name]``:
    a ``void*`` slot takes a contiguous CUDA tensor (passed as ``data_ptr()``), None (NULL) or an int (an address the caller computed,
    passed through unchecked); an ``int32*`` slot takes a contiguous int32 numpy array (a host table); every other slot passes through.
    All tensors must be on one device, which is the launch device; ``device=`` names it when no argument is a tensor and must agree
    with the tensors otherwise.  Every refusal names the entry and the argument position and is raised before any HIP call."""
    slots = _SIGNATURES[name][1]
    if not slots or slots[-1] is not c_void_p:
        raise TypeError(f"{name} takes no stream: it is a host query, call it on load() directly")
    if len(args) + 1 != len(slots):
        raise TypeError(f"{name} takes {len(slots) - 1} arguments before the stream (got {len(args)})")
    dev = None if device is None else torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    conv = []
    for i, (a, slot) in enumerate(zip(args, slots)):
        if slot is c_void_p and isinstance(a, torch.Tensor):
            if not a.is_contiguous():
                raise ValueError(f"{name}: argument {i} must be contiguous (shape {tuple(a.shape)}, strides {a.stride()})")
            if not a.is_cuda:
                raise RuntimeError(f"{name}: argument {i} must be a CUDA (HIP) tensor")
            if dev is None:
                dev = a.device
            elif a.device != dev:
                raise ValueError(f"{name}: argument {i} is on {a.device}, the launch goes to {dev}")
            a = a.data_ptr()
        elif slot is c_void_p and a is not None and not isinstance(a, int):
            raise TypeError(f"{name}: argument {i} must be a tensor, None or an address (got {type(a).__name__})")
        elif slot is _I32P:
            if not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.flags.c_contiguous):
                raise TypeError(f"{name}: argument {i} must be a contiguous int32 numpy array")
            a = a.ctypes.data_as(_I32P)
        conv.append(a)
    if dev is None:
        raise ValueError(f"{name}: no tensor argument names the launch device: pass device=")
    fn = getattr(load(), name)
    with torch.cuda.device(dev):
        check(fn(*conv, stream_ptr(dev)), name)


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def require_cuda_any(t, name):
    """The two native ops accept half / float / double like the reference's dtype dispatch; everything else is fp32."""
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA (HIP) tensor")  # mirrors CHECK_CUDA, op/upfirdn2d.cpp:7
    if t.dtype not in (torch.float16, torch.float32, torch.float64):
        raise RuntimeError(f"{name} must be float16, float32 or float64 (got {t.dtype})")
    return t.contiguous()


DTYPE_SUFFIX = {torch.float16: "f16", torch.float32: "f32", torch.float64: "f64"}


def require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA (HIP) tensor")  # mirrors CHECK_CUDA, op/upfirdn2d.cpp:7
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32 (got {t.dtype}); the MI355X path computes in fp32")
    return t.contiguous()


def device_info():
    lib = load()
    cu, lds = c_int(0), c_int(0)
    buf = ctypes.create_string_buffer(256)
    check(lib.maua_device_info(ctypes.byref(cu), ctypes.byref(lds), buf, 256), "maua_device_info")
    return {"cu_count": cu.value, "lds_bytes": lds.value, "name": buf.value.decode()}


def last_modconv_instance():
    """rocprofv3 name of the kernel instance the last modulated-conv call launched (key of profiles/*_pmc_traffic.json)."""
    buf = ctypes.create_string_buffer(128)
    check(load().maua_modconv_last_instance(buf, 128), "maua_modconv_last_instance")
    return buf.value.decode()


def planned_modconv_instance(batch, cin, cout, h, w, mode):
    """(rc, name): the instance maua_modconv3x3_f32 would launch for the shape in modes 0 .. 4 (rc 0), or its refusal (name None).
    Shapes only, no launch: works without a GPU."""
    buf = ctypes.create_string_buffer(128)
    rc = load().maua_modconv_plan_instance(batch, cin, cout, h, w, mode, buf, 128)
    return rc, (buf.value.decode() if rc == 0 else None)


def planned_upfirdn2d_instance(major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """(rc, name, tiles_x, tiles_y): the instance maua_upfirdn2d_f32 would launch for the geometry ("tile4.wx2", "up2.wx4", "down2.wx1",
    "generic"; "none" for major == 0) and its workgroups per plane (0, 0 where there are no tiles), or its refusal (name None).
    Geometry only, no launch: works without a GPU."""
    buf = ctypes.create_string_buffer(64)
    rc = load().maua_upfirdn2d_plan_instance(major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1,
                                             buf, 64)
    if rc != 0:
        return rc, None, 0, 0
    name, _, tiles = buf.value.decode().partition(" ")
    tiles_x, tiles_y = (int(v) for v in tiles.split("x")) if tiles else (0, 0)
    return rc, name, tiles_x, tiles_y


SOSFILT_PLAN_FIELDS = ("chunk", "nc", "launches", "zero_groups", "final_groups", "tiles", "last_tile", "last_chunk")


def planned_sosfilt(n_filters, n_sections, n, chunk=0):
    """(rc, plan): what maua_sosfilt_f64 would do with these shape arguments, as a dict over SOSFILT_PLAN_FIELDS (rc 0), or its refusal
    (plan None).  Shapes only, no launch: works without a GPU."""
    out = (ctypes.c_int32 * 8)()
    rc = load().maua_sosfilt_plan(n_filters, n_sections, n, chunk, out)
    return rc, (dict(zip(SOSFILT_PLAN_FIELDS, out)) if rc == 0 else None)


RESAMPLE_FILTERS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4}  # MAUA_RESAMPLE_* (include/maua_hip.h)
RESAMPLE_MAX_TAPS = 64


def resample_coeffs(in_size, in0, in1, out_size, filter):
    """(rc, k, bounds): maua_resample_coeffs' tables of one axis as int32 numpy arrays [out_size, ksize] and [out_size, 2] (rc = ksize), or
    its refusal (rc < 0, tables None).  Host only: works without a GPU."""
    filter_id = RESAMPLE_FILTERS.get(filter, -1) if isinstance(filter, str) else int(filter)
    n = max(int(out_size), 1)
    k = np.empty(n * RESAMPLE_MAX_TAPS, np.int32)
    bounds = np.empty((n, 2), np.int32)
    rc = load().maua_resample_coeffs(in_size, in0, in1, out_size, filter_id, k.ctypes.data, bounds.ctypes.data, k.size)
    if rc <= 0:
        return rc, None, None
    return rc, k[: n * rc].reshape(n, rc).copy(), bounds


def planned_resample(sample_bytes, batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, ksize_x, ksize_y, out_misalign=0):
    """(rc, instance, fields): what maua_resample_u8 / _u16 would launch — "fused.u8.vec", "fused.u16.scalar", "twopass.u8", ... and the
    plan's key=value fields as a dict of strings (the fused tile, "64x64", "64x32" or "64x16", under "tile") — or the refusal (instance None).  ksize 0 = a copied axis
    (NULL tables).  Arguments only, no launch: works without a GPU."""
    buf = ctypes.create_string_buffer(128)
    rc = load().maua_resample_plan(sample_bytes, batch, in_h, in_w, out_h, out_w, dst_x0, dst_y0, dst_w, dst_h, ksize_x, ksize_y,
                                   out_misalign, buf, 128)
    if rc != 0:
        return rc, None, {}
    name, *rest = buf.value.decode().split(" ")
    fields = dict(part.split("=") for part in rest if "=" in part)
    fields.update({"tile": part for part in rest if "=" not in part})
    return rc, name, fields


class HipEvent:
    """HIP event on an explicit stream (bench.py roofline timing)."""

    def __init__(self):
        self._h = c_void_p()
        check(load().maua_event_create(ctypes.byref(self._h)), "maua_event_create")

    def record(self, stream=None):
        check(load().maua_event_record(self._h, stream if stream is not None else stream_ptr()), "maua_event_record")

    def elapsed_ms(self, end):
        ms = c_float(0)
        check(load().maua_event_elapsed_ms(self._h, end._h, ctypes.byref(ms)), "maua_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            if self._h:
                load().maua_event_destroy(self._h)
        except Exception:
            pass


class HipGraph:
    """Capture-and-replay of everything launched on the current stream inside the ``with`` block."""

    def __init__(self):
        self._exec = c_void_p()
        self._stream = None

    def __enter__(self):
        self._stream = stream_ptr()
        check(load().maua_graph_begin_capture(self._stream), "maua_graph_begin_capture")
        return self

    def __exit__(self, et, ev, tb):
        rc = load().maua_graph_end_capture(self._stream, ctypes.byref(self._exec))
        if et is None:
            check(rc, "maua_graph_end_capture")
        return False

    def replay(self, stream=None):
        check(load().maua_graph_launch(self._exec, stream if stream is not None else stream_ptr()), "maua_graph_launch")

    def __del__(self):
        try:
            if self._exec:
                load().maua_graph_destroy(self._exec)
        except Exception:
            pass
