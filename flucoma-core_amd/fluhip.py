"""ctypes binding of libflucoma_hip.so (include/flucoma_hip.h) for the Python-side tests and
bench.py.  The product is the shared library and the C++ client headers; this module is a thin
caller that mirrors the C ABI one to one and FAILS LOUDLY when the library is missing -- there
is no numpy / torch fallback anywhere.
"""
from __future__ import annotations

import ctypes
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLUHIP_LIB: another build of the library (A/B timing of two source states on one GPU box); FLUHIP_AB=1: the build with the
# experiment switches of DESIGN 6b compiled in (build.py build_ab) -- the production library does not read them
LIB_AB_PATH = os.path.join(_HERE, "lib_ab", "libflucoma_hip_ab.so")
LIB_QC_PATH = os.path.join(_HERE, "lib_ab", "libflucoma_hip_qc.so")
LIB_PATH = os.environ.get("FLUHIP_LIB") or (LIB_AB_PATH if os.environ.get("FLUHIP_AB") == "1" else
                                            os.path.join(_HERE, "lib", "libflucoma_hip.so"))

OK, WARNING, ERROR, CANCELLED = 0, 1, 2, 3

_i64 = ctypes.c_int64
_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
_ip = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p
PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, _i64, ctypes.c_void_p)


class MatrixView(ctypes.Structure):
    """fluhip_matrix_view: element (r, c) at data[r * row_stride + c * col_stride] (strides in doubles)"""
    _fields_ = [("data", ctypes.POINTER(ctypes.c_double)), ("rows", _i64), ("cols", _i64), ("row_stride", _i64),
                ("col_stride", _i64)]

    @classmethod
    def of(cls, a):
        """view of a 2-D float64 numpy array with whatever strides it has (a.T, a[::2, 1:], ...)"""
        assert a.dtype == np.float64 and a.ndim == 2 and all(st % 8 == 0 for st in a.strides)
        return cls(ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_double)), a.shape[0], a.shape[1],
                   a.strides[0] // 8, a.strides[1] // 8)

class BufNMFJob(ctypes.Structure):
    """fluhip_bufnmf_job"""
    _fields_ = [("count", _i64), ("n", _i64), ("win", _i64), ("fft", _i64), ("hop", _i64), ("K", _i64), ("iters", _i64),
                ("update_w", ctypes.c_int), ("update_h", ctypes.c_int), ("seed", _i64), ("seeds", _ip),
                ("audio", _fp), ("bases_seed", _fp), ("acts_seed", _fp), ("bases", _fp), ("acts", _fp), ("resynth", _fp)]


EXPORTS = [
    "fluhip_abi_version", "fluhip_device_count", "fluhip_ctx_create", "fluhip_ctx_destroy",
    "fluhip_last_error", "fluhip_ctx_device_info", "fluhip_ctx_stream", "fluhip_ctx_synchronize", "fluhip_ctx_trim", "fluhip_ctx_set_progress_lag",
    "fluhip_fft_params", "fluhip_stft_num_frames", "fluhip_stft_f64", "fluhip_stft_f32",
    "fluhip_nmf_process_f64", "fluhip_nmf_process_views_f64", "fluhip_nmf_process_frames_f64", "fluhip_nndsvd_f64", "fluhip_bufnmfseed_f32",
    "fluhip_bufnmf_channel_f32", "fluhip_bufmelbands_f32", "fluhip_bufmfcc_f32", "fluhip_bufmelbands_padded_f32",
    "fluhip_bufmfcc_padded_f32",
    "fluhip_bufstft_forward_f32", "fluhip_bufstft_inverse_f32",
    "fluhip_corpus_create", "fluhip_corpus_create_ragged", "fluhip_corpus_frames_of", "fluhip_corpus_set_audio_ragged_host",
    "fluhip_corpus_writeback_ragged_host", "fluhip_corpus_resynth_ragged_host",
    "fluhip_corpus_destroy", "fluhip_corpus_frames", "fluhip_corpus_bins",
    "fluhip_corpus_device_bytes", "fluhip_corpus_set_audio_host", "fluhip_corpus_set_audio_dev",
    "fluhip_corpus_stft", "fluhip_corpus_stft_mag_only", "fluhip_corpus_nmf", "fluhip_corpus_set_factors", "fluhip_corpus_writeback_dev",
    "fluhip_corpus_writeback_host", "fluhip_corpus_keep_spectrum", "fluhip_corpus_resynth_dev",
    "fluhip_corpus_resynth_host", "fluhip_corpus_resynth_interleaved_host", "fluhip_corpus_read_f64", "fluhip_corpus_plan", "fluhip_prof_enable",
    "fluhip_prof_reset", "fluhip_prof_read", "fluhip_corpus_debug_words", "fluhip_corpus_update_clocks", "fluhip_corpus_last_loop_ms", "fluhip_last_error_is_out_of_memory", "fluhip_clear_error", "fluhip_debug_plan_lists", "fluhip_debug_plan_tail", "fluhip_debug_plan_kind", "fluhip_debug_plan_h_update", "fluhip_debug_plan_shape", "fluhip_debug_wnorm_form",
    "fluhip_pool_create", "fluhip_pool_destroy", "fluhip_pool_size", "fluhip_pool_device", "fluhip_pool_last_error",
    "fluhip_pool_bufnmf_f32", "fluhip_pool_bufnmf_job_f32", "fluhip_pool_bufnmf_ragged_f32", "fluhip_pool_bufmfcc_f32",
    "fluhip_pool_bufmelbands_f32", "fluhip_shard_range", "fluhip_balanced_assignment", "fluhip_nmfmatch_f32", "fluhip_nmffilter_f32",
    "fluhip_nmfcross_process_f64", "fluhip_griffinlim_f64", "fluhip_bufnmfcross_f32", "fluhip_debug_cross_plan", "fluhip_debug_jacobi_svd_f64",
    "fluhip_novelty_curve_f64", "fluhip_novelty_slices_f64", "fluhip_bufnoveltyslice_f32", "fluhip_bufnoveltyfeature_f32",
    "fluhip_debug_novelty_plan",
    "fluhip_onset_curve_f64", "fluhip_onset_slices_f64", "fluhip_bufonsetslice_f32", "fluhip_bufonsetfeature_f32",
    "fluhip_debug_onset_plan",
    "fluhip_hpss_planes_f64", "fluhip_bufhpss_f32", "fluhip_debug_hpss_plan",
    "fluhip_pitch_frames_f64", "fluhip_debug_pitch_curve_f64", "fluhip_bufpitch_f32", "fluhip_debug_pitch_plan",
    "fluhip_spectralshape_frames_f64", "fluhip_bufspectralshape_f32", "fluhip_debug_chroma_filters_f64",
    "fluhip_chroma_frames_f64", "fluhip_bufchroma_f32", "fluhip_debug_spectral_plan",
    "fluhip_loudness_frames_f64", "fluhip_bufloudness_f32", "fluhip_debug_loudness_plan",
    "fluhip_amp_envelope_f64", "fluhip_amp_slices_f64", "fluhip_bufampslice_f32", "fluhip_bufampfeature_f32",
    "fluhip_debug_amp_plan",
    "fluhip_amp_gate_f64", "fluhip_bufampgate_f32", "fluhip_debug_ampgate_plan",
    "fluhip_debug_features_plan", "fluhip_debug_resynth_f64", "fluhip_debug_corpus_read_layouts_f64",
    "fluhip_debug_cross_stencil_f64", "fluhip_debug_stft_frames_f32", "fluhip_debug_stft_frames_f64",
]


class FluhipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"fluhip status {status}: {message}")
        self.status = status
        self.message = message


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} is missing: build it with `python flucoma-core_amd/build.py` "
            "(there is no fallback implementation)")
    L = ctypes.CDLL(path)
    L.fluhip_abi_version.restype = ctypes.c_int
    L.fluhip_device_count.restype = ctypes.c_int
    L.fluhip_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
    L.fluhip_ctx_destroy.argtypes = [_vp]
    L.fluhip_ctx_destroy.restype = None
    L.fluhip_last_error.argtypes = [_vp]
    L.fluhip_last_error.restype = ctypes.c_char_p
    L.fluhip_ctx_device_info.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p,
                                         ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.fluhip_ctx_stream.argtypes = [_vp]
    L.fluhip_ctx_stream.restype = _vp
    L.fluhip_ctx_synchronize.argtypes = [_vp]
    L.fluhip_ctx_trim.argtypes = [_vp]
    L.fluhip_ctx_set_progress_lag.argtypes = [_vp, ctypes.c_int]
    L.fluhip_fft_params.argtypes = [_i64, _i64, _i64, _ip, _ip, _ip, _ip]
    L.fluhip_stft_num_frames.argtypes = [_i64, _i64, _i64]
    L.fluhip_stft_num_frames.restype = _i64
    L.fluhip_stft_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _dp, _dp, _ip]
    L.fluhip_stft_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _dp, _dp, _ip]
    L.fluhip_debug_resynth_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _dp, _dp, _i64, _dp]
    L.fluhip_debug_stft_frames_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dp, _dp]
    L.fluhip_debug_stft_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dp, _dp]
    L.fluhip_nmf_process_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int,
                                         ctypes.c_int, _i64, _dp, _dp, _dp, _dp, _dp, PROGRESS_FN, _vp]
    _mv = ctypes.POINTER(MatrixView)
    L.fluhip_nmf_process_views_f64.argtypes = [_vp, _mv, _i64, _i64, ctypes.c_int, ctypes.c_int, _i64, _mv, _mv, _mv, _mv, _mv,
                                               PROGRESS_FN, _vp]
    L.fluhip_nmf_process_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _dp, _dp]
    _dbl = ctypes.c_double
    L.fluhip_nndsvd_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, ctypes.c_int, _i64, _dp, _dp, _ip]
    L.fluhip_bufnmfseed_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, ctypes.c_int, _i64,
                                        _fp, _fp, _ip]
    L.fluhip_bufnmf_channel_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                            ctypes.c_int, ctypes.c_int, _i64, _fp, _fp, _fp, _fp,
                                            _fp, PROGRESS_FN, _vp]
    L.fluhip_bufmelbands_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                         ctypes.c_int, ctypes.c_int, _fp, _ip]
    L.fluhip_bufmfcc_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                     _fp, _ip]
    L.fluhip_bufmelbands_padded_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_int, _fp, _ip]
    L.fluhip_bufmfcc_padded_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                            ctypes.c_int, _fp, _ip]
    L.fluhip_bufstft_forward_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _fp, _fp, _ip]
    L.fluhip_bufstft_inverse_f32.argtypes = [_vp, _fp, _fp, _i64, _i64, _i64, _i64, ctypes.c_int, _fp, _ip]
    L.fluhip_nmfcross_process_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                              _dp, PROGRESS_FN, _vp]
    L.fluhip_debug_cross_plan.argtypes = [_vp, _i64, _i64, _i64, _ip]
    L.fluhip_debug_cross_stencil_f64.argtypes = [_vp, _dp, _i64, _i64, ctypes.c_int, _i64, _dp, _dp]
    L.fluhip_debug_jacobi_svd_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _dp, _dp, _dp, _ip]
    L.fluhip_griffinlim_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64]
    L.fluhip_bufnmfcross_f32.argtypes = [_vp, _fp, _i64, _i64, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64,
                                         _i64, _fp, PROGRESS_FN, _vp]
    _u8p = ctypes.POINTER(ctypes.c_ubyte)
    L.fluhip_novelty_curve_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _dp]
    L.fluhip_novelty_slices_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _i64, _u8p, _ip, _dp]
    L.fluhip_bufnoveltyslice_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, ctypes.c_int, _i64, _dbl, _i64, _i64, _i64,
                                             _i64, _i64, _dbl, _ip, _i64, _ip]
    L.fluhip_bufnoveltyfeature_f32.argtypes = [_vp, _fp, _i64, _i64, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, _dbl,
                                               ctypes.c_int, _fp, _ip]
    L.fluhip_debug_novelty_plan.argtypes = [_vp, _i64, _i64, _i64, _ip]
    L.fluhip_onset_curve_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _i64, _i64, _dp, _dp]
    L.fluhip_onset_slices_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _i64, _i64, _dbl,
                                          _i64, _u8p, _ip, _dp]
    L.fluhip_bufonsetslice_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, ctypes.c_int, _dbl, _i64, _i64, _i64, _i64, _i64,
                                           _i64, _ip, _i64, _ip]
    L.fluhip_bufonsetfeature_f32.argtypes = [_vp, _fp, _i64, _i64, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, ctypes.c_int,
                                             _fp, _ip]
    L.fluhip_debug_onset_plan.argtypes = [_vp, _i64, _i64, ctypes.c_int, _i64, _ip]
    L.fluhip_hpss_planes_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _dp, _dp, _dp, _dp,
                                         ctypes.POINTER(_dp)]
    L.fluhip_bufhpss_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _dp, _dp, _fp]
    L.fluhip_debug_hpss_plan.argtypes = [_vp, _i64, _i64, _ip]
    L.fluhip_pitch_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, ctypes.c_int, _dbl, _dbl, _dbl, _dp]
    L.fluhip_debug_pitch_curve_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, ctypes.c_int, _dbl, _dbl, _dbl, _dp]
    L.fluhip_bufpitch_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, _dbl, _dbl,
                                      ctypes.c_int, ctypes.c_int, _dbl, _fp, _ip]
    L.fluhip_debug_pitch_plan.argtypes = [_vp, _i64, _i64, ctypes.c_int, _ip]
    L.fluhip_spectralshape_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl, ctypes.c_int, ctypes.c_int,
                                                  _dbl, _dp]
    L.fluhip_bufspectralshape_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, _dbl, _dbl,
                                              _dbl, ctypes.c_int, ctypes.c_int, _dbl, _fp, _ip]
    L.fluhip_debug_chroma_filters_f64.argtypes = [_vp, _i64, _i64, _dbl, _dbl, _dp]
    L.fluhip_chroma_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _dbl, ctypes.c_int, _dbl, _dbl, _dbl, _dp]
    L.fluhip_bufchroma_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, _i64, _dbl, ctypes.c_int, _dbl,
                                       _dbl, _dbl, _fp, _ip]
    L.fluhip_debug_spectral_plan.argtypes = [_vp, _i64, _i64, ctypes.c_int, _ip]
    L.fluhip_loudness_frames_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, _dbl, _dp]
    L.fluhip_bufloudness_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         _dbl, _fp, _ip]
    L.fluhip_debug_loudness_plan.argtypes = [_vp, _i64, _i64, _dbl, _ip]
    L.fluhip_amp_envelope_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dp]
    L.fluhip_amp_slices_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl, _i64, _dbl,
                                        _u8p, _ip, _dp]
    L.fluhip_bufampslice_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl, _i64, _dbl,
                                         _dbl, _ip, _i64, _ip]
    L.fluhip_bufampfeature_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl, _fp]
    L.fluhip_debug_amp_plan.argtypes = [_vp, _dbl, _ip]
    L.fluhip_amp_gate_f64.argtypes = [_vp, _dp, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _i64, _i64, _i64, _i64, _i64, _i64, _dbl,
                                      _i64, _u8p, _dp]
    L.fluhip_bufampgate_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _i64, _i64, _i64, _i64, _i64, _i64,
                                        _dbl, _dbl, _i64, _ip, _i64, _ip]
    L.fluhip_debug_ampgate_plan.argtypes = [_vp, _ip]
    L.fluhip_debug_features_plan.argtypes = [_vp, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl, _ip]
    L.fluhip_corpus_create.argtypes = [_vp, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(_vp)]
    L.fluhip_corpus_create_ragged.argtypes = [_vp, _i64, _ip, _i64, _i64, _i64, _i64, ctypes.POINTER(_vp)]
    L.fluhip_corpus_frames_of.argtypes = [_vp, _i64]
    L.fluhip_corpus_frames_of.restype = _i64
    L.fluhip_corpus_set_audio_ragged_host.argtypes = [_vp, ctypes.POINTER(_fp)]
    L.fluhip_corpus_writeback_ragged_host.argtypes = [_vp, ctypes.POINTER(_fp), ctypes.POINTER(_fp)]
    L.fluhip_corpus_resynth_ragged_host.argtypes = [_vp, ctypes.POINTER(_fp)]
    L.fluhip_corpus_destroy.argtypes = [_vp]
    L.fluhip_corpus_destroy.restype = None
    for f in ("fluhip_corpus_frames", "fluhip_corpus_bins", "fluhip_corpus_device_bytes"):
        getattr(L, f).argtypes = [_vp]
        getattr(L, f).restype = _i64
    L.fluhip_corpus_set_audio_host.argtypes = [_vp, _fp]
    L.fluhip_corpus_set_audio_dev.argtypes = [_vp, _vp]
    L.fluhip_corpus_stft.argtypes = [_vp]
    L.fluhip_corpus_stft_mag_only.argtypes = [_vp]
    L.fluhip_corpus_nmf.argtypes = [_vp, _i64, ctypes.c_int, ctypes.c_int, _i64, _ip, PROGRESS_FN, _vp]
    L.fluhip_corpus_set_factors.argtypes = [_vp, _fp, _fp]
    L.fluhip_corpus_writeback_dev.argtypes = [_vp, _vp, _vp]
    L.fluhip_corpus_writeback_host.argtypes = [_vp, _fp, _fp]
    L.fluhip_corpus_read_f64.argtypes = [_vp, _dp, _dp, _dp]
    L.fluhip_debug_corpus_read_layouts_f64.argtypes = [_vp, _ip, _dp, _dp, _dp]
    L.fluhip_corpus_plan.argtypes = [_vp, _ip]
    L.fluhip_corpus_keep_spectrum.argtypes = [_vp, ctypes.c_int]
    L.fluhip_corpus_resynth_dev.argtypes = [_vp, _vp]
    L.fluhip_corpus_resynth_host.argtypes = [_vp, _fp]
    L.fluhip_corpus_resynth_interleaved_host.argtypes = [_vp, _fp, _i64]
    L.fluhip_prof_enable.argtypes = [_vp, ctypes.c_int]
    L.fluhip_prof_reset.argtypes = [_vp]
    L.fluhip_prof_read.argtypes = [_vp, ctypes.c_int, _ip, _dp]
    L.fluhip_corpus_debug_words.argtypes = [_vp, _ip]
    L.fluhip_corpus_update_clocks.argtypes = [_vp, _ip, ctypes.c_int]
    L.fluhip_last_error_is_out_of_memory.argtypes = [_vp]
    L.fluhip_last_error_is_out_of_memory.restype = ctypes.c_int
    L.fluhip_clear_error.argtypes = [_vp]
    L.fluhip_clear_error.restype = None
    L.fluhip_debug_plan_shape.argtypes = [_i64, _i64, _i64, _i64, _ip]
    L.fluhip_debug_wnorm_form.argtypes = [ctypes.c_int] * 7
    L.fluhip_corpus_last_loop_ms.argtypes = [_vp, ctypes.POINTER(ctypes.c_double)]
    L.fluhip_debug_plan_lists.argtypes = [_i64, _ip, _i64, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), _i64,
                                          ctypes.POINTER(ctypes.c_int32)]
    L.fluhip_debug_plan_lists.restype = _i64
    L.fluhip_debug_plan_tail.argtypes = [_i64, _i64, _i64, _i64, _ip]
    L.fluhip_debug_plan_kind.argtypes = [_i64, _i64, _i64, _i64]
    L.fluhip_debug_plan_h_update.argtypes = [_i64, _i64, _i64, _i64]
    L.fluhip_pool_create.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_vp)]
    L.fluhip_pool_destroy.argtypes = [_vp]
    L.fluhip_pool_destroy.restype = None
    L.fluhip_pool_size.argtypes = [_vp]
    L.fluhip_pool_device.argtypes = [_vp, ctypes.c_int]
    L.fluhip_pool_last_error.argtypes = [_vp]
    L.fluhip_pool_last_error.restype = ctypes.c_char_p
    L.fluhip_pool_bufmfcc_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                          ctypes.c_int, _fp, _ip]
    L.fluhip_pool_bufmelbands_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _dbl, _dbl, _dbl,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_int, _fp, _ip]
    L.fluhip_pool_bufnmf_f32.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int, ctypes.c_int,
                                         _i64, _ip, _fp, _fp, PROGRESS_FN, _vp]
    L.fluhip_pool_bufnmf_job_f32.argtypes = [_vp, ctypes.POINTER(BufNMFJob), PROGRESS_FN, _vp]
    L.fluhip_pool_bufnmf_ragged_f32.argtypes = [_vp, ctypes.POINTER(_fp), _ip, _i64, _i64, _i64, _i64, _i64, _i64, ctypes.c_int,
                                                ctypes.c_int, _i64, _ip, ctypes.POINTER(_fp), ctypes.POINTER(_fp), PROGRESS_FN, _vp]
    L.fluhip_shard_range.argtypes = [_i64, ctypes.c_int, ctypes.c_int, _ip, _ip]
    L.fluhip_shard_range.restype = None
    L.fluhip_balanced_assignment.argtypes = [_dp, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32)]
    return L


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _f(a):
    return a.ctypes.data_as(_fp) if a is not None else None


def _cb(progress):
    if progress is None:
        return PROGRESS_FN()
    return PROGRESS_FN(lambda it, _u: 1 if progress(int(it)) else 0)


class Context:
    """fluhip_ctx: one device, one stream."""

    def __init__(self, device: int = 0, lib: ctypes.CDLL | None = None):
        self.lib = lib or load_library()
        h = _vp()
        rc = self.lib.fluhip_ctx_create(device, ctypes.byref(h))
        if rc != OK:
            raise FluhipError(rc, f"cannot create context on device {device} "
                                  f"({self.lib.fluhip_device_count()} HIP devices visible)")
        self.h = h

    def close(self):
        if self.h:
            # a corpus must not outlive its context (its device buffers are freed on the context's stream)
            for ref in list(getattr(self, "_corpora", [])):
                c = ref()
                if c is not None:
                    c.close()
            self.lib.fluhip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, allow=(OK,)):
        if rc not in allow:
            raise FluhipError(rc, self.lib.fluhip_last_error(self.h).decode())
        return rc

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        arch = ctypes.create_string_buffer(256)
        cus = ctypes.c_int(0)
        self._check(self.lib.fluhip_ctx_device_info(self.h, name, 256, arch, 256, ctypes.byref(cus)))
        return name.value.decode(), arch.value.decode(), cus.value

    def synchronize(self):
        self._check(self.lib.fluhip_ctx_synchronize(self.h))

    def set_progress_lag(self, lag):
        self._check(self.lib.fluhip_ctx_set_progress_lag(self.h, int(lag)))

    # ---- algorithm::STFT ----------------------------------------------------------------
    def stft(self, audio, win, fft, hop, window_type=0, want_spec=True, want_mag=True, stride=1):
        audio = np.ascontiguousarray(audio)
        n = (audio.shape[0] + stride - 1) // stride
        T = (n + hop) // hop
        F = fft // 2 + 1
        spec = np.empty((T, F, 2)) if want_spec else None
        mag = np.empty((T, F)) if want_mag else None
        Tout = _i64(0)
        if audio.dtype == np.float32:
            rc = self.lib.fluhip_stft_f32(self.h, _f(audio), n, stride, win, fft, hop, window_type,
                                          _d(spec), _d(mag), ctypes.byref(Tout))
        else:
            audio = audio.astype(np.float64, copy=False)
            rc = self.lib.fluhip_stft_f64(self.h, _d(audio), n, stride, win, fft, hop, window_type,
                                          _d(spec), _d(mag), ctypes.byref(Tout))
        self._check(rc)
        assert Tout.value == T
        cs = spec[..., 0] + 1j * spec[..., 1] if want_spec else None
        return cs, mag

    def resynth_f64(self, spec, win, fft, hop, n, trim, W=None, H=None, out=None):
        """fluhip_debug_resynth_f64: the clients' inverse transform on doubles.  spec [T,F] complex (or [T,F,2] doubles);
        W [K,F] and H [T,K] (both or neither) for the ratio-masked components.  Returns [n] without factors, [K,n] with them;
        `out` (a C-contiguous float64 array of that shape) is filled in place when given."""
        spec = np.asarray(spec)
        if np.iscomplexobj(spec):
            spec = np.ascontiguousarray(spec, dtype=np.complex128).view(np.float64).reshape(spec.shape + (2,))
        spec = np.ascontiguousarray(spec, dtype=np.float64)
        T = spec.shape[0]
        assert spec.shape == (T, fft // 2 + 1, 2)
        Wc = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
        Hc = None if H is None else np.ascontiguousarray(H, dtype=np.float64)
        K = 0 if Wc is None else Wc.shape[0]
        assert Wc is None or Wc.shape == (K, fft // 2 + 1)
        assert Hc is None or Wc is None or Hc.shape == (T, K)
        shape = (n,) if Wc is None and Hc is None else (max(K, 1), n)
        if out is None:
            out = np.empty(shape)
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == shape
        self._check(self.lib.fluhip_debug_resynth_f64(self.h, _d(spec), T, win, fft, hop, n, trim, _d(Wc), _d(Hc), K, _d(out)))
        return out

    def debug_stft_frames(self, padded, n, guard, win, fft, hop, frame0, T, want_spec=True, want_mag=True):
        """fluhip_debug_stft_frames_f32 / _f64: T frames of every row of `padded` [B, guard + n + guard] (float32 or float64;
        the n samples of a buffer between guards of the caller's choosing), frame t at samples [frame0 + t hop, + win) of its
        buffer, zero outside [0, n).  Returns (spec complex [B, T, F] or None, mag [B, T, F] or None)."""
        padded = np.ascontiguousarray(padded)
        assert padded.ndim == 2 and padded.shape[1] == n + 2 * guard and padded.dtype in (np.float32, np.float64)
        B, F = padded.shape[0], fft // 2 + 1
        spec = np.empty((B, T, F, 2)) if want_spec else None
        mag = np.empty((B, T, F)) if want_mag else None
        if padded.dtype == np.float32:
            rc = self.lib.fluhip_debug_stft_frames_f32(self.h, _f(padded), B, n, guard, win, fft, hop, frame0, T, _d(spec), _d(mag))
        else:
            rc = self.lib.fluhip_debug_stft_frames_f64(self.h, _d(padded), B, n, guard, win, fft, hop, frame0, T, _d(spec), _d(mag))
        self._check(rc)
        return (spec[..., 0] + 1j * spec[..., 1] if want_spec else None), mag

    # ---- algorithm::NMF -----------------------------------------------------------------
    def nmf_process(self, X, K, iters, updateW=True, updateH=True, seed=42, W0=None, H0=None,
                    progress=None, want_v=True):
        X = np.asarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.strides[1] == 8
        T, F = X.shape
        ldx = X.strides[0] // 8
        W0c = None if W0 is None else np.ascontiguousarray(W0, dtype=np.float64)
        H0c = None if H0 is None else np.ascontiguousarray(H0, dtype=np.float64)
        W1, H1 = np.empty((K, F)), np.empty((T, K))
        V1 = np.empty((T, F)) if want_v else None
        cb = _cb(progress)
        rc = self.lib.fluhip_nmf_process_f64(self.h, X.ctypes.data_as(_dp), T, F, ldx, K, iters,
                                             int(updateW), int(updateH), seed, _d(W0c), _d(H0c),
                                             _d(W1), _d(H1), _d(V1), cb, None)
        self._check(rc, allow=(OK, CANCELLED))
        return W1, H1, V1, rc

    def nmf_process_views(self, X, K, iters, updateW=True, updateH=True, seed=42, W0=None, H0=None, W1=None, H1=None,
                          V1=None, progress=None):
        """NMF::process on numpy arrays used IN PLACE with their own strides (transposed views, sub-blocks)"""
        ref = lambda a: ctypes.byref(MatrixView.of(a)) if a is not None else None  # noqa: E731
        cb = _cb(progress)
        rc = self.lib.fluhip_nmf_process_views_f64(self.h, ref(X), K, iters, int(updateW), int(updateH), seed, ref(W0),
                                                   ref(H0), ref(W1), ref(H1), ref(V1), cb, None)
        return self._check(rc, allow=(OK, CANCELLED))

    def nmf_process_frames(self, X, W0, iters, seed=42, want_v=True):
        """NMF::processFrame (alg/NMF.hpp:45-89) on every row of X [T,F] with the dictionary W0 [K,F]."""
        X = np.asarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.strides[1] == 8
        T, F = X.shape
        W0c = np.ascontiguousarray(W0, dtype=np.float64)
        K = W0c.shape[0]
        assert W0c.shape == (K, F)
        H = np.empty((T, K))
        V = np.empty((T, F)) if want_v else None
        self._check(self.lib.fluhip_nmf_process_frames_f64(self.h, X.ctypes.data_as(_dp), T, F, X.strides[0] // 8,
                                                           _d(W0c), K, iters, seed, _d(H), _d(V)))
        return H, V

    def nndsvd(self, X, w_rows, min_rank=0, max_rank=200, amount=0.8, method=0, seed=-1):
        """NNDSVD::process (alg/NNDSVD.hpp:30-132): W [w_rows,F], H [T,w_rows], rank."""
        X = np.asarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.strides[1] == 8
        T, F = X.shape
        W, H = np.empty((w_rows, F)), np.empty((T, w_rows))
        k = ctypes.c_int64(0)
        self._check(self.lib.fluhip_nndsvd_f64(self.h, X.ctypes.data_as(_dp), T, F, X.strides[0] // 8, w_rows, min_rank,
                                               max_rank, amount, method, seed, _d(W), _d(H), ctypes.byref(k)))
        return W, H, int(k.value)

    def jacobi_svd(self, X):
        """the SVD behind nndsvd / bufnmfseed, whole: s [r], U [r,F] (row j = u_j), VT [r,T] of X^T for X [T,F], and the
        number of Jacobi sweeps; r = min(F, T)"""
        X = np.asarray(X, dtype=np.float64)
        assert X.ndim == 2 and X.strides[1] == 8
        T, F = X.shape
        r = min(T, F)
        s, U, VT = np.empty(r), np.empty((r, F)), np.empty((r, T))
        sweeps = ctypes.c_int64(0)
        self._check(self.lib.fluhip_debug_jacobi_svd_f64(self.h, X.ctypes.data_as(_dp), T, F, X.strides[0] // 8, _d(s), _d(U),
                                                         _d(VT), ctypes.byref(sweeps)))
        return s, U, VT, int(sweeps.value)

    def bufnmfseed(self, audio, win, fft, hop, min_rank=1, max_rank=200, coverage=0.5, method=0, seed=-1, stride=1):
        """BufNMFSeed (nrt/NMFSeedClient.hpp): bases [max_rank,F] f32, activations [max_rank,T] f32, rank."""
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        n = (audio.shape[0] + stride - 1) // stride
        T, F = (n + hop) // hop, fft // 2 + 1
        bases = np.empty((max_rank, F), dtype=np.float32)
        acts = np.empty((max_rank, T), dtype=np.float32)
        k = ctypes.c_int64(0)
        self._check(self.lib.fluhip_bufnmfseed_f32(self.h, _f(audio), n, stride, win, fft, hop, min_rank, max_rank,
                                                   coverage, method, seed, _f(bases), _f(acts), ctypes.byref(k)))
        return bases, acts, int(k.value)

    # ---- one BufNMF channel -------------------------------------------------------------
    def bufnmf_channel(self, audio, win, fft, hop, K, iters, seed, updateW=True, updateH=True,
                       bases_seed=None, acts_seed=None, progress=None, stride=1, resynth=False):
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        n = (audio.shape[0] + stride - 1) // stride
        T, F = (n + hop) // hop, fft // 2 + 1
        bases = np.empty((K, F), dtype=np.float32)
        acts = np.empty((K, T), dtype=np.float32)
        bs = None if bases_seed is None else np.ascontiguousarray(bases_seed, dtype=np.float32)
        as_ = None if acts_seed is None else np.ascontiguousarray(acts_seed, dtype=np.float32)
        cb = _cb(progress)
        res = np.empty((K, n), dtype=np.float32) if resynth else None
        rc = self.lib.fluhip_bufnmf_channel_f32(self.h, _f(audio), n, stride, win, fft, hop, K, iters,
                                                int(updateW), int(updateH), seed, _f(bs), _f(as_),
                                                _f(bases), _f(acts), _f(res), cb, None)
        self._check(rc, allow=(OK, CANCELLED))
        if resynth:
            return bases, acts, res, rc
        return bases, acts, rc

    # ---- feature pipeline -----------------------------------------------------------------
    @staticmethod
    def feature_frames(n, win, hop, padding_mode=1):
        pad = (0, win // 2, win - hop)[padding_mode]
        padded = n + win + 2 * pad
        if padding_mode == 2:
            padded = -(-padded // hop) * hop
        return 1 + (padded - win) // hop - win // hop

    def bufmfcc(self, audio, win, fft, hop, n_bands=40, n_coefs=13, start_coeff=0, lo=20.0, hi=20000.0,
                sr=44100.0, padding_mode=1):
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        T = self.feature_frames(n, win, hop, padding_mode)
        out = np.empty((count, n_coefs, T), dtype=np.float32)
        Tr = _i64(0)
        if padding_mode == 1:
            rc = self.lib.fluhip_bufmfcc_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, n_coefs,
                                             start_coeff, lo, hi, sr, _f(out), ctypes.byref(Tr))
        else:
            rc = self.lib.fluhip_bufmfcc_padded_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, n_coefs,
                                                    start_coeff, lo, hi, sr, padding_mode, _f(out), ctypes.byref(Tr))
        self._check(rc)
        assert Tr.value == T
        return out

    def bufmelbands(self, audio, win, fft, hop, n_bands=40, lo=20.0, hi=20000.0, sr=44100.0, normalize=True,
                    scale_db=False, padding_mode=1):
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        T = self.feature_frames(n, win, hop, padding_mode)
        out = np.empty((count, n_bands, T), dtype=np.float32)
        Tr = _i64(0)
        if padding_mode == 1:
            rc = self.lib.fluhip_bufmelbands_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, lo, hi, sr,
                                                 int(normalize), int(scale_db), _f(out), ctypes.byref(Tr))
        else:
            rc = self.lib.fluhip_bufmelbands_padded_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, lo, hi, sr,
                                                        int(normalize), int(scale_db), padding_mode, _f(out),
                                                        ctypes.byref(Tr))
        self._check(rc)
        assert Tr.value == T
        return out

    def features_plan(self, mfcc, win, fft, n_bands=40, n_coefs=13, start_coeff=0, lo=20.0, hi=20000.0, sr=44100.0):
        """(form, wavefronts per workgroup, frames per wavefront, dynamic LDS bytes, rows staged) of bufmfcc (mfcc true) /
        bufmelbands at a shape: form 0 is the fused STFT -> mel -> DCT launch (the other four are 0), form 1 the two-kernel
        form; rows staged 1: the magnitude rows of a wavefront's frames sit in the LDS, 0: they are read from memory"""
        out = (_i64 * 5)()
        self._check(self.lib.fluhip_debug_features_plan(self.h, int(bool(mfcc)), win, fft, n_bands, n_coefs, start_coeff, lo,
                                                        hi, sr, out))
        return tuple(int(v) for v in out)

    # ---- BufSTFT ----------------------------------------------------------------------------
    def nmfmatch(self, audio, bases, win, fft, hop, seed=42, padding_mode=1):
        """NMFMatch over a buffer (fluhip_nmfmatch_f32): audio [channels, n] or [n] floats, bases [K, F] -> [channels, K, T]"""
        a = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        b = np.ascontiguousarray(bases, dtype=np.float32)
        count, n = a.shape
        K = b.shape[0]
        T = _i64(0)
        f = self.lib.fluhip_nmfmatch_f32
        f.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _fp, _i64, _i64, ctypes.c_int, _fp, _ip]
        self._check(f(self.h, _f(a), count, n, win, fft, hop, _f(b), K, seed, padding_mode, None, ctypes.byref(T)))
        out = np.empty((count, K, T.value), dtype=np.float32)
        self._check(f(self.h, _f(a), count, n, win, fft, hop, _f(b), K, seed, padding_mode, _f(out), ctypes.byref(T)))
        return out

    def nmffilter(self, audio, bases, win, fft, hop, iters=10, seed=42):
        """NMFFilter over a buffer (fluhip_nmffilter_f32): -> [channels, K, n] floats"""
        a = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        b = np.ascontiguousarray(bases, dtype=np.float32)
        count, n = a.shape
        K = b.shape[0]
        out = np.empty((count, K, n), dtype=np.float32)
        f = self.lib.fluhip_nmffilter_f32
        f.argtypes = [_vp, _fp, _i64, _i64, _i64, _i64, _i64, _fp, _i64, _i64, _i64, _fp]
        self._check(f(self.h, _f(a), count, n, win, fft, hop, _f(b), K, iters, seed, _f(out)))
        return out

    def bufstft_forward(self, audio, win, fft, hop, padding_mode=1):
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        n = audio.shape[0]
        pad = [0, win >> 1, win - hop][padding_mode]
        padded = n + 2 * pad
        if padding_mode == 2:
            padded = -(-padded // hop) * hop
        T, F = 1 + (padded - win) // hop, fft // 2 + 1
        mag = np.empty((F, T), dtype=np.float32)
        ph = np.empty((F, T), dtype=np.float32)
        Tr = _i64(0)
        self._check(self.lib.fluhip_bufstft_forward_f32(self.h, _f(audio), n, 1, win, fft, hop, padding_mode,
                                                        _f(mag), _f(ph), ctypes.byref(Tr)))
        assert Tr.value == T
        return mag, ph

    def bufstft_inverse(self, mag, phase, win, fft, hop, padding_mode=1):
        mag = np.ascontiguousarray(mag, dtype=np.float32)
        phase = np.ascontiguousarray(phase, dtype=np.float32)
        F, T = mag.shape
        nout = _i64(0)
        self._check(self.lib.fluhip_bufstft_inverse_f32(self.h, _f(mag), _f(phase), T, win, fft, hop, padding_mode,
                                                        None, ctypes.byref(nout)))
        out = np.empty(nout.value, dtype=np.float32)
        self._check(self.lib.fluhip_bufstft_inverse_f32(self.h, _f(mag), _f(phase), T, win, fft, hop, padding_mode,
                                                        _f(out), ctypes.byref(nout)))
        return out

    # ---- BufNMFCross (alg/NMFCross.hpp, alg/GriffinLim.hpp, nrt/NMFCrossClient.hpp) ------------------------
    def nmfcross_process(self, X, W0, time_sparsity=7, polyphony=11, continuity=7, iters=50, seed=42, progress=None):
        """NMFCross::process: X [T,F] target magnitudes, W0 [K,F] source magnitudes (not modified) -> (H1 [T,K], status);
        status is CANCELLED when the progress callback refused an iteration"""
        X = np.asarray(X, dtype=np.float64)
        W0 = np.asarray(W0, dtype=np.float64)
        assert X.ndim == 2 and X.strides[1] == 8 and W0.ndim == 2 and W0.strides[1] == 8
        T, F = X.shape
        K = W0.shape[0]
        assert W0.shape[1] == F
        H1 = np.empty((T, K))
        rc = self.lib.fluhip_nmfcross_process_f64(self.h, X.ctypes.data_as(_dp), T, F, X.strides[0] // 8,
                                                  W0.ctypes.data_as(_dp), K, W0.strides[0] // 8, time_sparsity, polyphony,
                                                  continuity, iters, seed, _d(H1), _cb(progress), None)
        self._check(rc, allow=(OK, CANCELLED))
        return H1, rc

    def cross_plan(self, M, N, Kd):
        """(big_tiles, splits, split_depth) of an NMFCross GEMM of an M x N output over Kd on this device"""
        out = (_i64 * 3)()
        self._check(self.lib.fluhip_debug_cross_plan(self.h, M, N, Kd, out))
        return bool(out[0]), int(out[1]), int(out[2])

    def cross_stencil(self, H, which, size, energy=None):
        """fluhip_debug_cross_stencil_f64: one constraint stencil of the H loop on H [T,K] doubles -- which 0 continuity
        (size c), 1 temporal sparsity on its zeroing iteration (size r), 2 polyphony on its zeroing iteration (size p,
        energy [K]); returns the new [T,K]"""
        H = np.ascontiguousarray(H, dtype=np.float64)
        T, K = H.shape
        e = None if energy is None else np.ascontiguousarray(energy, dtype=np.float64)
        assert e is None or e.shape == (K,)
        out = np.empty((T, K))
        self._check(self.lib.fluhip_debug_cross_stencil_f64(self.h, _d(H), T, K, which, size, None if e is None else _d(e),
                                                            _d(out)))
        return out

    def griffinlim(self, spec, n_samples, win, fft, hop, iters=50, seed=42):
        """GriffinLim::process on a complex [T,F] spectrum; returns the new spectrum"""
        out = np.ascontiguousarray(spec, dtype=np.complex128).copy()
        T, F = out.shape
        self._check(self.lib.fluhip_griffinlim_f64(self.h, out.ctypes.data_as(_dp), T, F, n_samples, iters, win, fft, hop,
                                                   seed))
        return out

    def bufnmfcross(self, source, target, win=1024, fft=-1, hop=-1, time_sparsity=7, polyphony=11, continuity=7, iters=50,
                    seed=-1, progress=None, source_stride=1, target_stride=1):
        """NMFCrossClient::process on channel 0 of two float buffers: returns (output [n_target] float32, status);
        fft / hop < 0 take the FFTParams defaults (next power of two, win / 2)"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        source = np.ascontiguousarray(source, dtype=np.float32)
        target = np.ascontiguousarray(target, dtype=np.float32)
        n_src, n_tgt = len(source) // source_stride, len(target) // target_stride
        out = np.empty(max(n_tgt, 1), dtype=np.float32)
        rc = self.lib.fluhip_bufnmfcross_f32(self.h, _f(source), n_src, source_stride, _f(target), n_tgt, target_stride,
                                             w.value, f.value, h.value, time_sparsity, polyphony, continuity, iters, seed,
                                             _f(out), _cb(progress), None)
        self._check(rc, allow=(OK, CANCELLED))
        return out[:n_tgt], rc

    # ---- BufNoveltySlice / BufNoveltyFeature (util/Novelty.hpp, NoveltyFeature.hpp, NoveltySegmentation.hpp) ------------
    @staticmethod
    def _novelty_feat(feat):
        feat = np.asarray(feat, dtype=np.float64)
        if feat.ndim == 2:
            feat = feat[None]
        assert feat.ndim == 3 and feat.strides[2] == 8
        count, T, D = feat.shape
        ld = feat.strides[1] // 8
        assert count == 1 or feat.strides[0] == T * ld * 8, "buffers must lie T rows apart"
        return feat, count, T, D, ld

    def novelty_curve(self, feat, kernel_size=3, filter_size=1):
        """NoveltyFeature::processFrame over all frames: feat [count,T,D] (or [T,D]; rows may be strided) -> curve [count,T]"""
        feat, count, T, D, ld = self._novelty_feat(feat)
        curve = np.empty((count, T))
        self._check(self.lib.fluhip_novelty_curve_f64(self.h, feat.ctypes.data_as(_dp), count, T, D, ld, kernel_size,
                                                      filter_size, _d(curve)))
        return curve

    def novelty_slices(self, feat, kernel_size=3, filter_size=1, threshold=0.5, min_slice=2):
        """NoveltySegmentation::processFrame over all frames -> (det [count,T] uint8, counts [count], curve [count,T])"""
        feat, count, T, D, ld = self._novelty_feat(feat)
        curve = np.empty((count, T))
        det = np.empty((count, T), dtype=np.uint8)
        counts = np.empty(count, dtype=np.int64)
        self._check(self.lib.fluhip_novelty_slices_f64(self.h, feat.ctypes.data_as(_dp), count, T, D, ld, kernel_size,
                                                       filter_size, threshold, min_slice,
                                                       det.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                                       counts.ctypes.data_as(_ip), _d(curve)))
        return det, counts, curve

    def novelty_plan(self, T, D, kernel_size):
        """(form, rows held, curve values written) per workgroup: form 0 MFMA on chip, 1 FMAs on chip, 2 tiled"""
        out = (_i64 * 3)()
        self._check(self.lib.fluhip_debug_novelty_plan(self.h, T, D, kernel_size, out))
        return int(out[0]), int(out[1]), int(out[2])

    def bufnoveltyslice(self, audio, algorithm=0, kernel_size=3, threshold=0.5, filter_size=1, min_slice=2, win=1024,
                        fft=-1, hop=-1, sr=44100.0, start_frame=0, capacity=None):
        """NRTNoveltySliceClient on audio [count,channels,n] (or [channels,n] / [n]): a list of int64 index arrays, one per
        buffer ([-1] when nothing was detected).  capacity: values kept per buffer (default: every possible frame)"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.asarray(audio, dtype=np.float32)
        while audio.ndim < 3:
            audio = audio[None]
        audio = np.ascontiguousarray(audio)
        count, channels, n = audio.shape
        if capacity is None:
            capacity = n // h.value + 2
        idx = np.full((count, max(capacity, 1)), -2, dtype=np.int64)
        counts = np.zeros(count, dtype=np.int64)
        self._check(self.lib.fluhip_bufnoveltyslice_f32(self.h, _f(audio), count, channels, n, start_frame, algorithm,
                                                        kernel_size, threshold, filter_size, min_slice, w.value, f.value,
                                                        h.value, sr, idx.ctypes.data_as(_ip), capacity,
                                                        counts.ctypes.data_as(_ip)))
        self.last_slice_counts = counts
        return [idx[b, :min(int(counts[b]), capacity)].copy() for b in range(count)]

    def bufnoveltyfeature(self, audio, algorithm=0, kernel_size=3, filter_size=1, win=1024, fft=-1, hop=-1, sr=44100.0,
                          padding_mode=1):
        """NRTNoveltyFeatureClient on mono buffers [count,n] (or [n]) -> float32 [count,frames]"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        self._check(self.lib.fluhip_bufnoveltyfeature_f32(self.h, _f(audio), count, n, algorithm, kernel_size, filter_size,
                                                          w.value, f.value, h.value, sr, padding_mode, None,
                                                          ctypes.byref(Tr)))
        out = np.empty((count, Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufnoveltyfeature_f32(self.h, _f(audio), count, n, algorithm, kernel_size, filter_size,
                                                          w.value, f.value, h.value, sr, padding_mode, _f(out),
                                                          ctypes.byref(Tr)))
        return out

    # ---- BufOnsetSlice / BufOnsetFeature (util/OnsetDetectionFuncs.hpp, OnsetDetectionFunctions.hpp, OnsetSegmentation.hpp) --
    @staticmethod
    def _onset_signal(signal):
        signal = np.asarray(signal, dtype=np.float64)
        if signal.ndim == 1:
            signal = signal[None]
        assert signal.ndim == 2 and signal.strides[1] == 8
        count, n = signal.shape
        ld = signal.strides[0] // 8 if count > 1 else n
        return signal, count, n, ld

    def onset_curve(self, signal, T, win=1024, fft=1024, hop=512, function=0, filter_size=5, frame_delta=0):
        """OnsetDetectionFunctions::processFrame over T frames of padded signals [count,n] (or [n]): frame i reads
        [i hop, i hop + win + d) -> (raw [count,T], filtered [count,T])"""
        signal, count, n, ld = self._onset_signal(signal)
        raw = np.empty((count, T))
        filtered = np.empty((count, T))
        self._check(self.lib.fluhip_onset_curve_f64(self.h, signal.ctypes.data_as(_dp), count, n, ld, T, win, fft, hop,
                                                    function, filter_size, frame_delta, _d(raw), _d(filtered)))
        return raw, filtered

    def onset_slices(self, signal, T, win=1024, fft=1024, hop=512, function=0, filter_size=5, frame_delta=0, threshold=0.5,
                     min_slice=2):
        """OnsetSegmentation::processFrame over T frames -> (det [count,T] uint8, counts [count], filtered [count,T])"""
        signal, count, n, ld = self._onset_signal(signal)
        filtered = np.empty((count, T))
        det = np.empty((count, T), dtype=np.uint8)
        counts = np.empty(count, dtype=np.int64)
        self._check(self.lib.fluhip_onset_slices_f64(self.h, signal.ctypes.data_as(_dp), count, n, ld, T, win, fft, hop,
                                                     function, filter_size, frame_delta, threshold, min_slice,
                                                     det.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                                     counts.ctypes.data_as(_ip), _d(filtered)))
        return det, counts, filtered

    def onset_plan(self, fft, win, function, frame_delta=0):
        """(form, frames of history recomputed, transforms per frame, frames a workgroup writes); form 0: one fused launch, the
        spectra stay in the LDS (fft 1024 / 2048 / 4096, even window); form 1: two passes through a workspace (run 0)"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_onset_plan(self.h, fft, win, function, frame_delta, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def bufonsetslice(self, audio, function=0, threshold=0.5, min_slice=2, filter_size=5, frame_delta=0, win=1024, fft=-1,
                      hop=-1, start_frame=0, capacity=None):
        """NRTOnsetSliceClient on audio [count,channels,n] (or [channels,n] / [n]): a list of int64 index arrays, one per
        buffer ([-1] when nothing was detected).  capacity: values kept per buffer (default: every possible frame)"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.asarray(audio, dtype=np.float32)
        while audio.ndim < 3:
            audio = audio[None]
        audio = np.ascontiguousarray(audio)
        count, channels, n = audio.shape
        if capacity is None:
            capacity = n // h.value + 2
        idx = np.full((count, max(capacity, 1)), -2, dtype=np.int64)
        counts = np.zeros(count, dtype=np.int64)
        self._check(self.lib.fluhip_bufonsetslice_f32(self.h, _f(audio), count, channels, n, start_frame, function, threshold,
                                                      min_slice, filter_size, frame_delta, w.value, f.value, h.value,
                                                      idx.ctypes.data_as(_ip), capacity, counts.ctypes.data_as(_ip)))
        self.last_slice_counts = counts
        return [idx[b, :min(int(counts[b]), capacity)].copy() for b in range(count)]

    def bufonsetfeature(self, audio, function=0, filter_size=5, frame_delta=0, win=1024, fft=-1, hop=-1, padding_mode=1):
        """NRTOnsetFeatureClient on mono buffers [count,n] (or [n]) -> float32 [count,frames]"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        args = (function, filter_size, frame_delta, w.value, f.value, h.value, padding_mode)
        self._check(self.lib.fluhip_bufonsetfeature_f32(self.h, _f(audio), count, n, *args, None, ctypes.byref(Tr)))
        out = np.empty((count, Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufonsetfeature_f32(self.h, _f(audio), count, n, *args, _f(out), ctypes.byref(Tr)))
        return out

    # ---- BufHPSS (algorithms/public/HPSS.hpp, clients/rt/HPSSClient.hpp) ----------------------------------------------
    def hpss_planes(self, mag, h_size=17, v_size=31, mode=0, h_thresh=(0.0, 1.0, 1.0, 1.0), p_thresh=(0.0, 1.0, 1.0, 1.0)):
        """HPSS::processFrame over magnitude planes [count,T,F] (or [T,F]) -> (hmed, vmed, masks [3]) each [count,T,F]"""
        mag = np.asarray(mag, dtype=np.float64)
        if mag.ndim == 2:
            mag = mag[None]
        mag = np.ascontiguousarray(mag)
        count, T, F = mag.shape
        hmed, vmed = np.empty((count, T, F)), np.empty((count, T, F))
        masks = np.empty((3, count, T, F))
        mp = (_dp * 3)(*[_d(masks[i]) for i in range(3)])
        ht, pt = (ctypes.c_double * 4)(*h_thresh), (ctypes.c_double * 4)(*p_thresh)
        self._check(self.lib.fluhip_hpss_planes_f64(self.h, _d(mag), count, T, F, F, h_size, v_size, mode, ht, pt, _d(hmed),
                                                    _d(vmed), mp))
        return hmed, vmed, masks

    def bufhpss(self, audio, win=1024, fft=-1, hop=-1, h_size=17, v_size=31, mode=0, h_thresh=(0.0, 1.0, 1.0, 1.0),
                p_thresh=(0.0, 1.0, 1.0, 1.0)):
        """NRTHPSSClient on mono buffers [count,n] (or [n]) -> float32 [count,3,n]: harmonic, percussive, residual"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        out = np.empty((count, 3, n), dtype=np.float32)
        ht, pt = (ctypes.c_double * 4)(*h_thresh), (ctypes.c_double * 4)(*p_thresh)
        self._check(self.lib.fluhip_bufhpss_f32(self.h, _f(audio), count, n, w.value, f.value, h.value, h_size, v_size, mode,
                                                ht, pt, _f(out)))
        return out

    def hpss_plan(self, h_size, v_size):
        """(form of the H median, form of the V median, LDS bytes of a workgroup, bins of a workgroup); form 0: the window is
        ranked from the LDS (sizes up to 63), form 1: from the plane in memory"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_hpss_plan(self.h, h_size, v_size, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- BufPitch (algorithms/public/YINFFT.hpp, HPS.hpp, CepstrumF0.hpp, clients/rt/PitchClient.hpp) -------------------
    def _pitch_mag(self, mag):
        mag = np.asarray(mag, dtype=np.float64)
        if mag.ndim == 2:
            mag = mag[None]
        return np.ascontiguousarray(mag)

    def pitch_frames(self, mag, algorithm=2, min_freq=20.0, max_freq=10000.0, sample_rate=44100.0):
        """processFrame of Cepstrum (0), HPS (1) or YinFFT (2) over magnitude planes [count,T,F] (or [T,F]) ->
        [count,T,2] doubles (pitch in Hz, confidence)"""
        mag = self._pitch_mag(mag)
        count, T, F = mag.shape
        out = np.empty((count, T, 2))
        self._check(self.lib.fluhip_pitch_frames_f64(self.h, _d(mag), count, T, F, F, algorithm, min_freq, max_freq,
                                                     sample_rate, _d(out)))
        return out

    def pitch_curve(self, mag, algorithm=2, min_freq=20.0, max_freq=10000.0, sample_rate=44100.0):
        """the curve the algorithm searches, [count,T,F]: normalised yin, harmonic product or cepstrum"""
        mag = self._pitch_mag(mag)
        count, T, F = mag.shape
        curve = np.empty((count, T, F))
        self._check(self.lib.fluhip_debug_pitch_curve_f64(self.h, _d(mag), count, T, F, F, algorithm, min_freq, max_freq,
                                                          sample_rate, _d(curve)))
        return curve

    def bufpitch(self, audio, algorithm=2, min_freq=20.0, max_freq=10000.0, unit=0, select=3, win=1024, fft=-1, hop=-1,
                 padding_mode=1, sample_rate=44100.0):
        """NRTPitchClient on mono buffers [count,n] (or [n]) -> float32 [count,selected,frames]"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        args = (w.value, f.value, h.value, padding_mode, algorithm, min_freq, max_freq, unit, select, sample_rate)
        self._check(self.lib.fluhip_bufpitch_f32(self.h, _f(audio), count, n, *args, None, ctypes.byref(Tr)))
        out = np.empty((count, bin(select & 3).count("1"), Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufpitch_f32(self.h, _f(audio), count, n, *args, _f(out), ctypes.byref(Tr)))
        return out

    def pitch_plan(self, fft, win, algorithm):
        """(form, frames a workgroup of the on-chip form writes, transforms per frame, DCT rows of the cepstrum's GEMM at the
        default bounds); form 0: transform and pitch in one launch, magnitudes in the LDS (fft 1024 / 2048 / 4096, even
        window; run 32); form 1: two passes through a magnitude workspace (run 0)"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_pitch_plan(self.h, fft, win, algorithm, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- BufSpectralShape, BufChroma (algorithms/public/SpectralShape.hpp, ChromaFilterBank.hpp and their clients) --------
    def spectralshape_frames(self, mag, min_freq=0.0, max_freq=-1.0, rolloff_percent=95.0, unit=0, power=0, sample_rate=44100.0):
        """SpectralShape::processFrame over magnitude planes [count,T,F] (or [T,F]) -> [count,T,7] doubles (centroid, spread,
        skewness, kurtosis, rolloff, flatness, crest)"""
        mag = self._pitch_mag(mag)
        count, T, F = mag.shape
        out = np.empty((count, T, 7))
        self._check(self.lib.fluhip_spectralshape_frames_f64(self.h, _d(mag), count, T, F, F, min_freq, max_freq, rolloff_percent,
                                                             unit, power, sample_rate, _d(out)))
        return out

    def bufspectralshape(self, audio, select=127, min_freq=0.0, max_freq=-1.0, rolloff_percent=95.0, unit=0, power=0, win=1024,
                         fft=-1, hop=-1, padding_mode=1, sample_rate=44100.0):
        """NRTSpectralShapeClient on mono buffers [count,n] (or [n]) -> float32 [count,selected,frames]"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        args = (w.value, f.value, h.value, padding_mode, select, min_freq, max_freq, rolloff_percent, unit, power, sample_rate)
        self._check(self.lib.fluhip_bufspectralshape_f32(self.h, _f(audio), count, n, *args, None, ctypes.byref(Tr)))
        out = np.empty((count, bin(select & 127).count("1"), Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufspectralshape_f32(self.h, _f(audio), count, n, *args, _f(out), ctypes.byref(Tr)))
        return out

    def chroma_filters(self, num_chroma, F, ref=440.0, sample_rate=44100.0):
        """the table of ChromaFilterBank::init, [num_chroma,F] doubles"""
        out = np.empty((num_chroma, F))
        self._check(self.lib.fluhip_debug_chroma_filters_f64(self.h, num_chroma, F, ref, sample_rate, _d(out)))
        return out

    def chroma_frames(self, mag, num_chroma=12, ref=440.0, normalize=0, min_freq=0.0, max_freq=-1.0, sample_rate=44100.0):
        """ChromaFilterBank::processFrame over magnitude planes [count,T,F] (or [T,F]) -> [count,T,num_chroma] doubles"""
        mag = self._pitch_mag(mag)
        count, T, F = mag.shape
        out = np.empty((count, T, max(0, num_chroma)))
        self._check(self.lib.fluhip_chroma_frames_f64(self.h, _d(mag), count, T, F, F, num_chroma, ref, normalize, min_freq,
                                                      max_freq, sample_rate, _d(out)))
        return out

    def bufchroma(self, audio, num_chroma=12, ref=440.0, normalize=0, min_freq=0.0, max_freq=-1.0, win=1024, fft=-1, hop=-1,
                  padding_mode=1, sample_rate=44100.0):
        """NRTChromaClient on mono buffers [count,n] (or [n]) -> float32 [count,num_chroma,frames]"""
        w, h, f = _i64(), _i64(), _i64()
        self._check(self.lib.fluhip_fft_params(win, hop, fft, ctypes.byref(w), ctypes.byref(h), ctypes.byref(f), None))
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        args = (w.value, f.value, h.value, padding_mode, num_chroma, ref, normalize, min_freq, max_freq, sample_rate)
        self._check(self.lib.fluhip_bufchroma_f32(self.h, _f(audio), count, n, *args, None, ctypes.byref(Tr)))
        out = np.empty((count, num_chroma, Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufchroma_f32(self.h, _f(audio), count, n, *args, _f(out), ctypes.byref(Tr)))
        return out

    def spectral_plan(self, fft, win, kind):
        """(form, frames a workgroup of the on-chip form writes, transforms per frame, 1 when a GEMM follows) of SpectralShape
        (kind 0) or Chroma (kind 1); form 0: one launch, magnitudes in the LDS (fft 1024 / 2048 / 4096, even window; run 32);
        form 1: two passes through a magnitude workspace (run 0)"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_spectral_plan(self.h, fft, win, kind, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- BufLoudness (algorithms/public/Loudness.hpp, util/KWeightingFilter.hpp, util/TruePeak.hpp and the client) -----------
    def loudness_frames(self, x, win=1024, hop=512, k_weighting=1, true_peak=1, sample_rate=44100.0):
        """Loudness::processFrame over the frames x[j hop : j hop + win] of signals [count,n] (or [n]), the filter and the
        interpolator carried from frame 0 -> [count,T,2] doubles (loudness, peak), T = 1 + (n - win) // hop"""
        x = np.ascontiguousarray(np.atleast_2d(x), dtype=np.float64)
        count, n = x.shape
        T = 1 + (n - win) // hop if (n >= win and hop >= 1 and win >= 1) else 0
        out = np.empty((count, max(T, 0), 2))
        self._check(self.lib.fluhip_loudness_frames_f64(self.h, _d(x), count, n, win, hop, k_weighting, true_peak, sample_rate,
                                                        _d(out)))
        return out

    def bufloudness(self, audio, select=3, k_weighting=1, true_peak=1, win=1024, hop=512, padding_mode=1, sample_rate=44100.0):
        """NRTLoudnessClient on mono buffers [count,n] (or [n]) -> float32 [count,selected,frames]"""
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        Tr = _i64(0)
        args = (win, hop, padding_mode, select, k_weighting, true_peak, sample_rate)
        self._check(self.lib.fluhip_bufloudness_f32(self.h, _f(audio), count, n, *args, None, ctypes.byref(Tr)))
        out = np.empty((count, bin(select & 3).count("1"), Tr.value), dtype=np.float32)
        self._check(self.lib.fluhip_bufloudness_f32(self.h, _f(audio), count, n, *args, _f(out), ctypes.byref(Tr)))
        return out

    def loudness_plan(self, win, hop, sample_rate=44100.0):
        """(form, frames a workgroup owns, interpolation factor 4 / 2 / 1, history samples the interpolator reads in front of
        a frame); form 0: lane = frame, the filter states by a double-double scan per buffer"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_loudness_plan(self.h, win, hop, sample_rate, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- BufAmpSlice / BufAmpFeature (algorithms/public/Envelope.hpp, EnvelopeSegmentation.hpp and the two clients) ---------
    def amp_envelope(self, x, fast_up=1, fast_down=1, slow_up=100, slow_down=100, floor=-144.0, hipass=0.0):
        """Envelope::processSample over signals [count,n] (or [n]) of doubles, hipass the cutoff as a fraction of the sample
        rate -> [count,n] doubles"""
        x, count, n, ld = self._onset_signal(x)
        out = np.empty((count, n))
        self._check(self.lib.fluhip_amp_envelope_f64(self.h, x.ctypes.data_as(_dp), count, n, ld, fast_up, fast_down, slow_up,
                                                     slow_down, floor, hipass, _d(out)))
        return out

    def amp_slices(self, x, fast_up=1, fast_down=1, slow_up=100, slow_down=100, on=144.0, off=-144.0, floor=-144.0, min_slice=2,
                   hipass=0.0, want_det=True, want_envelope=True):
        """EnvelopeSegmentation::processSample over signals [count,n] (or [n]) -> (det [count,n] uint8 or None, counts [count],
        envelope [count,n] or None)"""
        x, count, n, ld = self._onset_signal(x)
        det = np.empty((count, n), dtype=np.uint8) if want_det else None
        env = np.empty((count, n)) if want_envelope else None
        counts = np.empty(count, dtype=np.int64)
        self._check(self.lib.fluhip_amp_slices_f64(self.h, x.ctypes.data_as(_dp), count, n, ld, fast_up, fast_down, slow_up,
                                                   slow_down, on, off, floor, min_slice, hipass,
                                                   det.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if want_det else None,
                                                   counts.ctypes.data_as(_ip), _d(env)))
        return det, counts, env

    def bufampslice(self, audio, fast_up=1, fast_down=1, slow_up=100, slow_down=100, on=144.0, off=-144.0, floor=-144.0,
                    min_slice=2, high_pass_freq=85.0, sample_rate=44100.0, start_frame=0, capacity=None):
        """NRTAmpSliceClient on audio [count,channels,n] (or [channels,n] / [n]): a list of int64 index arrays, one per buffer
        ([-1] when nothing was detected).  capacity: values kept per buffer (default: every possible one)"""
        audio = np.asarray(audio, dtype=np.float32)
        while audio.ndim < 3:
            audio = audio[None]
        audio = np.ascontiguousarray(audio)
        count, channels, n = audio.shape
        if capacity is None:
            capacity = n // 2 + 2   # a detection needs the previous value below the threshold: every other sample at most
        idx = np.full((count, max(capacity, 1)), -2, dtype=np.int64)
        counts = np.zeros(count, dtype=np.int64)
        self._check(self.lib.fluhip_bufampslice_f32(self.h, _f(audio), count, channels, n, start_frame, fast_up, fast_down,
                                                    slow_up, slow_down, on, off, floor, min_slice, high_pass_freq, sample_rate,
                                                    idx.ctypes.data_as(_ip), capacity, counts.ctypes.data_as(_ip)))
        self.last_slice_counts = counts
        return [idx[b, :min(int(counts[b]), capacity)].copy() for b in range(count)]

    def bufampfeature(self, audio, fast_up=1, fast_down=1, slow_up=100, slow_down=100, floor=-144.0, high_pass_freq=85.0,
                      sample_rate=44100.0):
        """NRTAmpFeatureClient on audio [count,channels,n] (or [channels,n] / [n]) -> float32 [count,channels,n]"""
        audio = np.asarray(audio, dtype=np.float32)
        while audio.ndim < 3:
            audio = audio[None]
        audio = np.ascontiguousarray(audio)
        count, channels, n = audio.shape
        out = np.empty((count, channels, n), dtype=np.float32)
        self._check(self.lib.fluhip_bufampfeature_f32(self.h, _f(audio), count, channels, n, fast_up, fast_down, slow_up,
                                                      slow_down, floor, high_pass_freq, sample_rate, _f(out)))
        return out

    def amp_plan(self, hipass=85.0 / 44100.0):
        """(form, samples of a front-end chunk, signals per wavefront of the serial follower kernel, 1 if the high-pass scan
        launches run)"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_amp_plan(self.h, hipass, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- BufAmpGate (algorithms/public/EnvelopeGate.hpp and clients/rt/AmpGateClient.hpp) -----------------------------------
    def amp_gate(self, x, ramp_up=10, ramp_down=10, on=-90.0, off=-90.0, min_slice=1, min_silence=1, min_above=1, min_below=1,
                 look_back=0, look_ahead=0, hipass=0.0, max_size=88200, want_smoothed=True):
        """EnvelopeGate::processSample over signals [count,n] (or [n]) of doubles, hipass the cutoff as a fraction of the sample
        rate -> (what it returned per sample [count,n] uint8, the smoothed values [count,n] or None)"""
        x, count, n, ld = self._onset_signal(x)
        out = np.empty((count, n), dtype=np.uint8)
        smoothed = np.empty((count, n)) if want_smoothed else None
        self._check(self.lib.fluhip_amp_gate_f64(self.h, x.ctypes.data_as(_dp), count, n, ld, ramp_up, ramp_down, on, off, min_slice,
                                                 min_silence, min_above, min_below, look_back, look_ahead, hipass, max_size,
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), _d(smoothed)))
        return out, smoothed

    def bufampgate(self, audio, ramp_up=10, ramp_down=10, on=-90.0, off=-90.0, min_slice=1, min_silence=1, min_above=1,
                   min_below=1, look_back=0, look_ahead=0, high_pass_freq=85.0, max_size=88200, sample_rate=44100.0, start_frame=0,
                   capacity=None):
        """NRTAmpGateClient on audio [count,channels,n] (or [channels,n] / [n]): a list of (onsets, offsets) int64 arrays, one
        pair per buffer ([-1], [-1] when the gate never switches; None where it changes on the last sample: the count is -1).
        capacity: values kept per row (default: every possible one)"""
        audio = np.asarray(audio, dtype=np.float32)
        while audio.ndim < 3:
            audio = audio[None]
        audio = np.ascontiguousarray(audio)
        count, channels, n = audio.shape
        if capacity is None:
            capacity = n // 2 + 2   # a rise needs a fall in front of it: every other sample at most
        idx = np.full((count, 2, max(capacity, 1)), -2, dtype=np.int64)
        counts = np.zeros(count, dtype=np.int64)
        self._check(self.lib.fluhip_bufampgate_f32(self.h, _f(audio), count, channels, n, start_frame, ramp_up, ramp_down, on, off,
                                                   min_slice, min_silence, min_above, min_below, look_back, look_ahead, high_pass_freq,
                                                   sample_rate, max_size, idx.ctypes.data_as(_ip), capacity,
                                                   counts.ctypes.data_as(_ip)))
        self.last_slice_counts = counts
        return [None if counts[b] < 0 else (idx[b, 0, :min(int(counts[b]), capacity)].copy(),
                                            idx[b, 1, :min(int(counts[b]), capacity)].copy()) for b in range(count)]

    def ampgate_plan(self):
        """(form, signals per wavefront of the two serial kernels, samples of a row staged at a time, 0 if a lookup reads its
        window from global memory / 1 from the LDS)"""
        out = (_i64 * 4)()
        self._check(self.lib.fluhip_debug_ampgate_plan(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    # ---- profiling ----------------------------------------------------------------------
    def prof_enable(self, on=True):
        self._check(self.lib.fluhip_prof_enable(self.h, int(on)))

    def prof_reset(self):
        self._check(self.lib.fluhip_prof_reset(self.h))

    def prof_read(self, cls):
        n, ms = _i64(0), ctypes.c_double(0)
        self._check(self.lib.fluhip_prof_read(self.h, cls, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value


class Corpus:
    """fluhip_corpus: `count` equal-shape mono buffers resident in HBM."""

    def __init__(self, ctx: Context, count, n, win, fft, hop, K):
        self.ctx = ctx
        self.count, self.n, self.win, self.fft, self.hop, self.K = count, n, win, fft, hop, K
        h = _vp()
        ctx._check(ctx.lib.fluhip_corpus_create(ctx.h, count, n, win, fft, hop, K, ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_corpora"):
            ctx._corpora = []
        ctx._corpora.append(weakref.ref(self))
        self.T = int(ctx.lib.fluhip_corpus_frames(h))
        self.F = int(ctx.lib.fluhip_corpus_bins(h))

    def close(self):
        if self.h:
            if self.ctx.h:
                self.ctx.lib.fluhip_corpus_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_bytes(self):
        return int(self.ctx.lib.fluhip_corpus_device_bytes(self.h))

    def set_audio(self, audio):
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        assert audio.shape == (self.count, self.n)
        self.ctx._check(self.ctx.lib.fluhip_corpus_set_audio_host(self.h, _f(audio)))

    def set_audio_dev(self, dev_ptr: int):
        self.ctx._check(self.ctx.lib.fluhip_corpus_set_audio_dev(self.h, _vp(dev_ptr)))

    def stft(self):
        self.ctx._check(self.ctx.lib.fluhip_corpus_stft(self.h))

    def stft_mag_only(self):
        """the frame-major magnitudes alone (what a spectrogram-only caller runs); nmf() then needs stft() again"""
        self.ctx._check(self.ctx.lib.fluhip_corpus_stft_mag_only(self.h))

    def nmf(self, iters, seed=42, updateW=True, updateH=True, seeds=None, progress=None):
        sarr = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int64)
        sp = sarr.ctypes.data_as(_ip) if sarr is not None else None
        cb = _cb(progress)
        rc = self.ctx.lib.fluhip_corpus_nmf(self.h, iters, int(updateW), int(updateH), seed, sp, cb, None)
        return self.ctx._check(rc, allow=(OK, CANCELLED))

    def set_factors(self, bases_seed=None, acts_seed=None):
        """Seed / Fixed factors for the following nmf() calls: [count, K, F] / [count, K, T] floats, or None for random draws"""
        bs = None if bases_seed is None else np.ascontiguousarray(bases_seed, dtype=np.float32)
        hs = None if acts_seed is None else np.ascontiguousarray(acts_seed, dtype=np.float32)
        assert bs is None or bs.shape == (self.count, self.K, self.F)
        assert hs is None or hs.shape == (self.count, self.K, self.T)
        self.ctx._check(self.ctx.lib.fluhip_corpus_set_factors(self.h, _f(bs), _f(hs)))

    def writeback_dev(self, bases_ptr: int | None, acts_ptr: int | None):
        self.ctx._check(self.ctx.lib.fluhip_corpus_writeback_dev(
            self.h, _vp(bases_ptr) if bases_ptr else None, _vp(acts_ptr) if acts_ptr else None))

    def writeback(self):
        bases = np.empty((self.count, self.K, self.F), dtype=np.float32)
        acts = np.empty((self.count, self.K, self.T), dtype=np.float32)
        self.ctx._check(self.ctx.lib.fluhip_corpus_writeback_host(self.h, _f(bases), _f(acts)))
        return bases, acts

    def keep_spectrum(self, on=True):
        self.ctx._check(self.ctx.lib.fluhip_corpus_keep_spectrum(self.h, int(on)))

    def resynth(self):
        """[count, K, n] f32: every component of every buffer resynthesised (NMFClient.hpp:302-334)"""
        out = np.empty((self.count, self.K, self.n), dtype=np.float32)
        self.ctx._check(self.ctx.lib.fluhip_corpus_resynth_host(self.h, _f(out)))
        return out

    def resynth_interleaved(self, frame_stride=None):
        """fluhip_corpus_resynth_interleaved_host: [n][frame_stride] floats, component k of buffer b in column b K + k"""
        chans = self.count * self.K
        fs = chans if frame_stride is None else frame_stride
        out = np.zeros((self.n, fs), dtype=np.float32)
        self.ctx._check(self.ctx.lib.fluhip_corpus_resynth_interleaved_host(self.h, _f(out), fs))
        return out

    def plan(self):
        out = (ctypes.c_int64 * 8)()
        self.ctx._check(self.ctx.lib.fluhip_corpus_plan(self.h, out))
        keys = ("kernel", "split_w", "split_h", "deferred_norm", "side_column", "strips_w", "padded_rank", "strip")
        d = dict(zip(keys, [int(v) for v in out]))
        d["compute_rank"] = d["padded_rank"] >> 16   # rank the factor updates compute (48 / 96 for the off-size ranks)
        d["padded_rank"] &= 0xFFFF
        d["tail_h"] = d["split_h"] >> 16  # pieces of the tail launch of a two-launch H update (0: one launch)
        d["split_h"] &= 0xFFFF
        return d

    def update_clocks(self, reset=False):
        """per factor update: launches, shader cycles and 100 MHz ticks of one wavefront per launch, summed since the last reset;
        derived: cycles per launch and the clock the part sustained (fluhip_corpus_update_clocks)"""
        out = (ctypes.c_int64 * 8)()
        self.ctx._check(self.ctx.lib.fluhip_corpus_update_clocks(self.h, out, int(reset)))
        res = {}
        for name, o in (("w", 0), ("h", 4)):
            n, cyc, ticks = int(out[o]), int(out[o + 1]), int(out[o + 2])
            res[name] = {"launches": n, "shader_cycles": cyc, "ticks_100mhz": ticks,
                         "cycles_per_launch": cyc / n if n else None,
                         "sustained_mhz": 100.0 * cyc / ticks if ticks else None}
        return res

    def last_loop_ms(self):
        """device time of the last nmf() call's iteration loop (HIP events behind the initialisation / the last launch)"""
        ms = ctypes.c_double(0)
        self.ctx._check(self.ctx.lib.fluhip_corpus_last_loop_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def read_f64(self, mag=True, factors=True):
        m = np.empty((self.count, self.T, self.F)) if mag else None
        W1 = np.empty((self.count, self.K, self.F)) if factors else None
        H1 = np.empty((self.count, self.T, self.K)) if factors else None
        self.ctx._check(self.ctx.lib.fluhip_corpus_read_f64(self.h, _d(m), _d(W1), _d(H1)))
        return m, W1, H1

    def read_layouts_f64(self, mag=True, magT=True, spec=False):
        """fluhip_debug_corpus_read_layouts_f64: (mag [count, Tp, Fp], magT [count, Fp, Tp], spec complex [count, T, F]) as
        they lie on the device, padding included; None for what was not asked for"""
        dims = (ctypes.c_int64 * 5)()
        self.ctx._check(self.ctx.lib.fluhip_debug_corpus_read_layouts_f64(self.h, dims, None, None, None))
        count, Fp, Tp, T, F = (int(v) for v in dims)
        assert (count, T, F) == (self.count, self.T, self.F)
        m = np.empty((count, Tp, Fp)) if mag else None
        mT = np.empty((count, Fp, Tp)) if magT else None
        sp = np.empty((count, T, F, 2)) if spec else None
        self.ctx._check(self.ctx.lib.fluhip_debug_corpus_read_layouts_f64(self.h, None, _d(m), _d(mT), _d(sp)))
        return m, mT, (sp[..., 0] + 1j * sp[..., 1] if spec else None)


class RaggedCorpus(Corpus):
    """fluhip_corpus_create_ragged: mono buffers of DIFFERENT lengths as one device-resident batch.  T / n are those of the
    longest buffer (the shapes read_f64 returns; frames past a buffer's own are zero); Ts holds every buffer's own frames."""

    def __init__(self, ctx: Context, lens, win, fft, hop, K):
        self.ctx = ctx
        self.lens = [int(x) for x in lens]
        self.count, self.n, self.win, self.fft, self.hop, self.K = len(self.lens), max(self.lens), win, fft, hop, K
        arr = (ctypes.c_int64 * self.count)(*self.lens)
        h = _vp()
        ctx._check(ctx.lib.fluhip_corpus_create_ragged(ctx.h, self.count, arr, win, fft, hop, K, ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_corpora"):
            ctx._corpora = []
        ctx._corpora.append(weakref.ref(self))
        self.T = int(ctx.lib.fluhip_corpus_frames(h))
        self.F = int(ctx.lib.fluhip_corpus_bins(h))
        self.Ts = [int(ctx.lib.fluhip_corpus_frames_of(h, i)) for i in range(self.count)]

    def set_audio(self, audios):
        audios = [np.ascontiguousarray(a, dtype=np.float32) for a in audios]
        assert [a.shape[0] for a in audios] == self.lens
        ap = (_fp * self.count)(*[a.ctypes.data_as(_fp) for a in audios])
        self.ctx._check(self.ctx.lib.fluhip_corpus_set_audio_ragged_host(self.h, ap))

    def resynth(self):
        out = [np.empty((self.K, n), dtype=np.float32) for n in self.lens]
        op = (_fp * self.count)(*[o.ctypes.data_as(_fp) for o in out])
        self.ctx._check(self.ctx.lib.fluhip_corpus_resynth_ragged_host(self.h, op))
        return out

    def writeback(self):
        bases = [np.empty((self.K, self.F), dtype=np.float32) for _ in range(self.count)]
        acts = [np.empty((self.K, T), dtype=np.float32) for T in self.Ts]
        bp = (_fp * self.count)(*[b.ctypes.data_as(_fp) for b in bases])
        cp = (_fp * self.count)(*[c.ctypes.data_as(_fp) for c in acts])
        self.ctx._check(self.ctx.lib.fluhip_corpus_writeback_ragged_host(self.h, bp, cp))
        return bases, acts


class Pool:
    """fluhip_pool: several devices (or several contexts on one) behind one host process."""

    def __init__(self, devices=None, lib: ctypes.CDLL | None = None):
        self.lib = lib or load_library()
        h = _vp()
        if devices is None:
            rc = self.lib.fluhip_pool_create(None, 0, ctypes.byref(h))
        else:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = self.lib.fluhip_pool_create(arr, len(devices), ctypes.byref(h))
        if rc != OK:
            raise FluhipError(rc, "fluhip_pool_create failed (no usable device?)")
        self.h = h

    def close(self):
        if self.h:
            self.lib.fluhip_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return int(self.lib.fluhip_pool_size(self.h))

    def devices(self):
        return [int(self.lib.fluhip_pool_device(self.h, i)) for i in range(self.size())]

    def bufnmf(self, audio, win, fft, hop, K, iters, seed=42, updateW=True, updateH=True, seeds=None, progress=None):
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        count, n = audio.shape
        F, T = fft // 2 + 1, int(self.lib.fluhip_stft_num_frames(n, win, hop))
        bases = np.empty((count, K, F), dtype=np.float32)
        acts = np.empty((count, K, T), dtype=np.float32)
        sarr = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int64)
        cb = _cb(progress)
        rc = self.lib.fluhip_pool_bufnmf_f32(self.h, _f(audio), count, n, win, fft, hop, K, iters, int(updateW), int(updateH),
                                             seed, sarr.ctypes.data_as(_ip) if sarr is not None else None, _f(bases), _f(acts),
                                             cb, None)
        if rc not in (OK, CANCELLED):
            raise FluhipError(rc, self.lib.fluhip_pool_last_error(self.h).decode())
        return bases, acts, rc

    def bufmfcc(self, audio, win, fft, hop, n_bands=40, n_coefs=13, start_coeff=0, lo=20.0, hi=20000.0, sr=44100.0,
                padding_mode=1):
        """fluhip_pool_bufmfcc_f32: BASELINE config 5 over several devices, slices dealt in contiguous blocks"""
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        T = Context.feature_frames(n, win, hop, padding_mode)
        out = np.empty((count, n_coefs, T), dtype=np.float32)
        Tr = _i64(0)
        rc = self.lib.fluhip_pool_bufmfcc_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, n_coefs, start_coeff, lo, hi, sr,
                                              padding_mode, _f(out), ctypes.byref(Tr))
        if rc != OK:
            raise FluhipError(rc, self.lib.fluhip_pool_last_error(self.h).decode())
        assert Tr.value == T
        return out

    def bufmelbands(self, audio, win, fft, hop, n_bands=40, lo=20.0, hi=20000.0, sr=44100.0, normalize=True, scale_db=False,
                    padding_mode=1):
        audio = np.ascontiguousarray(np.atleast_2d(audio), dtype=np.float32)
        count, n = audio.shape
        T = Context.feature_frames(n, win, hop, padding_mode)
        out = np.empty((count, n_bands, T), dtype=np.float32)
        Tr = _i64(0)
        rc = self.lib.fluhip_pool_bufmelbands_f32(self.h, _f(audio), count, n, win, fft, hop, n_bands, lo, hi, sr, int(normalize),
                                                  int(scale_db), padding_mode, _f(out), ctypes.byref(Tr))
        if rc != OK:
            raise FluhipError(rc, self.lib.fluhip_pool_last_error(self.h).decode())
        assert Tr.value == T
        return out

    def bufnmf_job(self, audio, win, fft, hop, K, iters, seed=42, updateW=True, updateH=True, seeds=None, bases_seed=None,
                   acts_seed=None, resynth=False, progress=None):
        """fluhip_pool_bufnmf_job_f32: the batched form with Seed / Fixed factors and the resynthesis output"""
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        count, n = audio.shape
        F, T = fft // 2 + 1, int(self.lib.fluhip_stft_num_frames(n, win, hop))
        bases = np.empty((count, K, F), dtype=np.float32)
        acts = np.empty((count, K, T), dtype=np.float32)
        res = np.empty((count, K, n), dtype=np.float32) if resynth else None
        sarr = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int64)
        bs = None if bases_seed is None else np.ascontiguousarray(bases_seed, dtype=np.float32)
        hs = None if acts_seed is None else np.ascontiguousarray(acts_seed, dtype=np.float32)
        job = BufNMFJob(count, n, win, fft, hop, K, iters, int(updateW), int(updateH), seed,
                        sarr.ctypes.data_as(_ip) if sarr is not None else None, _f(audio), _f(bs), _f(hs), _f(bases), _f(acts),
                        _f(res))
        rc = self.lib.fluhip_pool_bufnmf_job_f32(self.h, ctypes.byref(job), _cb(progress), None)
        if rc not in (OK, CANCELLED):
            raise FluhipError(rc, self.lib.fluhip_pool_last_error(self.h).decode())
        return bases, acts, res, rc

    def bufnmf_ragged(self, audios, win, fft, hop, K, iters, seed=42, updateW=True, updateH=True, seeds=None, progress=None):
        """buffers of different lengths: lists of per-buffer bases [K,F] and activations [K,T_i]"""
        audios = [np.ascontiguousarray(a, dtype=np.float32) for a in audios]
        count = len(audios)
        F = fft // 2 + 1
        Ts = [int(self.lib.fluhip_stft_num_frames(a.shape[0], win, hop)) for a in audios]
        bases = [np.empty((K, F), dtype=np.float32) for _ in range(count)]
        acts = [np.empty((K, T), dtype=np.float32) for T in Ts]
        fpp = ctypes.POINTER(ctypes.c_float)
        ap = (fpp * count)(*[a.ctypes.data_as(fpp) for a in audios])
        bp = (fpp * count)(*[b.ctypes.data_as(fpp) for b in bases])
        cp = (fpp * count)(*[c.ctypes.data_as(fpp) for c in acts])
        lens = (ctypes.c_int64 * count)(*[a.shape[0] for a in audios])
        sarr = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int64)
        cb = _cb(progress)
        rc = self.lib.fluhip_pool_bufnmf_ragged_f32(self.h, ap, lens, count, win, fft, hop, K, iters, int(updateW), int(updateH),
                                                    seed, sarr.ctypes.data_as(_ip) if sarr is not None else None, bp, cp, cb, None)
        if rc not in (OK, CANCELLED):
            raise FluhipError(rc, self.lib.fluhip_pool_last_error(self.h).decode())
        return bases, acts, rc
