"""ctypes binding of libspkhip.so (include/spkhip.h).  Fails loudly when the library is missing:
there is no CPU or eager-PyTorch fallback anywhere in this package."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SPK_LIB", os.path.join(_HERE, "libspkhip.so"))   # SPK_LIB: A/B builds of the same ABI

IN_AFFINE_RELU, EPI_AFFINE, EPI_ADD, EPI_RELU, EPI_STATS, EPI_BNBWD, IN_BNBWD, CONV_WS = 1, 2, 4, 8, 16, 32, 64, 128
CONV_PIPE = 1024
WGRAD_GROUPS = 2048        # spk_conv_wgrad flags: 1x1 f16x3 kernel with 1 << (bits 12-13) input-channel groups per block
IN_PRESPLIT, SIDE_PRESPLIT, DY_PRESPLIT = 1 << 14, 1 << 15, 1 << 16     # f16 pair tensors (include/spkhip.h)
CONV_M16 = 1 << 17      # 16x16x32 form of the pipelined convolution
CONV_CK32 = 1 << 23     # fused BatchNorm-backward data gradient at Cin = 32 (f16x3): whole 128-byte pixels per staging pass
WGRAD_NOSHIFT = 1 << 18  # 3x3 grouped weight gradient: plain K loop instead of the shifted-window form (A/B)
WGRAD_M16 = 1 << 19      # 3x3 grouped weight gradient on 16x16x32 with dy (a pair tensor) staged by LDS DMA
EPI_WMASK = 1 << 24     # length-masked epilogue: outputs at width x >= wlen[b] stored as 0 (spk_conv_mfma_len, spk_stem_conv_fwd_len)
PTR_ADD_MASK, PTR_BN_MASK, PTR_IN_MASK, PTR_IN_ACT, PTR_BN_ACT, PTR_SIDE_DZ = 1, 2, 4, 8, 16, 32   # spk_conv_variant_of `ptrs`
MASK_NONE, MASK_ACT, MASK_RAW, MASK_BITS = 0, 1, 2, 3

_P = ctypes.c_void_p
_I = ctypes.c_int
_L = ctypes.c_longlong
_F = ctypes.c_float
_D = ctypes.c_double
_IP = ctypes.POINTER(ctypes.c_int)


def _frontend_sig(mfcc, span):
    """spk_{fbank,mfcc}[_span]_fwd: one parameter list, with the four span pointers and the cepstral arguments where they apply"""
    def cep(*t):
        return list(t) if mfcc else []
    return ([_P, _P] + [_P] * 4 * span + [_P, _I, _L]      # wave, nsamp, (first, total, frame0, nframes,) utt_ids, B, Nmax
            + [_P] * 5 + cep(_P, _P)                        # window, twiddle, mel_w, mel_lo, mel_off (, dct, lifter)
            + [_I] * 4 + cep(_I) + [_I, _F, _F, _I, _F]     # L, S, P, F (, C), snip_edges, dither, preemph, remove_dc, energy_floor
            + cep(_I, _I)                                   # (use_energy, htk_compat)
            + [ctypes.c_ulonglong, _P, _P, _P, _I, _P])     # seed, feats, log_energy, T_out, Tcap, stream


_SIGS = {
    "spk_pack_conv_weight": [_P, _P, _I, _I, _I, _I, _I, _P],
    "spk_pack_conv_weight_split": [_P, _P, _I, _I, _I, _I, _I, _I, _P],
    "spk_pack_job_bytes": [],
    "spk_build_flags": [],
    "spk_pack_conv_weights_batched": [_P, _I, _I, _I, _P],
    "spk_conv_mfma": [_P] * 21 + [_I] * 14 + [_IP, _IP, _IP] + [_I] * 8 + [_P, _P, _P, _P],
    "spk_conv_mfma_len": [_P] * 21 + [_I] * 14 + [_IP, _IP, _IP] + [_I] * 8 + [_P, _P, _P, _P, _P],
    "spk_conv3x3_c32_stream": [_P] * 6 + [_I] * 4 + [_P, _P, _I, _P],
    "spk_conv1x1_stream": [_P] * 11 + [_L, _I, _I, _P, _P, _I, _P],
    "spk_conv1x1_stream_rows": [_I, _I],
    "spk_conv_wgrad": [_P] * 6 + [_I] * 16 + [_P, _P, _P],
    "spk_conv_wgrad_limits": [_I, _IP, _IP],
    "spk_wgrad_reduce": [_P, _P, _I, _I, _I, _I, _I, _P],
    "spk_conv_variant_of": [_I, _I, _I, _I, _I],       # host only: the FL / VAR instance a launch takes, -1 = generic
    "spk_wgrad_variant_of": [_I, _I, _I, _I, _I, _I, _I],
    "spk_stem_fwd_blocks": [_I, _I, _I],
    "spk_stem_conv_fwd": [_P] * 6 + [_I] * 4 + [_P, _P],
    "spk_stem_conv_fwd_len": [_P] * 6 + [_I] * 4 + [_P, _P, _P],
    "spk_stem_wgrad_blocks": [_I, _I, _I],
    "spk_stem_conv_wgrad": [_P] * 4 + [_I] * 4 + [_P],
    "spk_stem_stats": [_P] * 3 + [_I] * 3 + [_P],
    "spk_stem_fwd_apply": [_P] * 8 + [_I] * 3 + [_P],
    "spk_stem_bwd_wgrad": [_P] * 10 + [_I] * 4 + [_P],
    "spk_bn_stats_blocks": [_L, _I],
    "spk_bn_stats_partial": [_P, _P, _L, _I, _P],
    "spk_bn_finalize": [_P, _I, _I, _D] + [_P] * 9 + [_F, _F, _P, _P, _P, _P],
    "spk_bn_eval_coeffs": [_P] * 6 + [_I, _F, _P],
    "spk_bn_apply": [_P] * 8 + [_L, _I, _I, _P, _P],
    "spk_bn_bwd_reduce": [_P] * 8 + [_L, _I, _I, _P, _P],
    "spk_bn_bwd_finalize": [_P, _I, _I, _D] + [_P] * 5 + [_I, _P, _P, _P, _P, _P, _P, _P],
    "spk_bn_bwd_apply": [_P] * 10 + [_L, _I, _I, _P, _P, _P],
    "spk_absmax": [_P, _P, _L, _P],
    "spk_bnbwd_estimate": [_P, _P, _P, _I, _P, _P, _P, _P],
    "spk_f16_window_count": [_P, _P, _P, _L, _I, _P, _I, _P, _P],
    "spk_affine_estimate": [_P, _P, _I, _P, _P, _P],
    "spk_se_chunks": [_L],
    "spk_se_squeeze": [_P, _P, _P, _I, _I, _I, _I, _P, _P],
    "spk_se_excite": [_P] * 8 + [_I] * 5 + [_P, _P],
    "spk_se_apply": [_P] * 9 + [_I] * 5 + [_P, _P, _P],
    "spk_se_bwd_reduce": [_P] * 5 + [_I, _L, _I, _I, _P, _P],
    "spk_se_bwd_gate": [_P] * 20 + [_I] * 4 + [_L] + [_P] * 5,
    "spk_se_bwd_apply": [_P] * 10 + [_I, _L, _I, _I, _P, _P, _P],
    "spk_stats_pool_fwd": [_P, _P, _I, _I, _I, _I, _I, _P],
    "spk_stats_pool_fwd_len": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "spk_stats_pool_bwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "spk_stats_pool_row_form": [_I],
    "spk_stats_pool_row_cap": [],
    "spk_h16_packed_bytes": [_I, _I, _I, _I],
    "spk_h16_pack_conv_weight": [_P, _P, _I, _I, _I, _I, _P],
    "spk_h16_conv_tile": [_I],
    "spk_h16_stem_fwd": [_P] * 7 + [_I] * 3 + [_P],
    "spk_h16_conv_fwd": [_P] * 8 + [_I] * 8 + [_P],
    "spk_h16_stats_pool_fwd": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "spk_gemm_f32": [_P] * 4 + [_I] * 3 + [_L] * 5 + [_F, _I, _P, _P],
    "spk_gemm_splitk": [_I, _I, _I],
    "spk_colsum": [_P, _P, _I, _I, _I, _P],
    "spk_l2norm_fwd": [_P, _P, _P, _I, _I, _F, _P],
    "spk_l2norm_bwd": [_P, _P, _P, _P, _I, _I, _F, _I, _P],
    "spk_aam_margin_fwd": [_P, _P, _P, _I, _I, _F, _F, _P],
    "spk_aam_margin_bwd": [_P, _P, _P, _P, _I, _I, _F, _F, _P],
    "spk_softmax_ce": [_P] * 5 + [_I, _I, _F, _P],
    "spk_mean": [_P, _P, _I, _P],
    "spk_relu_bwd": [_P, _P, _P, _L, _P],
    "spk_sgd_step": [_P, _P, _P, _L, _F, _F, _F, _F, _I, _P],
    "spk_center_normalize": [_P, _P, _P, _I, _I, _F, _P],
    "spk_trial_cosine": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "spk_topk_mean_std": [_P, _P, _P, _I, _I, _I, _L, _P],
    "spk_fbank_tile_frames": [_I, _I, _I, _I],
    "spk_fbank_fwd": _frontend_sig(False, False),
    "spk_mfcc_tile_frames": [_I, _I, _I, _I, _I],
    "spk_mfcc_fwd": _frontend_sig(True, False),
    "spk_fbank_span_fwd": _frontend_sig(False, True),
    "spk_mfcc_span_fwd": _frontend_sig(True, True),
    "spk_pcm16_to_f32": [_P, _P, _I, _L, _P, _P],
    "spk_fbank_dither_noise":[_P, _L, ctypes.c_ulonglong, _I, _I, _I, _P],
    "spk_vad_count": [_P, _P, _I, _I, _D, _D, _I, _D, _P, _P, _P, _P],
    "spk_vad_segments": [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P, _P],
    "spk_cmn_select": [_P] * 6 + [_I] * 5 + [_P],
    "spk_resample_tile": [_I, _I, _I],
    "spk_resample_fwd": [_P, _P, _I, _L, _P, _P, _I, _I, _I, _P, _P, _L, _P],
    "spk_augment_max_rir": [],
    "spk_augment_max_early": [],
    "spk_augment_workspace": [_I, _L, _I, _I, _L, _I, ctypes.POINTER(_L)],
    "spk_cm_decode": [_P, _P, _P, _I, _I, _I, _P, _P],
    "spk_cm_compress": [_P, _P, _I, _I, _I, _P, _P, _P, _P, _P],
    "spk_eval_tile": [_I],
    "spk_segment_mean": [_P, _P, _P, _P, _I, _I, _I, _P],
    "spk_trial_snorm": [_P, _I] + [_P] * 7 + [_I, _P],
    "spk_sort_trials": [_P, _P, _P, _I, _P],
    "spk_error_sweep": [_P, _P, _P, _P, _I, _P, _P, _P, _I, _P],
    "spk_scatter_slab_rows": [_L],
    "spk_scatter_f64": [_P, _I, _L, _P, _P, _P, _P, _L, _I, _P],
    "spk_segment_sum_f64": [_P, _I, _L, _P, _P, _P, _P, _I, _I, _I, _P],
    "spk_affine_lennorm": [_P, _I, _L, _P, _P, _P, _I, _P, _I, _L, _I, _I, _P],
    "spk_plda_posterior_rows": [_P] * 5 + [_I, _I, _P],
    "spk_plda_llr": [_P] * 8 + [_I, _P, _I, _I, _I, _I, _P],
    "spk_window_gather": [_P, _I, _I, _I, _IP, _IP, _IP, _P, _P, _I, _I, _P],
    "spk_window_mean": [_P, _I, _I, _IP, _P, _P, _P, _I, _P],
    "spk_diar_tables": [_P, _I, _L, _P],                # host only: rec_off (host int64) -> rec_off / mat_off / tile_off
    "spk_score_dense_q": [_P, _P, _D, _P, _L, _I, _P],
    "spk_score_dense": [_P, _P, _P, _P, _P, _D, _P, _L, _I, _I, _P],
    "spk_ahc_threads": [],
    "spk_ahc_max_n": [],
    "spk_ahc_batch": [_P, _P, _P, _P, _P, _P, _L, _P, _P, _P, _P, _L, _I, _P],
    "spk_vbx_threads": [],
    "spk_vbx_max_states": [],
    "spk_vbx_ws_elems": [_P, _I, _I, _I],               # host only; returns long long (restype set in lib())
    "spk_vbx_batch": [_P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _I, _D, _P, _L, _P, _P, _L, _I, _I, _I, _P],
    "spk_syevj_max_dim": [],
    "spk_syevj_max_sweeps": [],
    "spk_syevj_threads": [],
    "spk_syevj_ws_elems": [_I, _I],                     # host only; returns long long (restype set in lib())
    "spk_syevj_batch": [_P, _P, _P, _P, _L, _P, _P, _P, _P, _I, _I, _P],
    "spk_pca_plda_ws_elems": [_P, _I, _I],              # host only; returns long long
    "spk_pca_plda_batch": [_P] * 8 + [_D, _P, _L] + [_P] * 6 + [_L, _I, _I, _P],
    "spk_pca_score_terms": [_P] * 5 + [_I, _I, _P],
    "spk_affine_lennorm_rec": [_P] * 7 + [_I, _P, _L, _I, _I, _P],
    "spk_score_dense_q_rec": [_P, _P, _P, _P, _D, _P, _L, _I, _I, _P],
    "spk_score_dense_rec": [_P] * 7 + [_L, _I, _I, _P],
    "spk_augment_fwd": [_P, _P, _I, _L, _P, _L, _P, _P, _I, _I, _P, _L, _P, _P, _P, _P, _I, _L, _P, _P, _P, _P, _I, _P, _P, _P],
}

# diarization scoring (include/spkder.h, csrc/der.hip): declared in a header of its own and counted apart from include/spkhip.h
_DER_SIGS = {
    "spk_ahc_cut_batch": [_P] * 6 + [_I, _P, _L, _I, _P],
    "spk_der_pieces": [_P] * 5 + [_I, _P, _P, _L, _I, _P],
    "spk_der_max_ref": [],
    "spk_der_max_hyp": [],
    "spk_der_max_turns": [],
    "spk_der_ws_elems": [_I, _I, _I],                   # host only; returns long long
    "spk_der_batch": [_P, _P, _P, _L, _I, _P, _P, _I, _P, _P, _P, _L, _P, _L, _P, _P, _P],
}

# calibration and fusion of trial scores (include/spkcal.h, csrc/cal.hip): the third header, counted apart from the other two
_CAL_SIGS = {
    "spk_cal_max_k": [],
    "spk_cal_tile": [_I],
    "spk_cal_apply": [_P, _P, _I, _P, _I, _P],
    "spk_cal_cllr_ws_elems": [_I],                      # host only; the three *_ws_elems return long long
    "spk_cal_train_ws_elems": [_I, _I],
    "spk_cal_pav_ws_elems": [_I],
    "spk_cal_cllr": [_P, _P, _P, _P, _I, _P, _P, _P, _L, _I, _P],
    "spk_cal_train": [_P, _P, _I, _I, _L, _D, _D, _D, _D, _I, _P, _P, _P, _L, _P],
    "spk_cal_pav": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _P],
}

# training from audio with speed perturbation (include/spkwav.h, csrc/resample.hip): the fourth header; its names are spkw_*, so the
# set of spk_* exports that the other three tables pin is as it was
_WAV_SIGS = {
    "spkw_resample_span_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _L, _P, _P, _I, _I, _I, _P, _L, _P],
    "spkw_copy_rows_fwd": [_P, _P, _P, _I, _I, _L, _P, _L, _P],
}

# speaker-level bootstrap of the error-rate sweep (include/spkboot.h, csrc/boot.hip): the fifth header; its names are spkb_*
_BOOT_SIGS = {
    "spkb_limit": [_I],
    "spkb_pitch": [_I],
    "spkb_group": [_I],
    "spkb_pack": [_P, _P, _P, _P, _P, _P, _I, _P, _P, _I, _I, _P],
    "spkb_sweep_ws_elems": [_I, _I, _I, _I],            # host only; returns long long
    "spkb_sweep": [_P, _P, _I, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _L, _I, _I, _P],
}

_lib = None


def lib():
    """Load libspkhip.so (built by build.py / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH) and "SPK_LIB" not in os.environ:
            # not built yet (fresh checkout): compile it now with hipcc; there is no other implementation to fall back to
            try:
                import importlib.util
                spec = importlib.util.spec_from_file_location("spk_build", os.path.join(_HERE, "build.py"))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                mod.build(force=True, verbose=False)
            except Exception as e:
                raise RuntimeError("libspkhip.so is missing at %s and building it failed (%s). Run `python "
                                   "__graft_entry__.py build` (hipcc --offload-arch=gfx950). There is no fallback path."
                                   % (LIB_PATH, e))
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libspkhip.so is missing at %s: run `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950). There is no fallback path." % LIB_PATH)
        l = ctypes.CDLL(LIB_PATH)
        l.spk_last_error.restype = ctypes.c_char_p
        l.spk_version.restype = ctypes.c_int
        l.spk_conv_wgrad_workspace.restype = ctypes.c_size_t
        l.spk_conv_wgrad_workspace.argtypes = [_I, _I, _I, _I]
        l.spk_bn_finalize_workspace.restype = ctypes.c_size_t
        l.spk_bn_finalize_workspace.argtypes = [_I, _I]
        l.spk_gemm_workspace.restype = ctypes.c_size_t
        l.spk_gemm_workspace.argtypes = [_I, _I, _I]
        l.spk_sort_trials_workspace.restype = ctypes.c_size_t
        l.spk_sort_trials_workspace.argtypes = [_I]
        l.spk_error_sweep_workspace.restype = ctypes.c_size_t
        l.spk_error_sweep_workspace.argtypes = [_I, _I]
        l.spk_scatter_f64_workspace.restype = ctypes.c_size_t
        l.spk_scatter_f64_workspace.argtypes = [_L, _I]
        for name, sig in (list(_SIGS.items()) + list(_DER_SIGS.items()) + list(_CAL_SIGS.items()) + list(_WAV_SIGS.items())
                          + list(_BOOT_SIGS.items())):
            fn = getattr(l, name)
            fn.argtypes = sig
            fn.restype = ctypes.c_int
        l.spk_vbx_ws_elems.restype = ctypes.c_longlong
        l.spk_syevj_ws_elems.restype = ctypes.c_longlong
        l.spk_pca_plda_ws_elems.restype = ctypes.c_longlong
        l.spk_der_ws_elems.restype = ctypes.c_longlong
        for name in ("spk_cal_cllr_ws_elems", "spk_cal_train_ws_elems", "spk_cal_pav_ws_elems", "spkb_sweep_ws_elems"):
            getattr(l, name).restype = ctypes.c_longlong
        if os.environ.get("SPK_POOL_ROWS", "1") == "0":      # A/B: the serial two-pass pooling forward at every width
            l.spk_stats_pool_row_form(0)
        _lib = l
    return _lib


def has_experimental():
    """the library was built with SPK_EXPERIMENTAL=1: the measured, not-faster kernel forms are present"""
    return bool(lib().spk_build_flags() & 1)


def exported_symbols():
    return ["spk_version", "spk_last_error", "spk_conv_wgrad_workspace", "spk_bn_finalize_workspace", "spk_gemm_workspace",
            "spk_sort_trials_workspace", "spk_error_sweep_workspace", "spk_scatter_f64_workspace"] + list(_SIGS)


def der_symbols():
    """the exports include/spkder.h declares"""
    return list(_DER_SIGS)


def cal_symbols():
    """the exports include/spkcal.h declares"""
    return list(_CAL_SIGS)


def wav_symbols():
    """the exports include/spkwav.h declares"""
    return list(_WAV_SIGS)


def boot_symbols():
    """the exports include/spkboot.h declares"""
    return list(_BOOT_SIGS)


def ptr(t):
    """Device pointer of a tensor (None -> NULL). Requires a contiguous fp32/fp16/int64/int32 CUDA(HIP) tensor."""
    if t is None:
        return None
    assert t.is_cuda, "libspkhip takes device tensors only"
    assert t.is_contiguous(), "libspkhip takes contiguous tensors only"
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(rc, name):
    if rc != 0:
        msg = lib().spk_last_error().decode()
        raise RuntimeError("%s failed (rc=%d): %s" % (name, rc, msg))


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    check(rc, name)
