"""CPU side of the length-masked extraction: the padded batching rule (ingest.pad_batches), the padded native reader
(spk_ark_read_padded / ArkTable.read_padded) against kaldi_io, the new C symbols, and the argument checks of the masked entries
(host-side: they refuse before any launch)."""
import os
import re

import numpy as np
import pytest
import torch

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import hip, ingest, kaldi_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lengths(seed, n=2000):
    rng = np.random.RandomState(seed)
    return np.clip(rng.lognormal(np.log(700), 0.5, n), 400, 3000).astype(np.int64)


@pytest.mark.parametrize("seed,bs,ratio,quantum", [(0, 64, 0.1, 8), (1, 16, 0.05, 8), (2, 128, 0.2, 16), (3, 1, 0.1, 8)])
def test_pad_batches_properties(seed, bs, ratio, quantum):
    L = _lengths(seed)
    batches = ingest.pad_batches(L, bs, max_pad_ratio=ratio, quantum=quantum)
    seen = np.concatenate([b for b, _ in batches])
    assert sorted(seen.tolist()) == list(range(len(L)))                 # every utterance exactly once
    for idx, T in batches:
        assert 1 <= len(idx) <= bs
        assert T % quantum == 0 and T >= L[idx].max() and T - L[idx].max() < quantum
        if len(idx) > 1:
            assert len(idx) * T <= (1 + ratio) * L[idx].sum()
    again = ingest.pad_batches(L, bs, max_pad_ratio=ratio, quantum=quantum)
    assert len(again) == len(batches) and all(np.array_equal(a, b) and s == t for (a, s), (b, t) in zip(again, batches))
    # sorted by length: batches do not interleave
    mx = [L[b].max() for b, _ in batches]
    mn = [L[b].min() for b, _ in batches]
    assert all(mx[i] <= mn[i + 1] for i in range(len(batches) - 1))


def test_pad_batches_groups_equal_lengths_and_rejects_bad_input():
    b = ingest.pad_batches([100] * 10 + [5], 4)
    assert [len(i) for i, _ in b] == [1, 4, 4, 2] and [t for _, t in b] == [8, 104, 104, 104]
    assert ingest.pad_batches([], 4) == []
    with pytest.raises(ValueError):
        ingest.pad_batches([3, 0], 4)
    with pytest.raises(ValueError):
        ingest.pad_batches([3, 4], 0)


def _write_ark(tmp_path, mats, name="feats"):
    ark, scp = str(tmp_path / (name + ".ark")), str(tmp_path / (name + ".scp"))
    with open(ark, "wb") as f, open(scp, "w") as s:
        for i, m in enumerate(mats):
            f.write(("u%d " % i).encode())
            off = kaldi_io.write_mat(f, m)
            s.write("u%d %s:%d\n" % (i, ark, off))
    return scp


def test_read_padded_is_exact_with_zero_tails(tmp_path):
    rng = np.random.RandomState(3)
    F = 23
    lens = [37, 1, 64, 50, 63]
    mats = [rng.randn(n, F).astype(np.float32) for n in lens]
    scp = _write_ark(tmp_path, mats)
    rx = [l.split()[1] for l in open(scp)]
    tab = ingest.ArkTable(rx)
    assert tab.rows.tolist() == lens and (tab.cols == F).all()
    T = 72
    idx = np.array([4, 0, 1, 2, 3])
    out = torch.full((5, F, T), float("nan"))
    tab.read_padded(idx, T, out, nthreads=3)
    for j, i in enumerate(idx):
        ref = kaldi_io.read_mat(rx[i]).T
        assert np.array_equal(out[j, :, :lens[i]].numpy(), ref)
        assert (out[j, :, lens[i]:] == 0).all()
    # a batch whose longest utterance does not fit T is refused, as the crop reader refuses a short utterance
    with pytest.raises(RuntimeError, match="spk_ark_read_padded"):
        tab.read_padded(idx, 63, torch.empty(5, F, 63), nthreads=2)


def test_read_padded_takes_float32_only(tmp_path):
    """the native reader accepts 'FM ' matrices only: a float64 ark fails in the header probe, the same error read_crop users get"""
    scp = _write_ark(tmp_path, [np.zeros((4, 3), dtype=np.float64)], name="dm")
    with pytest.raises(RuntimeError, match="unsupported"):
        ingest.ArkTable([l.split()[1] for l in open(scp)])


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    for name in ("spk_conv_mfma_len", "spk_stem_conv_fwd_len", "spk_stats_pool_fwd_len"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols()
        assert hasattr(hip.lib(), name)
    assert re.search(r"\bspk_ark_read_padded\s*\(", open(os.path.join(ROOT, "include", "spkio.h")).read())
    assert hasattr(ingest.lib(), "spk_ark_read_padded")
    assert hip.EPI_WMASK == 1 << 24


def test_masked_entries_refuse_bad_flag_combinations():
    """SPK_EPI_WMASK only where it is implemented; refused on the host before any launch (no GPU needed)"""
    lib = hip.lib()
    i3 = (hip._I * 9)(*range(9))

    def conv(name, flags, wlen):
        args = [1, 1, 1] + [None] * 18 + [1, 8, 8, 64, 8, 8, 8, 8, 64, 1, 1, 0, 0, 9, i3, i3, i3, 8, 8, 1, 1, 1, 1, flags, 0,
                                          None, None, None]
        return getattr(lib, name)(*(args + ([wlen] if name.endswith("_len") else []) + [None]))

    assert conv("spk_conv_mfma", hip.EPI_WMASK | hip.EPI_AFFINE, None) < 0             # no wlen on the plain entry
    assert b"WMASK" in lib.spk_last_error()
    assert conv("spk_conv_mfma_len", hip.EPI_AFFINE, 1) < 0                             # wlen without the flag
    for extra in (hip.IN_BNBWD, hip.EPI_BNBWD, hip.IN_PRESPLIT, hip.CONV_WS):
        assert conv("spk_conv_mfma_len", hip.EPI_WMASK | extra, 1) < 0
        assert b"WMASK" in lib.spk_last_error()
    assert lib.spk_stem_conv_fwd(1, 1, 1, None, None, None, 1, 8, 8, hip.EPI_WMASK, None, None) < 0
    assert lib.spk_stem_conv_fwd_len(1, 1, 1, None, None, None, 1, 8, 8, 0, None, 1, None) < 0
    assert lib.spk_stem_conv_fwd_len(1, 1, 1, None, None, None, 1, 8, 8, hip.EPI_WMASK, None, None, None) < 0
    assert lib.spk_stats_pool_fwd_len(1, 1, None, 1, 1, 1, 1, 1, None) < 0
    assert lib.spk_conv1x1_stream(*([1, 1, 1] + [None] * 8 + [64, 64, hip.EPI_WMASK, 1, None, 1, None])) < 0
    assert lib.spk_conv3x3_c32_stream(1, 1, 1, None, None, None, 1, 8, 8, hip.EPI_WMASK, 1, None, 1, None) < 0
