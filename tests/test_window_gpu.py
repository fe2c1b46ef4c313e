"""Windowed extraction on the GPU (csrc/window.hip, Engine.predict_windows, decode.py --window) against
tests/window_ref.py.

spk_window_gather: the output is the slices bit for bit, the padding +0.  spk_window_mean: every element within
(K + 2) 2^-24 sum w |e| / tot of the fp64 mean (window_ref.mean_ref: derived from the kernel's K fused multiply-adds, the reciprocal
and the final multiply; nothing measured).  predict_windows: every row against predict() of its window run alone, by the bar
tests/test_masked_predict_gpu.py holds a padded row to against the row run alone (close: 1 - cos < 1e-6, scale-relative error
< 2e-5; a window whose pooled width is one frame is NaN where the solo run is); precision="f16" by the bar of tests/test_half_gpu.py
(the distance to the exact fp64 embedding within twice the distance of the CPU emulation of the half contract).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import half_ref as H  # noqa: E402
import window_ref as R  # noqa: E402
from test_half_gpu import make_model  # noqa: E402
from test_masked_predict_gpu import _read_vectors, close  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


def bits(t):
    return t.contiguous().view(torch.int32)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device="cuda")


# ---- spk_window_gather ------------------------------------------------------------------------------------------------------------
def edge_plan(B, T, Wcap, seed):
    """starts {0, 1, 2, 3, 4, T - len} x lengths {1, 3, 4, 8, 9} (those that fit Wcap), the source rows cycling so that windows of
    one row overlap, two identical windows, everything shuffled"""
    plan = []
    for l in (1, 3, 4, 8, 9):
        if l > Wcap:
            continue
        for s in (0, 1, 2, 3, 4, T - l):                  # T - l: the window ends exactly at T
            plan.append((len(plan) % B, s, l))
    plan += [(1, 2, min(8, Wcap)), (1, 4, min(8, Wcap)), (1, 4, min(8, Wcap))]          # overlapping windows of one row, one twice
    order = np.random.RandomState(seed).permutation(len(plan))
    row, start, length = (np.asarray(v, dtype=np.int64)[order] for v in zip(*plan))
    assert (start + length == T).any()
    return row, start, length


def check_gather(ops, src, row, start, length, Wcap, out=None):
    got = ops.window_gather(src, row, start, length, Wcap, out=out)
    torch.cuda.synchronize()
    want = torch.from_numpy(R.gather_ref(src.cpu().numpy(), row, start, length, Wcap))
    assert got.shape == want.shape
    assert torch.equal(bits(got.cpu()), bits(want)), "not the slices bit for bit"          # padding: +0, whatever out held
    return got


@pytest.mark.parametrize("Wcap", [8, 12, 16])
@pytest.mark.parametrize("F", [5, 1])
def test_gather_is_the_slices(ops, Wcap, F):
    B, T = 3, 37
    src = torch.randn(B, F, T, generator=torch.Generator().manual_seed(Wcap + F)).cuda()
    src[0, 0, 3] = float("-0.0")
    src[1, 0, 5] = float("inf")
    row, start, length = edge_plan(B, T, Wcap, 7)
    N = len(row)
    check_gather(ops, src, row, start, length, Wcap, out=nan_like(N, F, Wcap))


@pytest.mark.parametrize("Wcap,src_off,out_off", [(8, 1, 0), (8, 0, 1), (8, 3, 2), (10, 0, 0), (9, 1, 3), (1, 0, 0)])
def test_gather_unaligned_buffers_and_widths(ops, Wcap, src_off, out_off):
    """a source or an output that starts 4, 8 or 12 bytes off a 16-byte boundary, a Wcap that is no multiple of 4: the 4-byte paths"""
    B, F, T = 3, 5, 37
    flat = torch.randn(B * F * T + 4, generator=torch.Generator().manual_seed(Wcap)).cuda()
    src = flat[src_off:src_off + B * F * T].view(B, F, T)
    row, start, length = edge_plan(B, T, Wcap, 9)
    N = len(row)
    obuf = nan_like(N * F * Wcap + 4)
    out = obuf[out_off:out_off + N * F * Wcap].view(N, F, Wcap)
    check_gather(ops, src, row, start, length, Wcap, out=out)
    assert torch.isnan(obuf[:out_off]).all() and torch.isnan(obuf[out_off + N * F * Wcap:]).all()     # nothing outside `out`


def test_gather_more_rows_than_a_grid_dimension(ops):
    N, B, F, T, Wcap = 14000, 7, 5, 12, 4           # N * F = 70 000 output rows > 65 535
    rng = np.random.RandomState(1)
    src = torch.randn(B, F, T, generator=torch.Generator().manual_seed(2)).cuda()
    length = rng.randint(1, Wcap + 1, size=N)
    start = np.array([rng.randint(0, T - l + 1) for l in length])
    row = rng.randint(0, B, size=N)
    check_gather(ops, src, row, start, length, Wcap, out=nan_like(N, F, Wcap))


def test_gather_refusals_leave_the_output_untouched(ops):
    B, F, T, Wcap = 3, 5, 37, 8
    src = torch.randn(B, F, T, device="cuda")
    for row, start, length in [([0, 3], [0, 0], [4, 4]), ([0, -1], [0, 0], [4, 4]), ([0, 1], [0, -1], [4, 4]), ([0, 1], [0, 0], [4, 0]),
                               ([0, 1], [0, 34], [4, 4]), ([0, 1], [0, 0], [4, 9])]:
        out = nan_like(2, F, Wcap)
        with pytest.raises(RuntimeError, match=r"spk_window_gather failed \(rc=-1\)"):
            ops.window_gather(src, np.array(row), np.array(start), np.array(length), Wcap, out=out)
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    with pytest.raises(TypeError):
        ops.window_gather(src, np.array([0.0]), np.array([0]), np.array([4]), Wcap)


# ---- spk_window_mean --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 256, 257])
def test_mean_within_the_fp32_bound(ops, D):
    segs = [1, 2, 7, 300, 1, 7]
    seg_off = np.concatenate([[0], np.cumsum(segs)])
    N = int(seg_off[-1])
    rng = np.random.RandomState(D)
    weight = (np.arange(N) % 300 + 1).astype(np.float32)                   # 1 .. 300: window lengths, exact in fp32
    emb = (rng.randn(N, D) * 10.0 ** rng.uniform(-3, 3, size=(N, 1)) * 10.0 ** rng.uniform(-1, 1, size=(N, D))).astype(np.float32)
    got = ops.window_mean(torch.from_numpy(emb).cuda(), seg_off, weight).cpu().numpy().astype(np.float64)
    want, bound = R.mean_ref(emb, seg_off, weight)
    assert got.shape == want.shape == (len(segs), D)
    ratio = np.abs(got - want) / bound
    print("window_mean D %d: worst error / bound %.3f" % (D, ratio.max()))
    assert (ratio <= 1.0).all()
    assert (emb > 0).any() and (emb < 0).any()
    for u in (0, 4):                   # a one-row segment: one rounding of w e, the rounded reciprocal, one rounding of the product
        r = int(seg_off[u])
        w, e = weight[r], emb[r]
        assert np.array_equal(got[u].astype(np.float32), (w * e).astype(np.float32) * (np.float32(1.0) / w))
        assert (np.abs(got[u] - e.astype(np.float64)) <= 3 * 2.0 ** -24 * np.abs(e)).all()


def test_mean_is_deterministic_and_refuses_an_empty_segment(ops):
    emb = torch.randn(12, 64, device="cuda")
    w = np.arange(1, 13, dtype=np.float32)
    a = ops.window_mean(emb, [0, 5, 12], w)
    b = ops.window_mean(emb, np.array([0, 5, 12]), torch.from_numpy(w).cuda())
    assert torch.equal(a, b)
    for bad in ([0, 5, 5, 12], [0, 5, 11], [1, 5, 12]):
        with pytest.raises(RuntimeError, match=r"spk_window_mean failed \(rc=-1\)"):
            ops.window_mean(emb, bad, w)


# ---- predict_windows ---------------------------------------------------------------------------------------------------------------
LENGTHS = (104, 61, 5)
RUNS = [(24, 8, 1), (24, 24, 10)]


@pytest.fixture(scope="module")
def r18():
    """the r18_s21 model of tests/half_ref.py, its input with NaN past each utterance's length, and both runs of predict_windows"""
    case = H.CASES["r18_s21"]
    m, npst = make_model(case)
    x = torch.from_numpy(H.case_input(case)).clone()
    assert tuple(x.shape) == (3, 40, 104)
    for b, l in enumerate(LENGTHS):
        x[b, :, l:] = float("nan")               # never read: no window reaches past its utterance
    xg = x.cuda()
    runs = {}
    with torch.no_grad():
        for W, P, M in RUNS:
            emb, utt, start, length = m.predict_windows(xg, list(LENGTHS), W, P, M)
            runs[(W, P, M)] = (emb.cpu(), utt, start, length, m.engine().windows_skipped.tolist())
    return {"m": m, "npst": npst, "x": x, "xg": xg, "runs": runs, "case": case}


def same_as_alone(row, solo):
    """test_masked_predict_gpu's bar for a padded row against the row run alone; NaN where the solo run is NaN (one pooled frame)"""
    row, solo = row.numpy(), solo.numpy()
    if np.isnan(solo).any():
        return np.array_equal(np.isnan(row), np.isnan(solo))
    return bool(np.isfinite(row).all()) and close(row, solo)


@pytest.mark.parametrize("rule", RUNS)
def test_predict_windows_rows_are_the_windows_run_alone(r18, rule):
    W, P, M = rule
    emb, utt, start, length, skipped = r18["runs"][rule]
    want = R.brute_plan(LENGTHS, W, P, M)
    assert (utt.tolist(), start.tolist(), length.tolist(), skipped) == want
    assert skipped == ([2] if M == 10 else [])                    # the utterance of 5 frames
    assert emb.shape == (len(want[0]), 256) and emb.dtype == torch.float32
    m, xg = r18["m"], r18["xg"]
    with torch.no_grad():
        for i, (b, s, l) in enumerate(zip(utt, start, length)):
            solo = m.predict(xg[b:b + 1, :, s:s + l].contiguous()).cpu()
            assert same_as_alone(emb[i:i + 1], solo), (rule, i, b, s, l)
    finite = torch.isfinite(emb).all(dim=1).numpy()
    assert finite[length > 8].all() and finite.sum() >= len(finite) - 1


@pytest.mark.parametrize("rule", RUNS)
def test_average_is_the_weighted_mean_of_the_rows(r18, rule):
    W, P, M = rule
    emb, utt, start, length, skipped = r18["runs"][rule]
    with torch.no_grad():
        avg, uu = r18["m"].predict_windows(r18["xg"], torch.tensor(LENGTHS), W, P, M, average=True)
    uniq, first = np.unique(utt, return_index=True)
    assert uu.tolist() == uniq.tolist() == [u for u in range(3) if u not in skipped]
    want, bound = R.mean_ref(emb.numpy(), np.append(first, len(utt)), length)
    got = avg.cpu().numpy().astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and not nan[:2].any()
    assert (np.abs(got - want)[~nan] <= bound[~nan]).all()


def test_one_window_per_utterance_is_the_masked_predict(r18):
    m, xg = r18["m"], r18["xg"]
    with torch.no_grad():
        avg, uu = m.predict_windows(xg, list(LENGTHS), 128, 128, 1, average=True)
        emb, utt, start, length = m.predict_windows(xg, list(LENGTHS), 104, 7, 1)
        ref = m.predict(xg, lengths=list(LENGTHS)).cpu()
    assert uu.tolist() == utt.tolist() == [0, 1, 2] and start.tolist() == [0, 0, 0] and length.tolist() == list(LENGTHS)
    for b in range(3):
        assert same_as_alone(avg[b:b + 1].cpu(), ref[b:b + 1]), b
        assert same_as_alone(emb[b:b + 1].cpu(), ref[b:b + 1]), b


def test_predict_windows_arguments(r18):
    m, xg = r18["m"], r18["xg"]
    with torch.no_grad():
        for kw in (dict(window=0, period=1), dict(window=8, period=0), dict(window=8, period=8, min_window=9)):
            with pytest.raises(ValueError):
                m.predict_windows(xg, list(LENGTHS), **kw)
        with pytest.raises(ValueError):
            m.predict_windows(xg, [104, 105, 5], 24, 8)
        with pytest.raises(TypeError):
            m.predict_windows(xg, torch.tensor([104.0, 61.0, 5.0]), 24, 8)
        with pytest.raises(ValueError, match="precision"):
            m.predict_windows(xg, list(LENGTHS), 24, 8, precision="bf16")
        m.train()
        try:
            with pytest.raises(RuntimeError, match="eval"):
                m.predict_windows(xg, list(LENGTHS), 24, 8)
        finally:
            m.eval()
        # lengths=None: T frames each; every utterance skipped: empty results
        emb, utt, start, length = m.predict_windows(xg[:, :, :61].contiguous(), None, 61, 61)
        assert emb.shape == (3, 256) and length.tolist() == [61, 61, 61]
        emb, utt = m.predict_windows(xg, [5, 3, 0], 24, 24, 10, average=True)
        assert emb.shape == (0, 256) and utt.size == 0 and m.engine().windows_skipped.tolist() == [0, 1, 2]


# ---- precision="f16" ---------------------------------------------------------------------------------------------------------------
def test_half_rows_within_the_half_bar(r18):
    """tests/test_half_gpu.py's bar, row by row: the distance to the exact fp64 embedding of the window within 2 x the distance of
    the CPU emulation of the half contract (its factor, test_distance_to_the_exact_embedding / test_lengths)"""
    m, x, npst, case = r18["m"], r18["x"], r18["npst"], r18["case"]
    W, P, M = RUNS[1]
    with torch.no_grad():
        emb, utt, start, length = m.predict_windows(r18["xg"], list(LENGTHS), W, P, M, precision="f16")
    ovf = m.engine().half_overflow
    assert ovf.dtype == torch.int32 and ovf.cpu().tolist() == [0] * len(utt)
    assert (utt.tolist(), start.tolist(), length.tolist()) == R.brute_plan(LENGTHS, W, P, M)[:3]
    emb = emb.cpu()
    for i, (b, s, l) in enumerate(zip(utt, start, length)):
        xb = x[b:b + 1, :, s:s + l].numpy()
        e64, _, _ = H.embed(npst, xb, case[0], case[5], half=False)
        emu, _, _ = H.embed(npst, xb, case[0], case[5], half=True)
        rel_e, cos_e = H.distance(emu, e64)
        rel, cosd = H.distance(emb[i:i + 1], e64)
        print("window %d (utt %d, %d+%d): half vs fp64 %.3e %.3e; emulation %.3e %.3e" % (i, b, s, l, rel, cosd, rel_e, cos_e))
        assert rel <= 2.0 * rel_e and cosd <= 2.0 * cos_e, (i, b, s, l)


def test_half_overflow_is_reported_per_window():
    case = H.SCALED_CASE
    m, _ = make_model(case)
    x = torch.from_numpy(H.case_input(case, 12))
    xs = x.clone()
    xs[1] *= 1e4
    W, P = 48, 28                                  # three windows per utterance of 104 frames
    with torch.no_grad():
        # nine windows in one batch: the scaled utterance's rows sit between the others'
        e, utt, start, length = m.predict_windows(xs.cuda(), None, W, P, precision="f16", batch_size=9)
        ovf = m.engine().half_overflow.cpu()
        base, _, _, _ = m.predict_windows(x.cuda(), None, W, P, precision="f16", batch_size=9)
        ovf0 = m.engine().half_overflow.cpu()
        rest, utt2, _, _ = m.predict_windows(xs[[0, 2]].cuda(), None, W, P, precision="f16", batch_size=9)
        ovf2 = m.engine().half_overflow.cpu()
        avg, uu = m.predict_windows(xs.cuda(), None, W, P, average=True, precision="f16", batch_size=9)
        ovf_avg = m.engine().half_overflow.cpu()
    assert utt.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and start.tolist() == [0, 28, 56] * 3 and length.tolist() == [48] * 9
    assert ovf0.tolist() == [0] * 9 and ovf2.tolist() == [0] * 6 and utt2.tolist() == [0, 0, 0, 1, 1, 1]
    assert ((ovf > 0).numpy() == (utt == 1)).all(), ovf.tolist()            # exactly the windows of the scaled utterance
    assert torch.equal(ovf_avg, ovf) and uu.tolist() == [0, 1, 2]           # per window, also when the rows are averaged
    others = torch.from_numpy(utt != 1)
    assert torch.equal(e.cpu()[others], base.cpu()[others])                 # the same batch with the row unscaled
    assert torch.equal(e.cpu()[others], rest.cpu())                         # a run without that row


# ---- decode.py --window ------------------------------------------------------------------------------------------------------------
LENS = [30, 120, 44, 37, 88, 61, 104, 75]
NAMES = ["utt%03d" % i for i in range(len(LENS))]
SHORT = ["utt000", "utt003"]                         # fewer than 40 frames


@pytest.fixture(scope="module")
def decode_case(tmp_path_factory):
    """an 8-utterance archive, the r18_s21 checkpoint, and what predict_windows gives for the two runs"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import kaldi_io
    d = tmp_path_factory.mktemp("decode_windows")
    case = H.CASES["r18_s21"]
    Fd = case[2]
    rng = np.random.RandomState(11)
    feats = [rng.randn(n, Fd).astype(np.float32) for n in LENS]
    ark, scp = str(d / "feats.ark"), str(d / "feats.scp")
    with open(ark, "wb") as f, open(scp, "w") as s:
        for key, mat in zip(NAMES, feats):
            f.write(key.encode() + b" ")
            off = f.tell()
            kaldi_io.write_mat(f, mat)
            s.write("%s %s:%d\n" % (key, ark, off))
    m, npst = make_model(case)
    ckpt = str(d / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    x = torch.zeros(len(LENS), Fd, max(LENS))
    for b, mat in enumerate(feats):
        x[b, :, :LENS[b]] = torch.from_numpy(mat.T)
    with torch.no_grad():
        emb, utt, start, length = m.predict_windows(x.cuda(), LENS, 24, 12)
        avg, uu = m.predict_windows(x.cuda(), LENS, 48, 48, 40, average=True)
    assert (utt.tolist(), start.tolist(), length.tolist()) == R.brute_plan(LENS, 24, 12, 1)[:3]
    keys = ["%s-%08d-%08d" % (NAMES[b], s, s + l) for b, s, l in zip(utt, start, length)]
    segments = ["%s %s %.3f %.3f" % (k, NAMES[b], s * 0.01, (s + l) * 0.01) for k, b, s, l in zip(keys, utt, start, length)]
    assert [NAMES[b] for b in uu] == [n for n in NAMES if n not in SHORT]
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def decode(tag, fmt, *flags):
        out = str(d / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(H.SPK_NUM), "--arch", case[0],
               "--input-dim", str(Fd), "--pooling", case[5], "--model-path", ckpt, "--decode-scp", scp, "--out-path", out,
               "--native-reader", "--pad-batches", "--batch-size", "16", "--out-format", fmt] + list(flags)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return out, r

    return {"decode": decode, "emb": emb.cpu().numpy(), "avg": avg.cpu().numpy(), "keys": keys, "segments": segments,
            "avg_names": [NAMES[b] for b in uu], "case": case, "npst": npst, "x": x, "plan": (utt, start, length)}


@pytest.mark.parametrize("fmt", ["text", "fv"])
def test_decode_one_vector_per_window(decode_case, fmt):
    c = decode_case
    out, r = c["decode"]("win_" + fmt, fmt, "--window", "24", "--period", "12")
    got = _read_vectors(os.path.join(out, "alone"), fmt)
    assert len(got) == len(c["keys"]) and sorted(got) == sorted(c["keys"])
    for i, k in enumerate(c["keys"]):
        assert close(got[k][None], c["emb"][i:i + 1]), (fmt, k)
    assert sorted(open(os.path.join(out, "segments.alone")).read().splitlines()) == sorted(c["segments"])
    assert "=> 0 of 8 utterances shorter than --min-window were skipped" in r.stdout


@pytest.mark.parametrize("fmt", ["text", "fv"])
def test_decode_average_windows(decode_case, fmt):
    c = decode_case
    out, r = c["decode"]("avg_" + fmt, fmt, "--window", "48", "--average-windows", "--min-window", "40")
    got = _read_vectors(os.path.join(out, "alone"), fmt)
    assert sorted(got) == c["avg_names"]                                 # one line per utterance that has a window
    for i, name in enumerate(c["avg_names"]):
        assert close(got[name][None], c["avg"][i:i + 1]), (fmt, name)
    assert not os.path.exists(os.path.join(out, "segments.alone"))
    for name in NAMES:
        assert (("=> skipping %s:" % name) in r.stderr) == (name in SHORT)
    assert "=> 2 of 8 utterances shorter than --min-window were skipped" in r.stdout


def test_decode_windows_half(decode_case):
    c = decode_case
    out, r = c["decode"]("half", "text", "--window", "24", "--period", "12", "--half")
    assert "=> 0 of %d windows left the fp16 range and were extracted in fp32" % len(c["keys"]) in r.stdout
    got = _read_vectors(os.path.join(out, "alone"), "text")
    assert sorted(got) == sorted(c["keys"])
    # the bar of test_half_rows_within_the_half_bar, window by window: the distance to the exact fp64 embedding of the window
    # within twice the distance of the CPU emulation of the half contract on that same window
    case, x = c["case"], c["x"]
    for k, b, s, l in zip(c["keys"], *c["plan"]):
        xb = x[b:b + 1, :, s:s + l].numpy()
        e64, _, _ = H.embed(c["npst"], xb, case[0], case[5], half=False)
        emu, _, _ = H.embed(c["npst"], xb, case[0], case[5], half=True)
        rel_e, cos_e = H.distance(emu, e64)
        rel, cosd = H.distance(torch.from_numpy(got[k][None]), e64)
        assert rel <= 2.0 * rel_e and cosd <= 2.0 * cos_e, (k, rel, cosd, rel_e, cos_e)


# ---- decode.py --wav-scp --window ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wav_case(tmp_path_factory):
    """six short WAV files (one of them silent) and the r18_s21 checkpoint; decode(tag, *flags) -> (vectors by key, stdout, dir)"""
    from test_frontend_gpu import FB, _write_wavs
    d = tmp_path_factory.mktemp("decode_wav_windows")
    scp = _write_wavs(str(d), n=6, seed=3)
    case = H.CASES["r18_s21"]
    m, _ = make_model(case)
    ckpt = str(d / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def decode(tag, *flags):
        out = str(d / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(H.SPK_NUM), "--arch", case[0],
               "--input-dim", str(case[2]), "--pooling", case[5], "--model-path", ckpt, "--wav-scp", scp, "--out-path", out,
               "--batch-size", "8", "--fbank-config", os.path.join(FB, "fbank.conf"), "--vad-config", os.path.join(FB, "vad.conf")]
        r = subprocess.run(cmd + list(flags), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return _read_vectors(os.path.join(out, "alone"), "text"), r.stdout, out

    return decode


def test_decode_wav_one_window_per_utterance_is_the_plain_extraction(wav_case):
    """a window longer than every utterance, averaged: one window per utterance with its length as weight, so the vector is the
    whole-utterance one up to the two roundings of the mean kernel - the bar of a padded row against the row run alone"""
    whole, out0, _ = wav_case("whole")
    avg, out1, d1 = wav_case("avg", "--window", "400", "--average-windows", "--min-window", "1")
    assert sorted(avg) == sorted(whole) == ["utt%02d" % i for i in range(6) if i != 5]
    assert "utt05" in out1 and "no voiced frames" in out1 and "=> 0 of 5 utterances shorter than --min-window were skipped" in out1
    for k in whole:
        assert close(avg[k][None], whole[k][None]), k
    assert not os.path.exists(os.path.join(d1, "segments.alone"))


def test_decode_wav_windows_follow_the_rule(wav_case):
    """the keys of every utterance are the window rule applied to its voiced frame count (the end of its last window: period <=
    window and min-window 1 cover every frame), and segments.alone restates them in seconds"""
    vec, out, d = wav_case("win", "--window", "48", "--period", "24", "--frame-shift", "0.02")
    by_utt = {}
    for k in vec:
        u, s, e = k.rsplit("-", 2)
        by_utt.setdefault(u, []).append((int(s), int(e)))
    assert sorted(by_utt) == ["utt%02d" % i for i in range(6) if i != 5]
    segments = sorted(open(os.path.join(d, "segments.alone")).read().splitlines())
    want = []
    for u, w in by_utt.items():
        w.sort()
        n = w[-1][1]
        assert 48 < n < 400
        assert [(s, s + l) for s, l in R.brute_windows(n, 48, 24, 1)] == w, u
        want += ["%s-%08d-%08d %s %.3f %.3f" % (u, s, e, u, s * 0.02, e * 0.02) for s, e in w]
    assert segments == sorted(want)
    assert np.isfinite(np.stack(list(vec.values()))).all()
