"""csrc/eval.hip on a real MI355X: speaker means, adaptive S-norm, the trial sort and the error-rate sweep, and the stage
functions and scripts on top of them.  Nothing here is approximate, so every comparison is exact (array_equal / ==): against
the fixtures the reference's programs wrote (tests/golden/backend) and against the restatements of tests/backend_ref.py."""
import os
import runpy
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import backend_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = R.GOLD


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scoring():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import scoring as _scoring
    return _scoring


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- sort -----------------------------------------------------------------------------------------------------------------
def _sort_sizes(tile):
    return [1, 2, 3, tile - 1, tile, tile + 1, 2 * tile + 1, 3 * tile + 17, 100003]


def _sort_input(kind, T, rng):
    if kind == "equal":
        return np.full(T, 0.25)
    if kind == "sorted":
        return np.arange(T, dtype=np.float64) * 0.5 - 7
    if kind == "reversed":
        return -(np.arange(T, dtype=np.float64) * 0.5 - 7)
    if kind == "ties":                                      # rounded to 0.5: heavy ties; zeros of both signs
        s = np.round(rng.randn(T) * 2) / 2
        z = np.flatnonzero(s == 0)
        s[z[::2]] = -0.0
        return s
    if kind == "extremes":                                  # +-inf, subnormals, the largest and smallest normal numbers
        pool = np.array([np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e-310, -1e-310,
                         1.7976931348623157e308, -1.7976931348623157e308, 0.0, -0.0, 1.0, -1.0])
        return pool[rng.randint(len(pool), size=T)]
    if kind == "negative":
        return -np.abs(rng.randn(T)) - 1e-3
    assert kind == "ulps"                                   # 1 + k 2^-52, shuffled: equal once a key is narrowed to fp32
    return 1.0 + rng.permutation(T) * 2.0 ** -52


@pytest.mark.parametrize("kind", ["equal", "sorted", "reversed", "ties", "extremes", "negative", "ulps"])
def test_sort_trials(ops, kind):
    tile = ops.sort_tile()
    assert tile >= 1024 and tile & (tile - 1) == 0
    rng = np.random.RandomState(3)
    for T in _sort_sizes(tile):
        s = _sort_input(kind, T, rng)
        got = ops.sort_trials(dev(s)).cpu().numpy()
        assert got.dtype == np.int32
        want = np.lexsort((np.arange(T), s + 0.0))
        assert np.array_equal(got, want), (kind, T)
        if kind == "equal":
            assert np.array_equal(got, np.arange(T))


def test_sort_trials_rejects_nan_and_empty(ops):
    with pytest.raises(ValueError, match="NaN"):
        ops.sort_trials(dev(np.array([0.5, np.nan, 1.0])))
    with pytest.raises(ValueError):
        ops.sort_trials(torch.empty(0, dtype=torch.float64, device="cuda"))
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    assert lib.spk_sort_trials_workspace(1) == tile_bytes(ops, ops.sort_tile())
    assert lib.spk_sort_trials_workspace(ops.sort_tile() + 1) == tile_bytes(ops, 2 * ops.sort_tile())
    assert lib.spk_sort_trials(None, None, None, 0, None) < 0 and b"spk_sort_trials" in lib.spk_last_error()


def tile_bytes(ops, n):
    return n * 12           # an 8-byte key and a 4-byte index per padded position


# ---- sweep ----------------------------------------------------------------------------------------------------------------
def _device_sweep(ops, s, lab, costs):
    sd = dev(np.asarray(s, dtype=np.float64))
    order = ops.sort_trials(sd)
    out_d, out_i = ops.error_sweep(sd, dev(np.asarray(lab, dtype=np.uint8)), order, costs)
    d, i = out_d.cpu().tolist(), out_i.cpu().tolist()
    return d[0], i[0], [(d[1 + 2 * k], d[2 + 2 * k], i[3 + k]) for k in range(len(costs))], i[1], i[2]


def test_error_sweep_equals_the_reference_doubles(ops):
    for s, lab, costs, exp in R.golden_sweep_cases():
        eer, at, dcf, n_tar, n_non = _device_sweep(ops, s, lab, costs)
        assert [eer] + [v for d, t, _ in dcf for v in (d, t)] == exp.tolist()
        ref = R.sweep(s, lab, costs)
        assert (eer, at, dcf) == ref
        assert (n_tar, n_non) == (int(lab.sum()), len(lab) - int(lab.sum()))


def test_error_sweep_thresholds_keep_the_sign_of_zero(ops):
    # -0.0 sorts as +0.0 but is reported as it was given
    s, lab = np.array([-0.0, 0.0, 1.0, -1.0]), np.array([1, 0, 1, 0])
    eer, at, dcf, _, _ = _device_sweep(ops, s, lab, [(0.5, 1.0, 1.0)])
    assert (eer, at, dcf) == R.sweep(s, lab, [(0.5, 1.0, 1.0)])
    assert [np.signbit(t) for _, t, _ in dcf] == [np.signbit(t) for _, t, _ in R.sweep(s, lab, [(0.5, 1.0, 1.0)])[2]]


def test_error_sweep_across_scan_blocks(ops):
    block = ops.sweep_block()
    costs = [(0.01, 1.0, 1.0), (0.001, 1.0, 1.0), (0.05, 10.0, 1.0)]
    rng = np.random.RandomState(4)
    for T in (block - 1, block, block + 1, 100003):
        for ties in (False, True):
            lab = (rng.rand(T) < 0.2).astype(np.uint8)
            s = rng.randn(T) + 2.0 * lab
            if ties:
                s = np.round(s * 4) / 4
            got = _device_sweep(ops, s, lab, costs)
            assert got[:3] == R.sweep(s, lab, costs), (T, ties)
            assert got[3] == int(lab.sum())
    # no cost triple at all: the EER alone
    assert _device_sweep(ops, s, lab, [])[:2] == R.sweep(s, lab, [])[:2]


def test_error_sweep_ties_and_separable_lists(ops):
    block = ops.sweep_block()
    T = 2 * block + 6
    lab = np.zeros(T, dtype=np.uint8)
    lab[T // 2:] = 1                                      # all non-targets below all targets: EER 0, cost 0 at one position
    s = np.arange(T, dtype=np.float64)
    got = _device_sweep(ops, s, lab, [(0.5, 1.0, 1.0)])
    assert got[:3] == R.sweep(s, lab, [(0.5, 1.0, 1.0)])
    assert got[0] == 0.0 and got[2][0][0] == 0.0 and got[2][0][2] == T // 2 - 1
    # alternating labels: the minimum cost is attained at many positions, in more than one scan block; the first is returned
    lab = np.tile(np.array([0, 1], dtype=np.uint8), T // 2)
    ref = R.sweep(s, lab, [(0.5, 1.0, 1.0), (0.5, 2.0, 2.0)])
    fn = np.cumsum(lab) / float(lab.sum())
    fp = 1 - np.cumsum(1 - lab) / float(T - lab.sum())
    c = 1.0 * fn * 0.5 + 1.0 * fp * 0.5
    assert int((c == c.min()).sum()) > 1 and np.flatnonzero(c == c.min())[-1] >= block          # ties in more than one block
    got = _device_sweep(ops, s, lab, [(0.5, 1.0, 1.0), (0.5, 2.0, 2.0)])
    assert got[:3] == ref and got[2][0][2] == int(np.flatnonzero(c == c.min())[0])
    # all targets below all non-targets: every threshold is wrong on one side, EER as the reference computes it (1.0)
    lab = np.zeros(T, dtype=np.uint8)
    lab[:5] = 1
    got = _device_sweep(ops, s, lab, [(0.01, 1.0, 1.0)])
    assert got[:3] == R.sweep(s, lab, [(0.01, 1.0, 1.0)]) and got[0] == 1.0


def test_error_rates_backends_agree_and_validate(scoring):
    rng = np.random.RandomState(6)
    lab = (rng.rand(5000) < 0.3).astype(np.int64)
    s = np.round((rng.randn(5000) + lab) * 8) / 8
    assert scoring.error_rates(s, lab, backend="hip") == scoring.error_rates(s, lab, backend="host")
    assert scoring.min_dcf(s, lab, 0.05, 10, 2, backend="hip") == scoring.min_dcf(s, lab, 0.05, 10, 2, backend="host")
    with pytest.raises(ValueError, match="NaN"):
        scoring.error_rates([0.1, float("nan")], [0, 1], backend="hip")
    with pytest.raises(ValueError, match="NaN"):
        scoring.error_rates(dev(np.array([0.1, np.nan])), [0, 1], backend="hip")
    with pytest.raises(ValueError):
        scoring.error_rates([0.1, 0.2], [1, 1], backend="hip")
    with pytest.raises(ValueError, match="--p-target"):
        scoring.min_dcf([0.1, 0.2], [0, 1], p_target=1.0, backend="hip")


# ---- speaker means --------------------------------------------------------------------------------------------------------
def test_segment_mean_reproduces_the_reference_file(scoring, tmp_path):
    out = str(tmp_path / "spk_mean.vec")
    scoring.speaker_mean(scoring.read_embeddings(os.path.join(GOLD, "train.iv")), os.path.join(GOLD, "utt2spk"), out, backend="hip")
    assert open(out).read() == open(os.path.join(GOLD, "spk_mean.vec")).read()


@pytest.mark.parametrize("S,D", [(1, 1), (3, 16), (257, 256), (3, 256), (257, 1)])
def test_segment_mean_bit_for_bit(ops, S, D):
    rng = np.random.RandomState(S * 1000 + D)
    counts = rng.randint(1, 6, size=S)
    counts[0] = 1                                          # a speaker with one utterance
    counts[-1] = 1000 if S > 1 else 7                      # and one with a thousand
    spk_of = rng.permutation(np.repeat(np.arange(S), counts))            # interleaved: the archive is not grouped by speaker
    N = len(spk_of)
    # float32 values of mixed magnitude widened to float64, plus float64 noise: the fp32 rounding after every addition shows
    emb = (rng.randn(N, D).astype(np.float32) * 10.0 ** rng.randint(-3, 4, size=(N, 1))).astype(np.float64) + 1e-9 * rng.randn(N, D)
    keys = ["u%d" % i for i in range(N)]
    ref = R.speaker_mean(keys, emb, {k: int(s) for k, s in zip(keys, spk_of)})
    first = list(dict.fromkeys(spk_of.tolist()))
    assert list(ref) == first
    rows = np.argsort(spk_of, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(spk_of, minlength=S))]).astype(np.int32)
    got = ops.segment_mean(dev(emb), dev(rows), dev(seg_off)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (S, D)
    for s in range(S):
        assert np.array_equal(got[s], ref[s]), s
    # the order inside a speaker is part of the result: reversing it changes bits somewhere (so the test can see a reordering)
    if S == 257 and D == 256:
        rev = np.concatenate([rows[seg_off[s]:seg_off[s + 1]][::-1] for s in range(S)]).astype(np.int32)
        assert not np.array_equal(ops.segment_mean(dev(emb), dev(rev), dev(seg_off)).cpu().numpy(), got)


# ---- adaptive S-norm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 255, 256, 257, 10001])
def test_trial_snorm_bit_for_bit(ops, T):
    rng = np.random.RandomState(T)
    ne, nt = 37, 41
    e_mean, t_mean = rng.randn(ne) * 0.1, rng.randn(nt) * 0.1
    e_std, t_std = np.abs(rng.randn(ne)) * 0.2 + 0.01, np.abs(rng.randn(nt)) * 0.2 + 0.01
    e_std[0] = 0.0                                          # max(std, 1e-8) takes the constant
    t_std[1] = 1e-9
    t_std[2] = 1e-8
    ia, ib = rng.randint(ne, size=T).astype(np.int32), rng.randint(nt, size=T).astype(np.int32)
    ia[0], ib[0] = 0, 1
    s32 = (rng.rand(T) * 2 - 1).astype(np.float32)
    ref = R.snorm(s32.tolist(), ia, ib, e_mean, e_std, t_mean, t_std)
    got = ops.trial_snorm(dev(s32), dev(ia), dev(ib), dev(e_mean), dev(e_std), dev(t_mean), dev(t_std)).cpu().numpy()
    assert np.array_equal(got, ref)
    s64 = rng.rand(T) * 2 - 1                                # what a score file holds: any double
    ref = R.snorm(s64.tolist(), ia, ib, e_mean, e_std, t_mean, t_std)
    got = ops.trial_snorm(dev(s64), dev(ia), dev(ib), dev(e_mean), dev(e_std), dev(t_mean), dev(t_std)).cpu().numpy()
    assert np.array_equal(got, ref)


# ---- stage ----------------------------------------------------------------------------------------------------------------
def _script(name, args, capsys):
    argv = sys.argv
    sys.argv = [name] + args
    try:
        runpy.run_path(os.path.join(ROOT, "scripts", name), run_name="__main__")
    finally:
        sys.argv = argv
    return capsys.readouterr().out


def test_scripts_write_the_same_bytes_from_both_backends(tmp_path, capsys):
    d = str(tmp_path)
    g = lambda f: os.path.join(GOLD, f)      # noqa: E731
    out = {}
    for be in ("host", "hip"):
        o = lambda f: os.path.join(d, be + "_" + f)      # noqa: E731
        out[be] = [
            _script("compute_speaker_mean.py", ["--backend", be, g("train.iv"), g("utt2spk"), o("spk_mean.vec")], capsys).replace(o(""), ""),
            _script("adaptive_snorm.py", ["--backend", be, "--enroll", g("topk_mean_std"), "--test", g("topk_mean_std"), "--score-in",
                                          g("scores"), "--score-out", o("scores_snorm")], capsys).replace(o(""), ""),
            _script("compute_eer.py", ["--backend", be, o("scores_snorm"), g("trials")], capsys),
            _script("compute_min_dcf.py", ["--backend", be, "--p-target", "0.001", o("scores_snorm"), g("trials")], capsys),
            _script("compute_min_dcf.py", ["--backend", be, "--p-target", "0.05", "--c-miss", "10", "--c-fa", "2", g("scores"), g("trials")],
                    capsys),
            open(o("spk_mean.vec")).read(), open(o("scores_snorm")).read()]
    assert out["hip"] == out["host"]
    assert out["hip"][5] == open(g("spk_mean.vec")).read() and out["hip"][6] == open(g("scores_snorm")).read()
    assert out["hip"][4] == open(g("min_dcf_0.05_10_2.stdout")).read()


def test_test_sh_report_on_the_device(tmp_path):
    """stage 13 of test.sh (EER and the two minDCFs, one process each) with SPK_SCORE_BACKEND=hip: the reference's report"""
    d = str(tmp_path)
    shutil.copy(os.path.join(GOLD, "scores_snorm"), os.path.join(d, "scores_snorm_adapt_snorm"))
    env = dict(os.environ, SPK_SCORE_BACKEND="hip")
    p = subprocess.run(["bash", os.path.join(ROOT, "test.sh"), d, d, "snorm", "13", os.path.join(GOLD, "trials")], cwd=d, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr
    assert open(os.path.join(d, "eer_snorm_adapt_snorm")).read() == open(os.path.join(GOLD, "eer_snorm_adapt_snorm")).read()


def test_score_and_report_on_the_device(scoring, tmp_path):
    from pytorch_kaldi_resnet_amd import kaldi_io
    emb = scoring.read_embeddings(os.path.join(GOLD, "test.iv"))
    mean = kaldi_io.read_vec_flt(os.path.join(GOLD, "mean.vec"))
    trials = os.path.join(GOLD, "trials")
    sc, lab = scoring.cosine_score(emb, emb, trials, mean, backend="hip")           # the device's own cosine scores
    assert scoring.score_and_report(emb, emb, trials, mean, backend="hip") == scoring.error_rates(sc.astype(np.float64), lab)
    stats = scoring.read_mean_std(os.path.join(GOLD, "topk_mean_std"))
    path = str(tmp_path / "scores")
    rep = scoring.score_and_report(emb, emb, trials, mean, stats, stats, backend="hip", score_path=path)
    names = list(stats)
    pairs = [l.split()[:2] for l in open(trials)]
    mu, sd = np.array([stats[k][0] for k in names]), np.array([stats[k][1] for k in names])
    sn = R.snorm(sc.tolist(), [names.index(a) for a, _ in pairs], [names.index(b) for _, b in pairs], mu, sd, mu, sd)
    assert rep == scoring.error_rates(sn, lab)
    assert np.array_equal(np.array([float(l.split()[2]) for l in open(path)]), sn)
