"""csrc/plda.hip on a real MI355X: each kernel through the C ABI at its edges against the fp64 references and derived per-element
bounds of tests/plda_ref.py, then the whole stage on the `hip` back end against the restatement.  Run with -s to see the largest
error / bound of every group."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

import plda_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [1, 15, 16, 17, 24, 200, 256, 512]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    return _ops


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def pitched(x, pad):
    """device copy of x [N][D] whose rows are `pad` elements apart more than D"""
    if not pad:
        return dev(x)
    wide = np.full((x.shape[0], x.shape[1] + pad), 1e30 if x.dtype == np.float64 else np.float32(1e30), dtype=x.dtype)
    wide[:, :x.shape[1]] = x
    return dev(wide)[:, :x.shape[1]]


def ratio(got, ref, bound):
    """largest |got - ref| / bound; an element with bound 0 must be exact"""
    err = np.abs(got - ref)
    assert not (err[bound == 0] > 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


# ---- scatter --------------------------------------------------------------------------------------------------------------------
def _scatter_case(ops, rng, N, D, use_mu, use_w, f64, pad):
    x = (rng.randn(N, D) * 2 + 1).astype(np.float64 if f64 else np.float32)
    mu = rng.randn(D) + 1 if use_mu else None
    w = np.abs(rng.randn(N)) + rng.randint(1, 9, N) if use_w else None
    xd = pitched(x, pad)
    C = ops.scatter_f64(xd, None if mu is None else dev(mu), None if w is None else dev(w))
    C2 = ops.scatter_f64(xd, None if mu is None else dev(mu), None if w is None else dev(w))
    got = C.cpu().numpy()
    assert np.array_equal(got, got.T), (N, D)                                   # mirrored: symmetric bit for bit
    assert torch.equal(C, C2), (N, D)                                           # fixed slab order: two runs, the same bits
    ref, bound = R.scatter(x, mu, w)
    return ratio(got, ref, bound)


@pytest.mark.parametrize("D", DIMS)
def test_scatter_sizes(ops, D):
    slab = ops.scatter_slab_rows(1)
    assert slab >= 64 and ops.scatter_slab_rows(3 * slab - 1) == slab          # the sizes below really are 2 and 3 slabs
    rng = np.random.RandomState(D)
    worst = 0.0
    for i, N in enumerate([1, 3, 4, 5, 63, 64, 65, slab + 1, 3 * slab - 1]):
        k = i + D
        worst = max(worst, _scatter_case(ops, rng, N, D, k & 1, (k >> 1) & 1, (k >> 2) & 1, 3 if i % 2 else 0))
    print("scatter D=%d: largest |C - ref| / bound = %.3f" % (D, worst))
    assert worst <= 1.0


def test_scatter_every_option(ops):
    rng = np.random.RandomState(5)
    worst = max(_scatter_case(ops, rng, N, D, m, w, f, pad) for N, D in ((65, 24), (1025, 70)) for m in (0, 1) for w in (0, 1)
                for f in (0, 1) for pad in (0, 5))
    print("scatter options: largest |C - ref| / bound = %.3f" % worst)
    assert worst <= 1.0


def test_scatter_places_every_element(ops):
    """exact integer data, one row: C = x x^T has a different value at every (a, b) with a <= b, so a misplaced fragment shows"""
    for D in (17, 130):
        x = (np.arange(D, dtype=np.float64) * 3 + 1)[None, :]
        got = ops.scatter_f64(dev(x)).cpu().numpy()
        assert np.array_equal(got, x.T @ x)
    with pytest.raises(ValueError):
        ops.scatter_f64(torch.zeros(2, 513, device="cuda"))


# ---- class sums -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DIMS)
def test_segment_sum(ops, D):
    rng = np.random.RandomState(100 + D)
    worst = 0.0
    for case, (N, sizes) in enumerate([(7, [7]), (5, [1, 1, 1, 1, 1]), (40, [3, 1, 20, 16]), (300, [299, 1])]):
        x = rng.randn(N, D).astype(np.float32 if case % 2 else np.float64)
        seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        assert seg[-1] == N                                                      # the last class ends at N
        rows = rng.permutation(N).astype(np.int32) if case != 1 else None
        out, cnt = ops.segment_sum_f64(pitched(x, case), dev(seg), None if rows is None else dev(rows))
        ref, rc, bound = R.segment_sum(x, rows, seg)
        assert np.array_equal(cnt.cpu().numpy(), rc)
        worst = max(worst, ratio(out.cpu().numpy(), ref, bound))
        mean = ops.segment_sum_f64(pitched(x, case), dev(seg), None if rows is None else dev(rows), mean=True)[0].cpu().numpy()
        worst = max(worst, ratio(mean, ref / rc[:, None], (bound + np.abs(ref) * R.U53) / rc[:, None]))
    print("segment sum D=%d: largest error / bound = %.3f" % (D, worst))
    assert worst <= 1.0


# ---- affine map + length normalisation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Do,Di", [(1, 1), (17, 15), (16, 24), (200, 256)])
def test_affine_lennorm(ops, Do, Di):
    rng = np.random.RandomState(Do * 1000 + Di)
    A = rng.randn(Do, Di) / np.sqrt(Di)
    A[Do // 2, Di // 3] += 2.0                                                   # nothing symmetric about it
    b = rng.randn(Do)
    worst64, worst32 = 0.0, 0.0
    for N in (1, 63, 65):
        for variant in range(4):
            f64_in, use_q = variant & 1, variant >> 1
            x = (rng.randn(N, Di) * 3).astype(np.float64 if f64_in else np.float32)
            q = np.abs(rng.randn(Do)) + 0.1 if use_q else None
            xd = pitched(x, variant)
            for scale in (False, True):
                ref, bound = R.affine(x, A, b, q, scale)
                y64 = ops.affine_lennorm(xd, dev(A), dev(b), None if q is None else dev(q), scale, torch.float64).cpu().numpy()
                worst64 = max(worst64, ratio(y64, ref, bound))
                y32 = ops.affine_lennorm(xd, dev(A), dev(b), None if q is None else dev(q), scale, torch.float32).cpu().numpy()
                assert y32.dtype == np.float32
                r32 = ref.astype(np.float32)
                ulp = np.spacing(np.abs(r32)).astype(np.float64)
                worst32 = max(worst32, float((np.abs(y32.astype(np.float64) - r32.astype(np.float64)) / ulp).max()))
                if scale:                                                        # the weighted length really is sqrt(Do)
                    ss = (y64 * y64 * (1.0 if q is None else q)).sum(axis=1)
                    assert np.abs(ss / Do - 1).max() < 1e-12
    print("affine (%d, %d): fp64 largest error / bound = %.3f; fp32 largest error = %.2f ulp" % (Do, Di, worst64, worst32))
    assert worst64 <= 1.0 and worst32 <= 1.0


def test_affine_zero_row_identity_and_offsets(ops):
    rng = np.random.RandomState(9)
    A, x = rng.randn(17, 15), rng.randn(40, 15).astype(np.float32)
    x[[0, 33, 39]] = 0
    for out in (torch.float32, torch.float64):
        y = ops.affine_lennorm(dev(x), dev(A), None, None, True, out).cpu().numpy()
        assert not y[[0, 33, 39]].any() and np.isfinite(y).all()                 # a zero row stays zero, never NaN
        assert np.abs(np.linalg.norm(y[1].astype(np.float64)) - np.sqrt(17)) < 1e-5
    # A = NULL is the identity: ivector-normalize-length of float32 rows, and a plain copy without the scale
    v = (rng.randn(65, 200) * 2).astype(np.float32)
    v[7] = 0
    z = ops.affine_lennorm(dev(v), None, None, None, True, torch.float32).cpu().numpy()
    ref, _ = R.affine(v, None, None, None, True)
    r32 = ref.astype(np.float32)
    assert (np.abs(z.astype(np.float64) - r32) <= np.spacing(np.abs(r32))).all() and not z[7].any()
    assert np.array_equal(ops.affine_lennorm(dev(v), None, None, None, False, torch.float64).cpu().numpy(), v.astype(np.float64))
    # exact integer data with an asymmetric A: every output element lands in its place
    Ai = (np.arange(40 * 33).reshape(40, 33) % 17 - 8).astype(np.float64)
    xi = (np.arange(70 * 33).reshape(70, 33) % 13 - 6).astype(np.float64)
    got = ops.affine_lennorm(dev(xi), dev(Ai), dev(np.arange(40.0)), None, False, torch.float64).cpu().numpy()
    assert np.array_equal(got, xi @ Ai.T + np.arange(40.0))
    # writing into a row range of a larger table
    table = torch.zeros(100, 40, device="cuda", dtype=torch.float64)
    ops.affine_lennorm(dev(xi), dev(Ai), None, None, False, torch.float64, out=table[10:80])
    assert np.array_equal(table.cpu().numpy()[10:80], xi @ Ai.T) and not table[:10].any() and not table[80:].any()


def test_posterior_rows(ops):
    rng = np.random.RandomState(3)
    K, D = 37, 16
    mt, n, psi = rng.randn(K, D), rng.randint(1, 9, K).astype(np.int32), np.abs(rng.randn(D)) * 5
    psi[3] = 0
    w, r = ops.plda_posterior_rows(dev(mt), dev(n), dev(psi))
    g = n[:, None] * psi[None, :] / (n[:, None] * psi[None, :] + 1.0)
    assert np.allclose(w.cpu().numpy(), g * mt, rtol=4 * R.U53 * 2, atol=0)
    assert np.array_equal(r.cpu().numpy(), mt - w.cpu().numpy()) and not w.cpu().numpy()[:, 3].any()


# ---- trial scores ---------------------------------------------------------------------------------------------------------------
def _llr_tables(psi, counts):
    distinct = np.unique(counts)
    logs = np.array([[np.log(1.0 + psi / (c * psi + 1.0)).sum(), np.log(psi + 1.0).sum()] for c in distinct])
    return dev(distinct, np.int32), dev(logs)


@pytest.mark.parametrize("D", [1, 16, 200])
def test_plda_llr(ops, D):
    rng = np.random.RandomState(7 + D)
    n_en, n_te = 23, 31
    en, te = rng.randn(n_en, D) * 2, rng.randn(n_te, D) * 2
    psi = np.abs(rng.randn(D)) * 20
    if D > 1:
        psi[::5] = 0
    worst = 0.0
    for T in (1, 64, 65, 1000):
        ia, ib = rng.randint(0, n_en, T).astype(np.int32), rng.randint(0, n_te, T).astype(np.int32)
        ia[0], ib[0] = 0, 0
        ia[-1], ib[-1] = n_en - 1, n_te - 1                                      # first and last rows of both tables
        for counts in (None, np.where(np.arange(n_en) % 2, 3, 1).astype(np.int32)):
            tc, tl = _llr_tables(psi, np.array([1]) if counts is None else counts)
            got = ops.plda_llr(dev(en), dev(te), dev(ia), dev(ib), dev(psi), None if counts is None else dev(counts), tc, tl)
            ref, bound = R.llr_table(en, te, ia, ib, psi, counts)
            assert got.dtype == torch.float32
            worst = max(worst, ratio(got.cpu().numpy().astype(np.float64), ref, bound))
        # both sides from one table, the same row on both sides
        tc, tl = _llr_tables(psi, np.array([1]))
        got = ops.plda_llr(dev(en), dev(en), dev(ia), dev(ia), dev(psi), None, tc, tl)
        ref, bound = R.llr_table(en, en, ia, ia, psi)
        worst = max(worst, ratio(got.cpu().numpy().astype(np.float64), ref, bound))
    print("llr D=%d: largest error / bound = %.3f" % (D, worst))
    assert worst <= 1.0


def test_plda_llr_zero_psi_contributes_exactly_nothing(ops):
    rng = np.random.RandomState(1)
    for D in (1, 16, 70):
        en, te, psi = rng.randn(5, D) * 1e3, rng.randn(5, D) * 1e3, np.zeros(D)
        ia = np.arange(5, dtype=np.int32)
        counts = np.array([1, 3, 1, 3, 2], dtype=np.int32)
        tc, tl = _llr_tables(psi, counts)
        got = ops.plda_llr(dev(en), dev(te), dev(ia), dev(ia[::-1]), dev(psi), dev(counts), tc, tl).cpu().numpy()
        assert np.array_equal(got, np.zeros(5, dtype=np.float32))
    # a count the table does not hold cannot be scored: NaN, not a number that looks like a score
    tc, tl = _llr_tables(np.ones(4), np.array([1]))
    got = ops.plda_llr(dev(np.ones((1, 4))), dev(np.ones((1, 4))), dev(np.zeros(1, np.int32)), dev(np.zeros(1, np.int32)), dev(np.ones(4)),
                       dev(np.array([2], np.int32)), tc, tl).cpu().numpy()
    assert np.isnan(got).all()


# ---- the whole stage ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    S = R.synthetic()
    d = tmp_path_factory.mktemp("plda_gpu")
    R.write_text_ark(str(d / "train.iv"), S["train_keys"], S["train"])
    R.write_text_ark(str(d / "test.iv"), S["test_keys"], S["test"])
    (d / "mean.vec").write_text(" [ " + " ".join(map(str, S["mean"])) + " ]\n")
    (d / "utt2spk").write_text("".join("%s %s\n" % kv for kv in S["utt2spk"].items()))
    (d / "trials").write_text("".join("%s %s %s\n" % t for t in S["trials"]))
    return S, d, R.stage(S, True), R.stage(S, False)


def _pulled(lda, P):
    A = np.asarray(lda, dtype=np.float64)[:, :-1]
    psi, g1, g2 = R.invariants(P)
    return psi, A.T @ g1 @ A, A.T @ g2 @ A


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_whole_stage_on_hip_against_the_restatement(ops, stage):
    """The yardstick is the restatement's own sensitivity to the stage roundings, d = |rounded - all-fp64|; `hip` rounds the same
    stages in another summation order, so it must lie within 2 d of the all-fp64 restatement.  Measured on MI355X: see the printed
    ratios (DESIGN.md section 6j quotes them)."""
    from pytorch_kaldi_resnet_amd import plda, scoring
    S, d, r, f = stage
    tr, te = scoring.read_embeddings(str(d / "train.iv")), scoring.read_embeddings(str(d / "test.iv"))
    T, ev = plda.compute_lda(tr, S["utt2spk"], R.LDA_DIM, mean=S["mean"], backend="hip")
    P = plda.compute_plda(tr, S["utt2spk"], T, R.EM_ITERS, S["mean"], backend="hip")
    scores, labels = plda.plda_score(te, te, str(d / "trials"), S["mean"], T, P, backend="hip", score_path=str(d / "scores_hip"))
    assert _rel(ev[:R.LDA_DIM], r["lda_ev"][:R.LDA_DIM]) < 1e-10                 # fp64 from the same float32 x0
    got, rounded, full = _pulled(T, P), _pulled(r["lda"], r["plda"]), _pulled(f["lda"], f["plda"])
    d_psi = float((np.abs(rounded[0] - full[0]) / full[0]).max())
    e_psi = float((np.abs(got[0] - full[0]) / full[0]).max())
    print("psi: |hip - fp64| / d = %.3f (d = %.2e relative)" % (e_psi / d_psi, d_psi))
    assert e_psi <= 2 * d_psi
    for k, name in ((1, "T^T T"), (2, "T^T psi T")):
        dk = _rel(rounded[k], full[k])
        print("%s: |hip - fp64| / d = %.3f (d = %.2e)" % (name, _rel(got[k], full[k]) / dk, dk))
        assert _rel(got[k], full[k]) <= 2 * dk
    d_s = float(np.abs(r["scores"] - f["scores"]).max())
    e_s = float(np.abs(scores.astype(np.float64) - f["scores"]).max())
    print("scores: |hip - fp64| / d = %.3f (d = %.2e on %.1f ... %.1f)" % (e_s / d_s, d_s, f["scores"].min(), f["scores"].max()))
    assert scores.dtype == np.float32 and e_s <= 2 * d_s
    lab = [t[2] == "target" for t in S["trials"]]
    rep = scoring.score_and_report(te, te, str(d / "trials"), S["mean"], plda=P, transform=T, backend="hip")
    assert (rep["eer"], rep["min_dcf"][0][0], rep["min_dcf"][1][0]) == pytest.approx(R.error_rates(r["scores"], lab), abs=1e-15)
    # the estimator in the per-iteration basis is the class loop: the host back end on the same transform gives the same object
    Ph = plda.compute_plda(tr, S["utt2spk"], T, R.EM_ITERS, S["mean"], backend="host")
    assert _rel(P[2], Ph[2]) <= 2 * d_psi and _rel(P[1].T @ P[1], Ph[1].T @ Ph[1]) <= 2 * _rel(rounded[1], full[1])
    # the files of the two back ends: the same keys in the same order
    plda.plda_score(te, te, str(d / "trials"), S["mean"], T, P, backend="host", score_path=str(d / "scores_host"))
    keys = [[l.split()[:2] for l in open(str(d / n))] for n in ("scores_hip", "scores_host")]
    assert keys[0] == keys[1] == [list(t[:2]) for t in S["trials"]]


def test_scoring_options_on_hip(ops, stage):
    from pytorch_kaldi_resnet_amd import plda, scoring
    S, d, r, f = stage
    te = scoring.read_embeddings(str(d / "test.iv"))
    num = {k: (3 if i % 2 else 1) for i, k in enumerate(S["test_keys"])}
    args = (S["test_keys"], S["test"], S["test_keys"], S["test"], S["trials"], S["mean"], r["lda"], r["plda"])
    for kw, rkw in ((dict(num_utts=num), dict(num_utts=num)), (dict(simple_length_normalization=True), dict(simple=True)),
                    (dict(normalize_length=False), dict(normalize_length=False)), (dict(smoothing=0.1, num_utts=num), dict(smoothing=0.1, num_utts=num))):
        full = R.score(*args, rounded=False, **rkw)
        dd = float(np.abs(R.score(*args, rounded=True, **rkw) - full).max())
        got, _ = plda.plda_score(te, te, str(d / "trials"), S["mean"], r["lda"], r["plda"], backend="hip", **kw)
        e = float(np.abs(got.astype(np.float64) - full).max())
        print("%s: |hip - fp64| / d = %.3f" % (sorted(kw), e / dd))
        assert e <= 2 * dd


def test_scripts_on_hip(ops, stage, monkeypatch, capsys):
    from pytorch_kaldi_resnet_amd import plda
    S, d, r, f = stage
    monkeypatch.chdir(str(d))
    for argv in (["compute_lda.py", "--backend", "hip", "--dim", str(R.LDA_DIM), "--mean", "mean.vec", "train.iv", "utt2spk", "transform.mat"],
                 ["compute_plda.py", "--backend", "hip", "--mean", "mean.vec", "train.iv", "utt2spk", "transform.mat", "plda"],
                 ["plda_score.py", "--backend", "hip", "--mean", "mean.vec", "--transform", "transform.mat", "--plda", "plda", "--enroll",
                  "test.iv", "--test", "test.iv", "--trials", "trials", "--score-file", "scores_plda"]):
        monkeypatch.setattr(sys, "argv", argv)
        runpy.run_path(os.path.join(ROOT, "scripts", argv[0]), run_name="__main__")
    got = np.array([float(l.split()[2]) for l in open(str(d / "scores_plda"))])
    d_s = float(np.abs(r["scores"] - f["scores"]).max())
    assert float(np.abs(got - f["scores"]).max()) <= 2 * d_s
    assert plda.read_transform(str(d / "transform.mat")).shape == (R.LDA_DIM, R.D + 1) and len(plda.read_plda(str(d / "plda"))[2]) == R.LDA_DIM
