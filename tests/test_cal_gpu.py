"""Calibration and fusion of trial scores on the device (csrc/cal.hip): the `hip` back end against the host
back end and against the restatement in tests/cal_ref.py.  apply, the miss / false-alarm counts, the actDCF doubles, the pools and the
per-trial pool index are equal; Cllr, minCllr and the training are held to the bounds of section 6s.  The lists are the smallest at
which each kernel can go wrong (cal_ref.pav_cases).  With -s every test prints its largest error / bound."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cal_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "backend")
EPS = 1e-18
COSTS = [(0.01, 1, 1), (0.001, 1, 1), (0.5, 1, 1), (0.05, 10, 2)]


@pytest.fixture(scope="module")
def C():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import calibration
    return calibration


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


@pytest.fixture(scope="module")
def cases(ops):
    block, tile = ops.cal_sizes()[:2]
    return R.pav_cases(block, tile)


CASE_NAMES = R.PAV_CASE_NAMES


# ---- apply ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 8])
def test_apply_is_bit_equal_to_host(C, ops, K):
    import torch
    block, _, _, threads = ops.cal_sizes()
    rng = np.random.RandomState(K)
    for T in (1, 2, 3, 63, 64, 65, threads - 1, threads, threads + 1, block - 1, block, block + 1, 2 * block + 1):
        cols, th = rng.randn(K, T) * 5, rng.randn(K + 1)
        m = C.Model(th[:K], th[K])
        got = C.apply(m, cols, backend="hip")
        assert isinstance(got, np.ndarray) and np.array_equal(got, C.apply(m, cols)), (K, T)
        dev = C.apply(m, torch.from_numpy(cols).cuda(), backend="hip")
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    with pytest.raises(ValueError, match="NaN or infinite"):
        C.apply(m, torch.from_numpy(np.array([[0.0, np.inf]] * K)).cuda(), backend="hip")


# ---- Cllr, actDCF -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_cllr_and_counts(C, cases, name):
    """the scores of the case, shifted and scaled into the range where the thresholds lie, read as log-likelihood ratios"""
    s, lab = cases[name]
    llr = (s - np.median(s)) * (12.0 / max(np.ptp(s), 1.0))
    if name == "signed_zeros":
        llr = s
    host, dev = C.evaluate(llr, lab, COSTS), C.evaluate(llr, lab, COSTS, backend="hip")
    assert (dev["n_target"], dev["n_nontarget"]) == (host["n_target"], host["n_nontarget"])
    for h, d in zip(host["act_dcf"], dev["act_dcf"]):
        assert (d["miss"], d["fa"], d["threshold"]) == (h["miss"], h["fa"], h["threshold"]) and d["act_dcf"] == h["act_dcf"]
    ld = R.cllr_ld(llr, lab)
    err, bound = abs(dev["cllr"] - float(ld)), R.sum_bound(llr.size, ld)
    print("%s: T=%d Cllr %.6f error / bound %.3g" % (name, llr.size, dev["cllr"], err / bound))
    assert err <= bound
    assert abs(host["cllr"] - float(ld)) <= bound


def test_cllr_thresholds_on_a_score(C):
    """llr == eta is accepted; one value on every side of every threshold, in a block of its own and across a block edge"""
    eta = [C.bayes_threshold(*c) for c in COSTS]
    vals = np.array(sorted(eta + [np.nextafter(e, -np.inf) for e in eta] + [np.nextafter(e, np.inf) for e in eta]))
    llr = np.tile(vals, 200)
    lab = (np.arange(llr.size) // vals.size) % 2
    host, dev = C.evaluate(llr, lab, COSTS), C.evaluate(llr, lab, COSTS, backend="hip")
    for (p, cm, cf), h, d in zip(COSTS, host["act_dcf"], dev["act_dcf"]):
        want = R.act_dcf(llr.tolist(), lab.tolist(), p, cm, cf)
        assert (h["act_dcf"], h["miss"], h["fa"]) == want[:3] and (d["act_dcf"], d["miss"], d["fa"]) == want[:3]


# ---- pools ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_pools_and_min_cllr(C, ops, cases, name):
    s, lab = cases[name]
    hv, hp, hi, hd = C.min_cllr(s, lab, details=True)
    dv, dp, di, dd = C.min_cllr(s, lab, backend="hip", details=True)
    assert np.array_equal(dd["tie_pools"], hd["tie_pools"]) and dd["counts"][0] == hd["tie_pools"].shape[0]
    assert dp.dtype == np.int64 and np.array_equal(dp, hp) and np.array_equal(di, hi)
    assert dd["counts"][0] >= dd["counts"][1] >= dd["counts"][2] >= dd["counts"][3] == hp.shape[0]
    if hd["tie_pools"].shape[0] <= 120:
        tie, order = R.tie_pools(s.tolist(), lab.tolist())
        want = R.pav_minimax(tie)
        assert [tuple(p) for p in dp.tolist()] == want and di.tolist() == R.pool_index(want, order)
    n_tar = int(lab.sum())
    ld = R.min_cllr_ld(hp.tolist(), n_tar, lab.size - n_tar)
    bound = R.sum_bound(hp.shape[0], ld)
    print("%s: T=%d pools %s minCllr %.6f error / bound %.3g" % (name, s.size, dd["counts"], dv, abs(dv - float(ld)) / bound if bound else 0.0))
    assert abs(dv - float(ld)) <= bound and abs(hv - float(ld)) <= bound
    if name in ("separated", "separated_shuffled"):
        assert dv == 0.0 and dp.shape[0] == 2
    if name in ("reversed", "all_equal"):
        assert dp.shape[0] == 1 and abs(dv - 1.0) <= R.sum_bound(1, 1.0)
    if name == "more_final_pools_than_a_tile":
        assert dp.shape[0] > ops.cal_sizes()[1]


def test_pools_of_a_device_tensor_stay_on_the_device(C):
    import torch
    lab, llr = R.gaussian_llr(3, 500)
    v, pools, pool_of = C.min_cllr(torch.from_numpy(llr).cuda(), lab, backend="hip")
    hv, hp, hi = C.min_cllr(llr, lab)
    assert pool_of.is_cuda and np.array_equal(pool_of.cpu().numpy(), hi) and np.array_equal(pools, hp)
    with pytest.raises(ValueError, match="NaN or infinite"):
        C.min_cllr(torch.from_numpy(np.array([0.0, np.nan, 1.0])).cuda(), np.array([0, 1, 1]), backend="hip")


# ---- training --------------------------------------------------------------------------------------------------------------------------
def train_case(C, T, K):
    if T == 66:
        pairs, cols = C.read_score_files([os.path.join(GOLD, "scores"), os.path.join(GOLD, "scores_snorm")])
        lab = C.trial_labels(pairs, os.path.join(GOLD, "trials"))
        third = np.cos(np.arange(66.0))                                  # any per-trial number may be a column
        return lab, np.ascontiguousarray([cols[0], cols[1], third][:K]), 0.01, 0.0
    lab, cols = R.train_columns(7, T, K)
    return lab, cols, 0.2, 1e-6


@pytest.mark.parametrize("T", [66, 300, 4097])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_training(C, ops, T, K):
    import torch
    lab, cols, p, l2 = train_case(C, T, K)
    n_tar = int(lab.sum())
    cd, ld = torch.from_numpy(cols).cuda(), torch.from_numpy(lab).cuda()
    worst = 0.0
    # one evaluation at a fixed theta: the state holds f, g, H at the last accepted theta - zero, two steps on, the result
    for iters in (1, 3, 100):
        state, istate = ops.cal_train(cd, ld, n_tar, p, C.logit(p), l2, EPS, iters)
        st, ist = state.cpu().numpy(), istate.cpu().tolist()
        theta = st[9:9 + K + 1]
        o = R.objective_ld(cols, lab, theta, p, l2)
        b = lambda a: R.eval_bound(T, K, o["A"], a)                      # noqa: E731
        assert abs(st[27] - float(o["f"])) <= b(o["f_abs"])
        worst = max(worst, abs(st[27] - float(o["f"])) / b(o["f_abs"]))
        for j in range(K + 1):
            assert abs(st[30 + j] - float(o["g"][j])) <= b(o["g_abs"][j]), (iters, j)
            worst = max(worst, abs(st[30 + j] - float(o["g"][j])) / b(o["g_abs"][j]))
            for k in range(j + 1):
                e = abs(st[40 + j * (j + 1) // 2 + k] - float(o["H"][j, k]))
                assert e <= b(o["H_abs"][j, k]), (iters, j, k)
                worst = max(worst, e / b(o["H_abs"][j, k]))
        if iters == 1:
            assert not theta.any() and ist[:2] == [2, 1]
    # the returned theta
    host = C.train(cols, lab, p, l2)
    dev = C.train(cd, lab, p, l2, backend="hip")
    assert host.status == "converged" and dev.status == "converged" and dev.evaluations <= 20 and host.evaluations <= 20
    o = R.objective_ld(cols, lab, dev.theta, p, l2)
    for j in range(K + 1):
        assert abs(float(o["g"][j])) <= 2 * math.sqrt(EPS * float(o["H"][j, j])) + R.eval_bound(T, K, o["A"], o["g_abs"][j]), j
    oh = R.objective_ld(cols, lab, host.theta, p, l2)
    gap = abs(float(o["f"] - oh["f"]))
    assert gap <= 4 * EPS + 2 * R.eval_bound(T, K, max(o["A"], oh["A"]), max(o["f_abs"], oh["f_abs"]))
    print("T=%d K=%d: %d evaluations (host %d), f(hip) - f(host) = %.3g, largest evaluation error / bound %.3g, theta %s" % (
        T, K, dev.evaluations, host.evaluations, gap, worst, dev.theta.tolist()))
    # the same bits again, and when the call follows another on the stream
    again = C.train(cols, lab, p, l2, backend="hip")
    assert (again.weights, again.bias, again.status, again.evaluations, again.objective) == (
        dev.weights, dev.bias, dev.status, dev.evaluations, dev.objective)
    torch.cuda.synchronize()
    s1 = ops.cal_train(cd, ld, n_tar, p, C.logit(p), l2, EPS, 100)
    s2 = ops.cal_train(cd, ld, n_tar, p, C.logit(p), l2, EPS, 100)       # enqueued behind the first, nothing waited for
    torch.cuda.synchronize()
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]) and s1[0].cpu().numpy()[9:9 + K + 1].tolist() == dev.theta.tolist()


def test_training_at_eight_systems(C):
    lab, cols = R.train_columns(9, 2 * 1024 + 1, 8)
    host, dev = C.train(cols, lab, 0.1, 1e-4), C.train(cols, lab, 0.1, 1e-4, backend="hip")
    assert host.status == dev.status == "converged"
    o = R.objective_ld(cols, lab, dev.theta, 0.1, 1e-4)
    for j in range(9):
        assert abs(float(o["g"][j])) <= 2 * math.sqrt(EPS * float(o["H"][j, j])) + R.eval_bound(cols.shape[1], 8, o["A"], o["g_abs"][j]), j
    assert np.allclose(dev.theta, host.theta, rtol=1e-6, atol=1e-9)


def test_the_three_ways_a_training_ends(C):
    s = np.concatenate([np.linspace(-3, -1, 20), np.linspace(1, 3, 20)])
    lab = (s > 0).astype(np.uint8)
    m = C.train(s, lab, max_iters=30, backend="hip")
    assert m.status == "not_converged" and m.evaluations == 30 and m.weights[0] > 1.0
    assert C.train(s, lab, l2=1e-3, backend="hip").status == "converged"
    lab2, cols = R.train_columns(3, 200, 1)
    m = C.train(np.stack([cols[0], cols[0]]), lab2, backend="hip")
    assert m.status == "singular" and m.weights == [0.0, 0.0] and m.bias == 0.0 and m.evaluations == 1


def test_planted_calibration_is_recovered(C):
    lab, llr = R.gaussian_llr(1, 4097)                                   # the seed of tests/test_cal_cpu.py
    s = (llr - 1.5) / 4
    for backend in ("host", "hip"):
        m = C.train(s, lab, p_target=0.3, backend=backend)
        print(backend, m)
        assert m.status == "converged" and abs(m.weights[0] - 4.0) < 0.25 and abs(m.bias - 1.5) < 0.25, (backend, m)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_score_and_report_on_the_device(C, tmp_path):
    """the report on `hip` against the host rule on the scores the device wrote (its fp32 cosines differ from the host's by rounding)"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import kaldi_io, scoring
    vecs = scoring.read_embeddings(os.path.join(GOLD, "test.iv"))
    mean = kaldi_io.read_vec_flt(os.path.join(GOLD, "mean.vec"))
    trials = os.path.join(GOLD, "trials")
    scores, labels = scoring.cosine_score(vecs, vecs, trials, mean)
    model = C.train(scores.astype(np.float64), labels)
    plain = scoring.score_and_report(vecs, vecs, trials, mean, backend="hip")
    dev = scoring.score_and_report(vecs, vecs, trials, mean, calibration=model, backend="hip", score_path=str(tmp_path / "scores"))
    assert {k: dev[k] for k in plain} == plain and sorted(set(dev) - set(plain)) == ["act_dcf", "cllr", "min_cllr"]
    _, written = C.read_score_files([str(tmp_path / "scores")])
    llr = C.apply(model, written)
    ev = C.evaluate(llr, labels, scoring.DEFAULT_COSTS)
    assert dev["act_dcf"] == [a["act_dcf"] for a in ev["act_dcf"]]
    assert abs(dev["cllr"] - ev["cllr"]) <= 2 * R.sum_bound(llr.size, ev["cllr"])
    hv, hp, _ = C.min_cllr(llr, labels)
    assert abs(dev["min_cllr"] - hv) <= 2 * R.sum_bound(hp.shape[0], hv)


def test_scripts_on_the_device_reproduce_the_host_files(C, tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    s, sn, tr = (os.path.join(GOLD, n) for n in ("scores", "scores_snorm", "trials"))

    def run(script, *flags):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(flags), env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r
    out = {}
    for b in ("host", "hip"):
        run("calibrate.py", "train", "--scores", s, sn, "--trials", tr, "--out", str(tmp_path / ("model_" + b)), "--backend", b)
        run("calibrate.py", "apply", "--model", str(tmp_path / "model_host"), "--scores", s, sn, "--score-out", str(tmp_path / ("llr_" + b)),
            "--backend", b)
        r = run("compute_cllr.py", "--backend", b, str(tmp_path / "llr_host"), tr)
        out[b] = (C.load(str(tmp_path / ("model_" + b))), C.read_score_files([str(tmp_path / ("llr_" + b))]), r.stdout,
                  [l for l in r.stderr.splitlines() if "misses" in l])
    assert np.allclose(out["hip"][0].theta, out["host"][0].theta, rtol=1e-9, atol=0.0)
    assert out["hip"][1][0] == out["host"][1][0] and np.array_equal(out["hip"][1][1], out["host"][1][1])     # apply: the same bits
    # each back end's own model on its own back end: the scores agree to 1e-12 of their scale
    run("calibrate.py", "apply", "--model", str(tmp_path / "model_hip"), "--scores", s, sn, "--score-out", str(tmp_path / "own"), "--backend", "hip")
    own, ref = C.read_score_files([str(tmp_path / "own")])[1][0], out["host"][1][1][0]
    print("own model on the device against the host files: largest difference / scale %.3g" % (np.abs(own - ref).max() / np.abs(ref).max()))
    assert np.abs(own - ref).max() <= 1e-12 * np.abs(ref).max()
    assert out["hip"][2] == out["host"][2] and out["hip"][3] == out["host"][3] and len(out["hip"][3]) == 2
