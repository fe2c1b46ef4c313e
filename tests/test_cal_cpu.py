"""Calibration and fusion of trial scores on the host (no GPU): calibration.py's `host` back end against the
restatement in tests/cal_ref.py - the pools of pool-adjacent-violators equal the minimax pools, the closed-form cases, the partition
property, apply and actDCF bit-equal to the stated expressions, the training bounds on the golden back-end scores, the three ways a
training ends, the model file - then scripts/calibrate.py, scripts/compute_cllr.py and the SPK_CALIBRATION hook of test.sh on files,
and the exports of csrc/cal.hip in the C ABI with their refusals."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "backend")
EPS = 1e-18


@pytest.fixture(scope="module")
def C():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import calibration
    return calibration


@pytest.fixture(scope="module")
def golden(C):
    pairs, cols = C.read_score_files([os.path.join(GOLD, "scores"), os.path.join(GOLD, "scores_snorm")])
    return pairs, cols, C.trial_labels(pairs, os.path.join(GOLD, "trials"))


def tied_case(seed):
    rng = np.random.RandomState(seed)
    T = int(rng.randint(2, 60))
    s = rng.randint(0, rng.randint(1, 12), size=T) / 4.0 - 1.0
    lab = (rng.rand(T) < rng.choice([0.2, 0.5, 0.8])).astype(np.uint8)
    lab[rng.randint(T)] = 1
    lab[(np.flatnonzero(lab)[0] + 1) % T] = 0
    return s, lab


# ---- pool-adjacent-violators ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(30))
def test_pools_equal_the_minimax_pools(C, seed):
    s, lab = tied_case(seed)
    tie, order = R.tie_pools(s.tolist(), lab.tolist())
    want = R.pav_minimax(tie)
    value, pools, pool_of, det = C.min_cllr(s, lab, details=True)
    assert [tuple(p) for p in det["tie_pools"].tolist()] == tie
    assert [tuple(p) for p in pools.tolist()] == want and pools.dtype == np.int64
    assert all(a[0] * b[1] < b[0] * a[1] for a, b in zip(want, want[1:]))               # t / n strictly increasing
    assert pool_of.tolist() == R.pool_index(want, order)
    n_tar = int(lab.sum())
    ld = R.min_cllr_ld(want, n_tar, lab.size - n_tar)
    assert abs(value - float(ld)) <= R.sum_bound(len(want), ld)
    # minCllr <= Cllr of every increasing affine map of the scores
    for a, b in ((1.0, 0.0), (4.0, -1.5), (0.25, 3.0)):
        assert value <= C.cllr(a * s + b, lab) + 1e-12


def test_closed_form_cases(C):
    T = 40
    lab = (np.arange(T) >= 25).astype(np.uint8)
    v, pools, pool_of = C.min_cllr(np.arange(T) / 3.0, lab)                              # perfectly separated
    assert v == 0.0 and pools.tolist() == [[0, 25], [15, 15]] and pool_of.tolist() == [0] * 25 + [1] * 15
    v, pools, _ = C.min_cllr(-np.arange(T) / 3.0, lab)                                   # reversed
    assert v == 1.0 and pools.tolist() == [[15, 40]]
    v, pools, _ = C.min_cllr(np.zeros(T), lab)                                           # all equal
    assert v == 1.0 and pools.tolist() == [[15, 40]]
    # a tie [0, 1] is one pool: per-trial pooling without the tie pools would keep (0, 1), (1, 1) apart
    v, pools, pool_of = C.min_cllr(np.array([0.0, 0.0]), np.array([0, 1]))
    assert pools.tolist() == [[1, 2]] and pool_of.tolist() == [0, 0] and v == 1.0
    assert C.min_cllr(np.array([-0.0, 0.0, 0.0, -0.0]), np.array([1, 0, 1, 0]))[1].tolist() == [[2, 4]]


@pytest.mark.parametrize("seed", range(10))
def test_partition_property(C, seed):
    """the rule on any partition of the initial pools, then on the concatenation of the results: the same pools"""
    rng = np.random.RandomState(100 + seed)
    P = int(rng.randint(2, 80))
    n = rng.randint(1, 6, size=P)
    pools = np.stack([rng.randint(0, n + 1), n], axis=1).astype(np.int64)
    want = R.pav_minimax([tuple(p) for p in pools.tolist()]) if P <= 40 else None
    whole = C.pav_pools(pools)
    if want is not None:
        assert [tuple(p) for p in whole.tolist()] == want
    for parts in range(3):
        cuts = np.sort(rng.choice(np.arange(1, P), size=min(P - 1, int(rng.randint(1, 6))), replace=False))
        pieces = [C.pav_pools(p) for p in np.split(pools, cuts)]
        assert np.array_equal(C.pav_pools(np.concatenate(pieces)), whole)


# ---- apply, Cllr, actDCF ----------------------------------------------------------------------------------------------------------------
def test_apply_is_the_stated_expression(C):
    rng = np.random.RandomState(2)
    for K in (1, 2, 3, 8):
        cols, th = rng.randn(K, 50) * 3, rng.randn(K + 1)
        want = []
        for i in range(50):
            z = th[0] * cols[0, i]
            for k in range(1, K):
                z = z + th[k] * cols[k, i]
            want.append(z + th[K])
        got = C.apply(C.Model(th[:K], th[K]), cols)
        assert got.dtype == np.float64 and got.tolist() == [float(w) for w in want]
    with pytest.raises(ValueError, match="columns"):
        C.apply(C.Model([1.0, 2.0], 0.0), rng.randn(3, 5))
    with pytest.raises(ValueError, match="NaN or infinite"):
        C.apply(C.Model([1.0], 0.0), np.array([0.0, np.inf]))
    with pytest.raises(ValueError, match="NaN or infinite"):
        C.apply(C.Model([1.0], 0.0), np.array([0.0, np.nan]))
    with pytest.raises(ValueError, match="1 <= K <= 8"):
        C.apply(C.Model([1.0], 0.0), rng.randn(9, 5))


def test_cllr_and_act_dcf_are_the_stated_expressions(C):
    lab, llr = R.gaussian_llr(5, 300)
    costs = [(0.01, 1, 1), (0.001, 1, 1), (0.5, 1, 1), (0.05, 10, 2)]
    ev = C.evaluate(llr, lab, costs)
    ld = R.cllr_ld(llr, lab)
    assert abs(ev["cllr"] - float(ld)) <= R.sum_bound(300, ld)
    assert C.cllr(llr, lab) == ev["cllr"] and ev["n_target"] == int(lab.sum()) and ev["n_nontarget"] == 300 - int(lab.sum())
    for (p, cm, cf), a in zip(costs, ev["act_dcf"]):
        want, miss, fa, eta = R.act_dcf(llr.tolist(), lab.tolist(), p, cm, cf)
        assert (a["act_dcf"], a["miss"], a["fa"], a["threshold"]) == (want, miss, fa, eta)                # bit for bit
        assert C.act_dcf(llr, lab, p, cm, cf) == want
    assert C.bayes_threshold(0.5) == 0.0
    # a score on the threshold is accepted: llr >= eta
    eta = C.bayes_threshold(0.01)
    a = C.evaluate(np.array([eta, eta, np.nextafter(eta, -np.inf)]), np.array([1, 0, 1]), [(0.01, 1, 1)])["act_dcf"][0]
    assert (a["miss"], a["fa"]) == (1, 1)
    assert 0.0 < ev["cllr"] < 1.0 and abs(C.cllr(np.zeros(10), np.arange(10) % 2) - 1.0) < 1e-15
    with pytest.raises(ValueError, match="at most 8"):
        C.evaluate(llr, lab, [(0.01, 1, 1)] * 9)
    with pytest.raises(ValueError, match="p_target"):
        C.evaluate(llr, lab, [(1.0, 1, 1)])
    with pytest.raises(ValueError, match="target and one non-target"):
        C.cllr(llr, np.ones(300))


# ---- training --------------------------------------------------------------------------------------------------------------------------
def check_training(C, cols, lab, model, p_target=0.01, l2=0.0):
    """the bounds of section 6s on a converged model; -> the longdouble objective at it"""
    K, T = cols.shape
    theta = model.theta
    o = R.objective_ld(cols, lab, theta, p_target, l2)
    for j in range(K + 1):
        slack = R.eval_bound(T, K, o["A"], o["g_abs"][j])
        assert abs(float(o["g"][j])) <= 2 * math.sqrt(EPS * float(o["H"][j, j])) + slack, (j, float(o["g"][j]), slack)
    assert abs(model.objective - float(o["f"])) <= R.eval_bound(T, K, o["A"], o["f_abs"])
    return o


@pytest.mark.parametrize("which", ["cosine", "snorm", "both"])
def test_training_on_the_golden_scores(C, golden, which):
    _, cols, lab = golden
    c = {"cosine": cols[:1], "snorm": cols[1:], "both": cols}[which]
    assert c.shape[1] == 66 and int(lab.sum()) == 12
    m = C.train(c, lab)
    assert m.status == "converged" and m.evaluations <= 20 and m.p_target == 0.01 and m.l2 == 0.0 and len(m.weights) == c.shape[0]
    o = check_training(C, c, lab, m)
    # one evaluation of the host back end at that theta against longdouble
    f, g, H = C.objective_terms(c, lab, m.theta, 0.01, 0.0)
    K = c.shape[0]
    assert abs(f - float(o["f"])) <= R.eval_bound(66, K, o["A"], o["f_abs"])
    for j in range(K + 1):
        assert abs(g[j] - float(o["g"][j])) <= R.eval_bound(66, K, o["A"], o["g_abs"][j])
        for k in range(K + 1):
            assert abs(H[j, k] - float(o["H"][j, k])) <= R.eval_bound(66, K, o["A"], o["H_abs"][j, k])
    # calibration lowers Cllr towards minCllr, and does not change minCllr when the weight is positive
    if K == 1:
        assert m.weights[0] > 0
        raw, cal = C.cllr(c[0], lab), C.cllr(C.apply(m, c), lab)
        assert C.min_cllr(c[0], lab)[1].tolist() == C.min_cllr(C.apply(m, c), lab)[1].tolist()
        assert C.min_cllr(c[0], lab)[0] <= cal + 1e-12 and (which == "snorm" or cal < raw)


@pytest.mark.parametrize("T,K", [(300, 1), (300, 3), (4097, 2)])
def test_training_on_gaussian_scores(C, T, K):
    lab, cols = R.train_columns(7, T, K)
    m = C.train(cols, lab, p_target=0.2, l2=1e-6)
    assert m.status == "converged" and m.evaluations <= 20
    check_training(C, cols, lab, m, p_target=0.2, l2=1e-6)


def planted(C):
    lab, llr = R.gaussian_llr(1, 4097)
    return lab, (llr - 1.5) / 4


def test_planted_calibration_is_recovered(C):
    """llr ~ N(+-mu, 2 mu) is calibrated at every prior, and the scores are (llr - 1.5) / 4: the model must undo that.  The seed was chosen so
    that the host back end lands within 0.25 of (4, 1.5); tests/test_cal_gpu.py holds the device to the same"""
    lab, s = planted(C)
    m = C.train(s, lab, p_target=0.3)
    assert m.status == "converged" and abs(m.weights[0] - 4.0) < 0.25 and abs(m.bias - 1.5) < 0.25, m
    assert abs(C.cllr(C.apply(m, s), lab) - C.min_cllr(s, lab)[0]) < 0.05


def test_the_three_ways_a_training_ends(C):
    s = np.concatenate([np.linspace(-3, -1, 20), np.linspace(1, 3, 20)])
    lab = (s > 0).astype(np.uint8)
    m = C.train(s, lab, max_iters=30)                                                    # separable, no penalty: by design
    assert m.status == "not_converged" and m.evaluations == 30 and m.weights[0] > 1.0
    m = C.train(s, lab, l2=1e-3)
    assert m.status == "converged" and m.evaluations < 100
    check_training(C, s[None], lab, m, l2=1e-3)
    lab2, cols = R.train_columns(3, 200, 1)
    m = C.train(np.stack([cols[0], cols[0]]), lab2)                                      # two identical columns
    assert m.status == "singular" and m.weights == [0.0, 0.0] and m.bias == 0.0 and m.evaluations == 1
    for bad in (dict(p_target=0.0), dict(p_target=1.0), dict(l2=-1.0), dict(epsilon=-1.0), dict(max_iters=0)):
        with pytest.raises(ValueError):
            C.train(s, lab, **bad)
    with pytest.raises(ValueError, match="target and one non-target"):
        C.train(s, np.zeros(40))
    with pytest.raises(ValueError, match="backend"):
        C.train(s, lab, backend="cuda")


def test_model_file_round_trips(C, tmp_path):
    m = C.Model([0.1 + 0.2, -1e-300, 12345.678901234567], -2.264272462370302, p_target=0.0123456789012345678, l2=1e-7)
    f = str(tmp_path / "model")
    C.save(m, f)
    text = open(f).read().splitlines()
    assert text[0] == "spk-calibration 1" and [l.split()[0] for l in text[1:]] == ["p_target", "l2", "systems", "weight", "weight", "weight", "bias"]
    got = C.load(f)
    assert (got.weights, got.bias, got.p_target, got.l2) == (m.weights, m.bias, m.p_target, m.l2)
    for old, new, words in (("spk-calibration 1", "spk-calibration 9", ["not a calibration model"]), ("systems 3", "systems 2", ["line 7", "bias"]),
                            ("bias -", "bias x", ["bias"]), ("systems 3", "systems 0", ["systems"])):
        (tmp_path / "bad").write_text(open(f).read().replace(old, new))
        with pytest.raises(ValueError) as e:
            C.load(str(tmp_path / "bad"))
        assert all(w in str(e.value) for w in words), str(e.value)


# ---- scoring.score_and_report ----------------------------------------------------------------------------------------------------------
def test_score_and_report_with_a_model(C):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import scoring
    from pytorch_kaldi_resnet_amd import kaldi_io
    vecs = scoring.read_embeddings(os.path.join(GOLD, "test.iv"))
    mean = kaldi_io.read_vec_flt(os.path.join(GOLD, "mean.vec"))
    trials = os.path.join(GOLD, "trials")
    plain = scoring.score_and_report(vecs, vecs, trials, mean)
    assert sorted(plain) == ["eer", "eer_index", "min_dcf", "n_nontarget", "n_target"]
    scores, labels = scoring.cosine_score(vecs, vecs, trials, mean)
    model = C.train(scores.astype(np.float64), labels)
    rep = scoring.score_and_report(vecs, vecs, trials, mean, calibration=model)
    assert {k: rep[k] for k in plain} == plain and sorted(set(rep) - set(plain)) == ["act_dcf", "cllr", "min_cllr"]
    llr = C.apply(model, scores.astype(np.float64))
    assert rep["cllr"] == C.cllr(llr, labels) and rep["min_cllr"] == C.min_cllr(llr, labels)[0]
    assert rep["act_dcf"] == [C.act_dcf(llr, labels, 0.01), C.act_dcf(llr, labels, 0.001)]
    with pytest.raises(ValueError, match="one system"):
        scoring.score_and_report(vecs, vecs, trials, mean, calibration=C.Model([1.0, 1.0], 0.0))


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
def run(script, *flags, env=None):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT
    e.update(env or {})
    cmd = ["bash", os.path.join(ROOT, script)] if script.endswith(".sh") else [sys.executable, os.path.join(ROOT, "scripts", script)]
    return subprocess.run(cmd + list(flags), env=e, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def cli(C, golden, tmp_path_factory):
    d = tmp_path_factory.mktemp("cal_cli")
    s, sn, tr = (os.path.join(GOLD, n) for n in ("scores", "scores_snorm", "trials"))
    r = run("calibrate.py", "train", "--scores", s, sn, "--trials", tr, "--out", str(d / "fusion"))
    assert r.returncode == 0, r.stderr[-2000:]
    r = run("calibrate.py", "train", "--scores", s, "--trials", tr, "--out", str(d / "cosine"))
    assert r.returncode == 0, r.stderr[-2000:]
    return d, s, sn, tr


def test_calibrate_script_trains_and_applies(C, golden, cli):
    d, s, sn, tr = cli
    _, cols, lab = golden
    m, want = C.load(str(d / "fusion")), C.train(cols, lab)
    assert (m.weights, m.bias, m.p_target, m.l2) == (want.weights, want.bias, 0.01, 0.0)
    r = run("calibrate.py", "apply", "--model", str(d / "fusion"), "--scores", s, sn, "--score-out", str(d / "fused"))
    assert r.returncode == 0, r.stderr[-2000:]
    pairs, got = C.read_score_files([str(d / "fused")])
    assert pairs == golden[0] and got[0].tolist() == C.apply(want, cols).tolist()         # repr round-trips
    r = run("compute_cllr.py", str(d / "fused"), tr)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert [l.split(":")[0] for l in lines] == ["Cllr", "minCllr", "actDCF(p-target=0.01)", "actDCF(p-target=0.001)"]
    ev = C.evaluate(got[0], lab, [(0.01, 1, 1), (0.001, 1, 1)])
    assert lines[0] == "Cllr: %.4f" % ev["cllr"] and lines[1] == "minCllr: %.4f" % C.min_cllr(got[0], lab)[0]
    assert lines[2] == "actDCF(p-target=0.01): %.4f" % ev["act_dcf"][0]["act_dcf"]
    r = run("compute_cllr.py", "--p-target", "0.5", "--c-miss", "10", "--c-fa", "2", str(d / "fused"), tr)
    assert r.returncode == 0 and r.stdout.splitlines()[2] == "actDCF(p-target=0.5): %.4f" % C.act_dcf(got[0], lab, 0.5, 10, 2)
    # options reach the training
    r = run("calibrate.py", "train", "--scores", s, "--trials", tr, "--out", str(d / "m2"), "--p-target", "0.1", "--l2", "0.01", "--epsilon",
            "1e-12", "--max-iters", "50")
    assert r.returncode == 0, r.stderr[-2000:]
    m, want = C.load(str(d / "m2")), C.train(cols[:1], lab, 0.1, 0.01, 1e-12, 50)
    assert (m.weights, m.bias, m.p_target, m.l2) == (want.weights, want.bias, 0.1, 0.01)


def test_script_errors(C, cli, tmp_path):
    d, s, sn, tr = cli
    lines = open(s).read().splitlines()
    (tmp_path / "swapped").write_text("\n".join(lines[:4] + [lines[5], lines[4]] + lines[6:]) + "\n")
    (tmp_path / "short").write_text("\n".join(lines[:10]) + "\n")
    (tmp_path / "words").write_text("\n".join(lines[:2] + ["a b"] + lines[3:]) + "\n")
    (tmp_path / "nan").write_text("\n".join(lines[:7] + [" ".join(lines[7].split()[:2]) + " nan"] + lines[8:]) + "\n")
    out = str(tmp_path / "never")
    train = ["train", "--trials", tr, "--out", out]
    for script, flags, words in (
            ("calibrate.py", train + ["--scores", s, str(tmp_path / "swapped")], ["swapped:5", "not the trial"]),
            ("calibrate.py", train + ["--scores", s, str(tmp_path / "short")], ["short:11", "ends after 10"]),
            ("calibrate.py", train + ["--scores", str(tmp_path / "words")], ["words:3"]),
            ("calibrate.py", train + ["--scores", str(tmp_path / "nan")], ["nan:8", "NaN"]),
            ("calibrate.py", train + ["--scores", s, "--p-target", "1.5"], ["--p-target"]),
            ("calibrate.py", train + ["--scores", s, "--l2", "-1"], ["--l2"]),
            ("calibrate.py", train + ["--scores", s, "--max-iters", "0"], ["--max-iters"]),
            ("calibrate.py", train + ["--scores", s, "--backend", "cuda"], ["--backend"]),
            ("calibrate.py", train + ["--scores"] + [s] * 9, ["--scores", "8"]),
            ("calibrate.py", ["train", "--scores", s, "--trials", str(tmp_path / "missing"), "--out", out], ["missing"]),
            ("calibrate.py", [], ["train or apply"]),
            ("calibrate.py", ["apply", "--model", str(d / "fusion"), "--scores", s, "--score-out", out], ["1 files", "2 systems"]),
            ("calibrate.py", ["apply", "--model", s, "--scores", s, "--score-out", out], ["not a calibration model"]),
            ("compute_cllr.py", [s, str(tmp_path / "missing")], ["missing"]),
            ("compute_cllr.py", ["--p-target", "0", s, tr], ["p_target"]),
            ("compute_cllr.py", ["--backend", "cuda", s, tr], ["--backend"]),
            ("compute_cllr.py", [str(tmp_path / "words"), tr], ["words:3"])):
        r = run(script, *flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    assert not os.path.exists(out)
    # a training that does not converge writes its model, says so and exits with 3
    sep = tmp_path / "sep"
    sep.write_text("".join("a%d b %r\n" % (i, float(i - 10)) for i in range(20)))
    (tmp_path / "sep_trials").write_text("".join("a%d b %s\n" % (i, "target" if i >= 10 else "nontarget") for i in range(20)))
    r = run("calibrate.py", "train", "--scores", str(sep), "--trials", str(tmp_path / "sep_trials"), "--out", str(tmp_path / "sep_model"),
            "--max-iters", "12")
    assert r.returncode == 3 and "not_converged" in r.stderr and C.load(str(tmp_path / "sep_model")).weights[0] > 0, r.stderr


def test_test_sh_hook(C, golden, cli, tmp_path):
    """without SPK_CALIBRATION every file is what it was; with it stage 12 adds <scores>_cal and stage 13 <report>_cal"""
    d, s, sn, tr = cli
    _, cols, lab = golden
    outs = {}
    for name, env in (("plain", {}), ("cal", {"SPK_CALIBRATION": str(d / "cosine")})):
        w = tmp_path / name
        w.mkdir()
        for f in ("mean.vec", "test.iv", "trials"):
            shutil.copy(os.path.join(GOLD, f), str(w / f))
        r = run("test.sh", str(w), str(w), "cosine", "12", str(w / "trials"), env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = (r.stdout, {f: open(str(w / f), "rb").read() for f in sorted(os.listdir(str(w))) if os.path.isfile(str(w / f))})
    plain, cal = outs["plain"][1], outs["cal"][1]
    assert sorted(plain) == ["eer_cosine", "mean.vec", "scores_cosine", "test.iv", "trials"]
    assert sorted(set(cal) - set(plain)) == ["eer_cosine_cal", "scores_cosine_cal"] and all(cal[f] == plain[f] for f in plain)
    assert plain["eer_cosine"] == open(os.path.join(GOLD, "eer_cosine"), "rb").read()
    assert outs["cal"][0] == outs["plain"][0] + cal["eer_cosine_cal"].decode()
    _, raw = C.read_score_files([str(tmp_path / "cal" / "scores_cosine")])
    _, got = C.read_score_files([str(tmp_path / "cal" / "scores_cosine_cal")])
    model = C.load(str(d / "cosine"))
    assert got[0].tolist() == C.apply(model, raw).tolist()
    ev = C.evaluate(got[0], lab, [(0.01, 1, 1), (0.001, 1, 1)])
    assert cal["eer_cosine_cal"].decode().splitlines() == [
        "Cllr: %.4f" % ev["cllr"], "minCllr: %.4f" % C.min_cllr(got[0], lab)[0],
        "actDCF(p-target=0.01): %.4f" % ev["act_dcf"][0]["act_dcf"], "actDCF(p-target=0.001): %.4f" % ev["act_dcf"][1]["act_dcf"]]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ["spk_cal_max_k", "spk_cal_tile", "spk_cal_apply", "spk_cal_cllr_ws_elems", "spk_cal_train_ws_elems", "spk_cal_pav_ws_elems",
       "spk_cal_cllr", "spk_cal_train", "spk_cal_pav"]


def test_exports_are_declared_bound_and_exported():
    """the calibration entries have a header of their own, include/spkcal.h, and a binding table of their own: every name it declares
    is bound with as many parameters and exported, and the other two headers and their counts are as they were"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spkcal.h")).read(), flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|long long)\s+(spk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(decl) == sorted(NEW) == sorted(hip.cal_symbols()) == sorted(hip._CAL_SIGS)
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    others = open(os.path.join(ROOT, "include", "spkhip.h")).read() + open(os.path.join(ROOT, "include", "spkder.h")).read()
    for name in NEW:
        assert hasattr(hip.lib(), name) and re.search(r" T %s$" % name, nm, re.M), name
        params = [p for p in decl[name][1].split(",") if p.strip() != "void"]
        assert len(params) == len(hip._CAL_SIGS[name]), name
        assert (decl[name][0] == "long long") == (getattr(hip.lib(), name).restype is ctypes.c_longlong), name
        assert name not in hip.exported_symbols() and name not in hip.der_symbols() and not re.search(r"\b%s\b" % name, others), name
    exported = set(re.findall(r" T (spk_[a-z0-9_]+)$", nm, re.M))
    assert exported == set(hip.exported_symbols()) | set(hip.der_symbols()) | set(NEW)
    lib = hip.lib()
    assert lib.spk_cal_max_k() == 8 and lib.spk_cal_tile(0) % lib.spk_cal_tile(3) == 0 and lib.spk_cal_tile(1) >= 64
    assert lib.spk_cal_tile(2) >= 40 + 45
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "include/spkcal.h" in readme and "(128 exports)" in readme and "include/spkder.h" in readme


def test_calls_are_refused_on_the_host_before_any_launch():
    """no device is needed: a refused call launches nothing and touches no pointer"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    lib, P = hip.lib(), 16
    th = np.zeros(9)
    block = lib.spk_cal_tile(0)

    def refused(rc, name):
        assert rc < 0 and name.encode() in lib.spk_last_error(), (name, rc, lib.spk_last_error())
    for K in (0, 9, -1):
        refused(lib.spk_cal_apply(P, th.ctypes.data, K, P, 10, None), "spk_cal_apply")
        refused(lib.spk_cal_train(P, P, K, 10, 3, 0.01, -4.6, 0.0, 1e-18, 10, P, P, P, 1 << 20, None), "spk_cal_train")
        assert lib.spk_cal_train_ws_elems(10, K) < 0
    refused(lib.spk_cal_apply(P, th.ctypes.data, 1, P, 0, None), "spk_cal_apply")
    refused(lib.spk_cal_apply(None, th.ctypes.data, 1, P, 10, None), "spk_cal_apply")
    refused(lib.spk_cal_apply(P, None, 1, P, 10, None), "spk_cal_apply")
    refused(lib.spk_cal_apply(P, th.ctypes.data, 1, None, 10, None), "spk_cal_apply")
    costs, eta = np.array([0.01, 1.0, 1.0]), np.array([4.6])

    def cllr(T=10, Pn=1, ws=1 << 20, null=None, c=costs.ctypes.data, e=eta.ctypes.data):
        p = [None if i == null else P for i in range(5)]
        return lib.spk_cal_cllr(p[0], p[1], c, e, Pn, p[2], p[3], p[4], ws, T, None)
    for kw in (dict(T=1), dict(T=0), dict(Pn=9), dict(Pn=-1), dict(c=None), dict(e=None), dict(ws=lib.spk_cal_cllr_ws_elems(10) - 1),
               dict(T=block + 1, ws=lib.spk_cal_cllr_ws_elems(block)), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4)):
        refused(cllr(**kw), "spk_cal_cllr")

    def train(T=10, n_tar=3, p=0.01, l2=0.0, eps=1e-18, iters=10, ws=1 << 20, null=None, K=2):
        q = [None if i == null else P for i in range(5)]
        return lib.spk_cal_train(q[0], q[1], K, T, n_tar, p, -4.6, l2, eps, iters, q[2], q[3], q[4], ws, None)
    for kw in (dict(T=1), dict(n_tar=0), dict(n_tar=10), dict(p=0.0), dict(p=1.0), dict(l2=-1.0), dict(eps=-1.0), dict(iters=0),
               dict(ws=lib.spk_cal_train_ws_elems(10, 2) - 1), dict(T=block + 1, ws=lib.spk_cal_train_ws_elems(block, 2)),
               dict(ws=lib.spk_cal_train_ws_elems(10, 1)), dict(null=0), dict(null=1), dict(null=2), dict(null=3), dict(null=4)):
        refused(train(**kw), "spk_cal_train")

    def pav(T=10, ws=1 << 20, null=None):
        q = [None if i == null else P for i in range(9)]
        return lib.spk_cal_pav(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], ws, T, 0, None)
    for kw in (dict(T=1), dict(T=-5), dict(ws=lib.spk_cal_pav_ws_elems(10) - 1)) + tuple(dict(null=i) for i in range(9)):
        refused(pav(**kw), "spk_cal_pav")
    assert lib.spk_cal_cllr_ws_elems(0) < 0 and lib.spk_cal_pav_ws_elems(0) < 0 and lib.spk_cal_train_ws_elems(0, 1) < 0
    nb = lambda T: -(-T // block)                                                        # noqa: E731
    for T in (2, block, block + 1, 5 * block + 3):
        assert lib.spk_cal_cllr_ws_elems(T) == nb(T) * 19 and lib.spk_cal_train_ws_elems(T, 8) == nb(T) * 55
        assert lib.spk_cal_train_ws_elems(T, 1) == nb(T) * 6
        assert lib.spk_cal_pav_ws_elems(T) == 4 * (T + 1) + 2 * (nb(T) + 1) + -(-T // lib.spk_cal_tile(1)) + 1
