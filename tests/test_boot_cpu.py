"""Speaker-level bootstrap of the evaluation report without a GPU: the host back end against the independent
restatement of tests/boot_ref.py, bit for bit, the host logic around it, the script, the test.sh hook and the C ABI of
include/spkboot.h."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import boot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "backend")
COSTS = [(0.01, 1.0, 1.0), (0.001, 1.0, 1.0), (0.05, 10.0, 2.0)]
ACT = [(0.5, 1.0, 1.0), (0.3, 1.0, 2.0)]        # thresholds 0 and log(14 / 3): inside the score range of the cases


@pytest.fixture(scope="module")
def B():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import bootstrap
    return bootstrap


@pytest.fixture(scope="module")
def S():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import scoring
    return scoring


def make_case(U, T, seed):
    """every unit has a target trial and every pair of units a non-target trial; scores with one decimal (many ties), -0.0 and +0.0"""
    rng = np.random.RandomState(seed)
    ua = list(range(U)) + [a for a in range(U) for b in range(a + 1, U)]
    ub = list(range(U)) + [b for a in range(U) for b in range(a + 1, U)]
    lab = [1] * U + [0] * (len(ua) - U)
    assert len(ua) <= T
    while len(ua) < T:
        a, b = int(rng.randint(U)), int(rng.randint(U))
        ua.append(a)
        ub.append(b)
        lab.append(1 if a == b else int(rng.rand() < 0.1))       # (a few targets across units: ids that are their own unit)
    lab = np.array(lab, dtype=np.uint8)
    s = np.round(rng.randn(T) + 1.5 * lab, 1)
    s[s == 0.0] = np.where(rng.rand(int((s == 0.0).sum())) < 0.5, -0.0, 0.0)
    if T >= 4:
        s[rng.randint(T)], s[rng.randint(T)] = -0.0, 0.0
    return s, lab, np.array(ua, dtype=np.int32), np.array(ub, dtype=np.int32)


CASES = {"U2": (2, 40, 1), "U6": (6, 700, 2), "U12": (12, 5000, 3)}


def planted_rows(s, ua, ub, U):
    """one unit drawn U times; zeros on the units of the lowest-scored trials (the list opens with a run of weight 0); all ones"""
    one = np.zeros(U, dtype=np.int64)
    one[U // 2] = U
    zeros = np.ones(U, dtype=np.int64)
    low = np.lexsort((np.arange(len(s)), s + 0.0))[:3]
    zeros[ua[low]] = 0
    zeros[ub[low]] = 0
    if zeros.any():                                             # (U = 2: nothing is left, the row is degenerate)
        zeros[np.flatnonzero(zeros)[0]] += int((zeros == 0).sum())
    return np.stack([one, zeros, np.ones(U, dtype=np.int64)])


def assert_matches_ref(rep, s, lab, ua, ub, counts, costs, act):
    P, Pa = len(costs), len(act)
    for r in range(counts.shape[0]):
        ref = R.replicate(s.tolist(), lab.tolist(), ua.tolist(), ub.tolist(), counts[r].tolist(), costs, act)
        d, i = rep["d"][r], rep["i"][r]
        assert (i[0], i[1], i[2]) == (ref["flag"], ref["n_tar"], ref["n_non"]), r
        if ref["flag"]:
            assert np.isnan(d).all() and (i[3:] == -1).all() and rep["degenerate"][r], r
            continue
        assert d[0].tobytes() == np.float64(ref["eer"]).tobytes() and i[3] == ref["eer_pos"], r
        for m in range(P):
            assert d[1 + m].tobytes() == np.float64(ref["min_dcf"][m][0]).tobytes() and i[4 + m] == ref["min_dcf"][m][1], (r, m)
        for m in range(Pa):
            assert d[1 + P + m].tobytes() == np.float64(ref["act"][m][0]).tobytes(), (r, m)
            assert (i[4 + P + m], i[4 + P + Pa + m]) == ref["act"][m][1:], (r, m)


# ---- the counts table -----------------------------------------------------------------------------------------------------------------
def test_counts_table_is_the_stated_hash(B):
    got = B.bootstrap_counts(5, 3, 7)
    assert got.tolist() == [[1, 3, 0, 1, 0], [0, 1, 1, 2, 1], [1, 1, 0, 3, 0]] == R.counts_table(5, 3, 7)
    assert B.bootstrap_counts(5, 2, 8).tolist() == [[0, 1, 2, 2, 0], [2, 0, 2, 0, 1]]
    for U, n, seed in ((1, 4, 0), (40, 9, 123), (1251, 3, 2 ** 64 + 5)):
        t = B.bootstrap_counts(U, n, seed)
        assert t.shape == (n, U) and (t.sum(1) == U).all() and t.min() >= 0
        assert t.tolist() == R.counts_table(U, n, seed)
        assert (B.bootstrap_counts(U, n + 3, seed)[:n] == t).all()                 # row r does not depend on R
    assert not (B.bootstrap_counts(40, 9, 123) == B.bootstrap_counts(40, 9, 124)).all()
    assert not (B.bootstrap_counts(40, 8, 124) == B.bootstrap_counts(40, 9, 123)[1:]).all()        # seeds are not shifted copies
    for bad in ((0, 3), (65536, 3), (5, 0)):
        with pytest.raises(ValueError):
            B.bootstrap_counts(bad[0], bad[1], 0)


def test_trial_units(B, tmp_path):
    pairs = [("a-1", "a-2"), ("a-1", "b-1"), ("b-2", "a-2"), ("c-1", "c-1")]
    ua, ub, names = B.trial_units(pairs)
    assert names == ["a-1", "a-2", "b-1", "b-2", "c-1"] and ua.tolist() == [0, 0, 3, 4] and ub.tolist() == [1, 2, 1, 4]
    m = {u: u.split("-")[0] for p in pairs for u in p}
    ua, ub, names = B.trial_units(pairs, m)
    assert names == ["a", "b", "c"] and ua.tolist() == [0, 0, 1, 2] and ub.tolist() == [0, 1, 0, 2] and ua.dtype == np.int32
    f = tmp_path / "utt2spk"
    f.write_text("".join("%s %s\n" % kv for kv in m.items()))
    assert B.trial_units(pairs, str(f))[2] == names
    del m["b-2"]
    with pytest.raises(ValueError, match="b-2"):
        B.trial_units(pairs, m)


# ---- the sweep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_all_ones_row_is_the_plain_report(B, S, name):
    from pytorch_kaldi_resnet_amd import calibration
    s, lab, ua, ub = make_case(*CASES[name])
    assert (s == 0.0).sum() >= 2 and np.signbit(s[s == 0.0]).any() and not np.signbit(s[s == 0.0]).all()
    U = CASES[name][0]
    rep = B.bootstrap_replicates(s, lab, ua, ub, np.ones((2, U), dtype=np.int64), COSTS, ACT)
    want = S.error_rates(s, lab, COSTS)
    ev = calibration.evaluate(s, lab, ACT)
    for r in range(2):
        assert rep["eer"][r].tobytes() == np.float64(want["eer"]).tobytes() and rep["eer_index"][r] == want["eer_index"]
        assert (rep["n_target"][r], rep["n_nontarget"][r], rep["degenerate"][r]) == (want["n_target"], want["n_nontarget"], False)
        for m in range(len(COSTS)):
            assert rep["min_dcf"][r, m].tobytes() == np.float64(want["min_dcf"][m][0]).tobytes()
            assert rep["min_dcf_index"][r, m] == want["min_dcf"][m][2]
        for m in range(len(ACT)):
            assert rep["act_dcf"][r, m].tobytes() == np.float64(ev["act_dcf"][m]["act_dcf"]).tobytes()
            assert (rep["miss"][r, m], rep["fa"][r, m]) == (ev["act_dcf"][m]["miss"], ev["act_dcf"][m]["fa"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_weighted_sweep_against_the_restatement(B, name):
    U, T, seed = CASES[name]
    s, lab, ua, ub = make_case(U, T, seed)
    counts = np.concatenate([B.bootstrap_counts(U, 6, seed), planted_rows(s, ua, ub, U)])
    rep = B.bootstrap_replicates(s, lab, ua, ub, counts, COSTS, ACT)
    assert rep["d"].shape == (9, 1 + 3 + 2) and rep["i"].shape == (9, 4 + 3 + 4)
    assert rep["degenerate"][6] and not rep["degenerate"][8]
    assert rep["i"][7, 3] >= 3 or U == 2                       # the EER is not taken inside the opening run of weight 0
    assert_matches_ref(rep, s, lab, ua, ub, counts, COSTS, ACT)
    # no costs at all, and eight of each
    rep0 = B.bootstrap_replicates(s, lab, ua, ub, counts, (), ())
    assert rep0["d"].shape == (9, 1) and rep0["d"][:, 0].tobytes() == rep["d"][:, 0].tobytes()
    eight = [(p, 1.0, 1.0) for p in (0.5, 0.3, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0001)]
    rep8 = B.bootstrap_replicates(s, lab, ua, ub, counts[:3], eight, eight)
    assert_matches_ref(rep8, s, lab, ua, ub, counts[:3], eight, eight)


def test_counts_of_65535_at_two_trials(B):
    s, lab = np.array([0.5, -0.5]), np.array([1, 0])
    ua, ub = np.array([0, 0]), np.array([0, 1])
    counts = np.array([[65535, 65535], [65535, 1], [1, 65535], [65535, 0]])
    rep = B.bootstrap_replicates(s, lab, ua, ub, counts, COSTS, ACT)
    assert rep["n_target"].tolist() == [65535, 65535, 1, 65535] and rep["n_nontarget"].tolist() == [65535 ** 2, 65535, 65535, 0]
    assert rep["degenerate"].tolist() == [False, False, False, True]
    assert_matches_ref(rep, s, lab, ua, ub, counts, COSTS, ACT)


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_equal_the_replicated_list(B, S, name):
    """n_tar, n_non, miss and fa of a row are plain counts on the trial list with every unit copied as often as it was drawn"""
    from pytorch_kaldi_resnet_amd import calibration
    U, T, seed = CASES[name]
    s, lab, ua, ub = make_case(U, T, seed)
    counts = np.concatenate([B.bootstrap_counts(U, 4, seed + 10), planted_rows(s, ua, ub, U)[1:]])
    rep = B.bootstrap_replicates(s, lab, ua, ub, counts, (), ACT)
    seen = 0
    for r in range(counts.shape[0]):
        s2, lab2 = R.replicated_list(s.tolist(), lab.tolist(), ua.tolist(), ub.tolist(), counts[r].tolist())
        n_tar = sum(lab2)
        assert (rep["n_target"][r], rep["n_nontarget"][r]) == (n_tar, len(lab2) - n_tar), r
        if rep["degenerate"][r]:
            continue
        seen += 1
        ev = calibration.evaluate(np.array(s2), np.array(lab2), ACT)
        want = S.error_rates(np.array(s2), np.array(lab2), COSTS[:1])                  # (its thresholds also fall between copies)
        assert (rep["n_target"][r], rep["n_nontarget"][r]) == (want["n_target"], want["n_nontarget"]), r
        for m in range(len(ACT)):
            assert (rep["miss"][r, m], rep["fa"][r, m]) == (ev["act_dcf"][m]["miss"], ev["act_dcf"][m]["fa"]), (r, m)
            assert rep["act_dcf"][r, m].tobytes() == np.float64(ev["act_dcf"][m]["act_dcf"]).tobytes(), (r, m)
    assert seen >= 2


# ---- reports --------------------------------------------------------------------------------------------------------------------------
def test_degenerate_replicates_are_left_out_and_counted(B):
    s, lab, ua, ub = make_case(*CASES["U2"])
    with pytest.raises(ValueError, match="degenerate"):
        B.bootstrap_report(s, lab, ua, ub, COSTS, replicates=200, seed=7)
    rep = B.bootstrap_report(s, lab, ua, ub, COSTS, replicates=200, seed=7, max_degenerate=1.0)
    flags = np.array([min(row) == 0 for row in R.counts_table(2, 200, 7)])
    assert 60 <= rep["degenerate"] == int(flags.sum()) <= 140 and rep["replicates"] == 200
    assert (rep["values"]["degenerate"] == flags).all()
    v = rep["values"]["eer"][~flags]
    assert not np.isnan(v).any() and (rep["eer"]["lo"], rep["eer"]["hi"]) == tuple(np.quantile(v, [0.025, 0.975]))
    with pytest.raises(ValueError, match="fewer than 2"):
        B.bootstrap_report(s, lab, ua, ub, COSTS, counts=np.array([[2, 0], [0, 2], [1, 1]]), max_degenerate=1.0)


@pytest.mark.parametrize("name", ["U6", "U12"])
def test_intervals_are_quantiles_of_the_restated_values(B, S, name):
    from pytorch_kaldi_resnet_amd import calibration
    U, T, seed = CASES[name]
    s, lab, ua, ub = make_case(U, T, seed)
    n = 40 if name == "U6" else 12
    rep = B.bootstrap_report(s, lab, ua, ub, COSTS, ACT, replicates=n, seed=7, alpha=0.1)
    table = R.counts_table(U, n, 7)
    assert (B.bootstrap_counts(U, 2000, 7).min(1) < U).all()                       # no unit is drawn U times: nothing degenerate
    refs = [R.replicate(s.tolist(), lab.tolist(), ua.tolist(), ub.tolist(), row, COSTS, ACT) for row in table]
    assert rep["degenerate"] == 0 and rep["replicates"] == n and rep["units"] == U and rep["alpha"] == 0.1
    point, ev = S.error_rates(s, lab, COSTS), calibration.evaluate(s, lab, ACT)

    def same(entry, value, values):
        lo, hi = np.quantile(np.array(values), [0.05, 0.95])
        assert (entry["value"], entry["lo"], entry["hi"]) == (value, lo, hi)
        assert entry["mean"] == float(np.mean(values)) and entry["std"] == float(np.std(values)) and entry["lo"] <= entry["hi"]
    same(rep["eer"], point["eer"], [x["eer"] for x in refs])
    for m in range(len(COSTS)):
        same(rep["min_dcf"][m], point["min_dcf"][m][0], [x["min_dcf"][m][0] for x in refs])
    for m in range(len(ACT)):
        same(rep["act_dcf"][m], ev["act_dcf"][m]["act_dcf"], [x["act"][m][0] for x in refs])


def test_compare_two_systems(B):
    U, T, seed = CASES["U6"]
    s, lab, ua, ub = make_case(U, T, seed)
    sb = np.round(s + np.random.RandomState(5).randn(T) * 0.7, 1)
    both = B.bootstrap_compare(s, sb, lab, ua, ub, COSTS, ACT, replicates=30, seed=3)
    va = B.bootstrap_replicates(s, lab, ua, ub, B.bootstrap_counts(U, 30, 3), COSTS, ACT)
    vb = B.bootstrap_replicates(sb, lab, ua, ub, B.bootstrap_counts(U, 30, 3), COSTS, ACT)
    assert both["a"]["values"]["d"].tobytes() == va["d"].tobytes() and both["b"]["values"]["d"].tobytes() == vb["d"].tobytes()
    d = va["eer"] - vb["eer"]
    e = both["diff"]["eer"]
    assert (e["lo"], e["hi"]) == tuple(np.quantile(d, [0.025, 0.975])) and e["below_zero"] == float(np.mean(d < 0))
    assert e["value"] == both["a"]["eer"]["value"] - both["b"]["eer"]["value"] and e["below_zero"] > 0.5
    d = va["act_dcf"][:, 1] - vb["act_dcf"][:, 1]
    assert both["diff"]["act_dcf"][1]["mean"] == float(np.mean(d)) and len(both["diff"]["min_dcf"]) == 3
    same = B.bootstrap_compare(s, s.copy(), lab, ua, ub, COSTS, replicates=20, seed=3)["diff"]
    for e in [same["eer"]] + same["min_dcf"]:
        assert (e["value"], e["lo"], e["hi"], e["mean"], e["std"], e["below_zero"]) == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    # matching by '<utt1> <utt2>'
    pairs = [("e%d" % t, "t%d" % t) for t in range(T)]
    perm = np.random.RandomState(9).permutation(T)
    assert (B.match_scores(pairs, s, [pairs[t] for t in perm], sb[perm]) == sb).all()
    with pytest.raises(ValueError, match="'e3 t3' is missing from the second"):
        B.match_scores(pairs, s, [pairs[t] for t in perm if t != 3], sb[perm][perm != 3])
    with pytest.raises(ValueError, match="'x y' is missing from the first"):
        B.match_scores(pairs, s, pairs + [("x", "y")], np.append(sb, 0.0))
    with pytest.raises(ValueError, match="twice"):
        B.match_scores(pairs, s, pairs[:-1] + [pairs[0]], sb)


def test_refusals(B):
    s, lab, ua, ub = make_case(*CASES["U6"])
    ones = np.ones((2, 6), dtype=np.int64)
    bad = s.copy()
    bad[5] = np.nan
    big = ones.copy()
    big[1, 2] = 65536
    neg = ones.copy()
    neg[0, 0] = -1
    out = ua.copy()
    out[7] = 6
    for args, kw, words in (((bad, lab, ua, ub, ones), {}, "NaN"),
                            ((s, np.ones_like(lab), ua, ub, ones), {}, "at least one target"),
                            ((s, np.zeros_like(lab), ua, ub, ones), {}, "at least one target"),
                            ((s, lab, out, ub, ones), {}, "unit id"),
                            ((s, lab, ua, -ub - 1, ones), {}, "unit id"),
                            ((s, lab, ua, ub, big), {}, "65535"),
                            ((s, lab, ua, ub, neg), {}, "65535"),
                            ((s, lab, ua, ub, ones * 1.5), {}, "integer table"),
                            ((s, lab, ua, ub, ones[0]), {}, "integer table"),
                            ((s, lab, ua, ub, np.ones((2, 65536), dtype=np.int64)), {}, "units"),
                            ((s[:-1], lab, ua, ub, ones), {}, "scores for"),
                            ((s, lab, ua[:-1], ub, ones), {}, "unit ids for"),
                            ((s[:1], lab[:1], ua[:1], ub[:1], ones), {}, "T=1"),
                            ((s, lab, ua, ub, ones), dict(costs=[(0.01, 1, 1)] * 9), "P <= 8"),
                            ((s, lab, ua, ub, ones), dict(act_costs=[(0.01, 1, 1)] * 9), "P <= 8"),
                            ((s, lab, ua, ub, ones), dict(costs=[(1.0, 1, 1)]), "p_target"),
                            ((s, lab, ua, ub, ones), dict(backend="cuda"), "backend")):
        with pytest.raises(ValueError, match=words):
            B.bootstrap_replicates(*args, **kw)
    # max(counts)^2 * T must stay below 2^53: 65 535^2 * T reaches it at T = 2 097 217
    T = 2097217
    assert 65535 ** 2 * (T - 1) < 2 ** 53 <= 65535 ** 2 * T
    s2, lab2, u2 = np.zeros(T), np.arange(T) % 2, np.zeros(T, dtype=np.int32)
    with pytest.raises(ValueError, match="2\\^53"):
        B.bootstrap_replicates(s2, lab2, u2, u2, np.array([[65535]]))
    with pytest.raises(ValueError, match="alpha"):
        B.bootstrap_report(s, lab, ua, ub, counts=ones, alpha=1.0)


def test_score_and_report_gains_ci(B, S):
    vecs = S.read_embeddings(os.path.join(GOLD, "test.iv"))
    from pytorch_kaldi_resnet_amd import kaldi_io
    mean = kaldi_io.read_vec_flt(os.path.join(GOLD, "mean.vec"))
    trials = os.path.join(GOLD, "trials")
    plain = S.score_and_report(vecs, vecs, trials, mean)
    assert "ci" not in plain
    m = {u: u.split("-")[0] for u in vecs}
    rep = S.score_and_report(vecs, vecs, trials, mean, bootstrap=dict(replicates=50, seed=1, utt2spk=m, max_degenerate=1.0))
    ci = rep.pop("ci")
    assert rep == plain
    pairs = [tuple(l.split()[:2]) for l in open(trials)]
    scores, labels = S.cosine_score(vecs, vecs, trials, mean)
    ua, ub, names = B.trial_units(pairs, m)
    want = B.bootstrap_report(scores.astype(np.float64), labels, ua, ub, replicates=50, seed=1, max_degenerate=1.0, units=len(names))
    assert ci["eer"] == want["eer"] and ci["min_dcf"] == want["min_dcf"] and ci["act_dcf"] == [] and ci["units"] == len(names)
    assert ci["eer"]["value"] == plain["eer"] and ci["eer"]["lo"] <= ci["eer"]["hi"] and "values" not in ci


# ---- the script and test.sh ---------------------------------------------------------------------------------------------------------
def run(script, *flags, env=None):
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT
    e.pop("SPK_BOOTSTRAP", None)
    e.pop("SPK_BOOTSTRAP_UTT2SPK", None)
    e.update(env or {})
    cmd = ["bash", os.path.join(ROOT, script)] if script.endswith(".sh") else [sys.executable, os.path.join(ROOT, "scripts", script)]
    return subprocess.run(cmd + list(flags), env=e, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the golden scores and trials, a second system in another line order, and the speaker of every trial id"""
    d = tmp_path_factory.mktemp("boot_cli")
    lines = open(os.path.join(GOLD, "scores_snorm")).read().splitlines()
    order = np.random.RandomState(4).permutation(len(lines))
    (d / "scores_b").write_text("\n".join(lines[t] for t in order) + "\n")
    ids = sorted({u for l in lines for u in l.split()[:2]})
    (d / "utt2spk").write_text("".join("%s %s\n" % (u, u.split("-")[0]) for u in ids))
    # two speakers, targets inside a speaker and non-targets across: a replicate that draws one speaker twice has no non-target
    utts = ["%s%d" % (spk, k) for spk in "ab" for k in range(3)]
    two = [(x, y) for i, x in enumerate(utts) for y in utts[i + 1:]]
    (d / "two_scores").write_text("".join("%s %s %r\n" % (x, y, 0.25 * i - (x[0] != y[0])) for i, (x, y) in enumerate(two)))
    (d / "two_trials").write_text("".join("%s %s %s\n" % (x, y, "target" if x[0] == y[0] else "nontarget") for x, y in two))
    (d / "two_utt2spk").write_text("".join("%s %s\n" % (u, u[0]) for u in utts))
    (d / "utt2spk_short").write_text("".join("%s %s\n" % (u, u.split("-")[0]) for u in ids[1:]))
    return d, os.path.join(GOLD, "scores"), os.path.join(GOLD, "trials"), ids


def test_script_lines_and_replicates_file(B, files):
    from pytorch_kaldi_resnet_amd import calibration
    d, scores, trials, ids = files
    flags = ["--utt2spk", str(d / "utt2spk"), "--replicates", "60", "--seed", "5", "--max-degenerate", "1"]
    r = run("bootstrap_ci.py", *flags, "--llr", "--p-target", "0.01", "--p-target", "0.5", "--write-replicates", str(d / "reps"), scores, trials)
    assert r.returncode == 0, r.stderr[-2000:]
    pairs, cols = calibration.read_score_files([scores])
    lab = calibration.trial_labels(pairs, trials)
    ua, ub, names = B.trial_units(pairs, str(d / "utt2spk"))
    costs = [(0.01, 1.0, 1.0), (0.5, 1.0, 1.0)]
    want = B.bootstrap_report(cols[0], lab, ua, ub, costs, costs, replicates=60, seed=5, max_degenerate=1.0, units=len(names))
    lines = r.stdout.splitlines()
    assert lines == B.report_lines(want)
    assert [l.split(":")[0] for l in lines] == ["EER", "minDCF(p-target=0.01)", "minDCF(p-target=0.5)", "actDCF(p-target=0.01)",
                                                "actDCF(p-target=0.5)", "degenerate replicates"]
    e = want["eer"]
    assert lines[0] == "EER: %.4f%% [%.4f, %.4f]" % (100 * e["value"], 100 * e["lo"], 100 * e["hi"])
    e = want["min_dcf"][0]
    assert lines[1] == "minDCF(p-target=0.01): %.4f [%.4f, %.4f]" % (e["value"], e["lo"], e["hi"])
    assert lines[5].startswith("degenerate replicates: %d of 60 (%d units" % (want["degenerate"], len(names)))
    rows = [l.split() for l in open(str(d / "reps")) if not l.startswith("#")]
    assert len(rows) == 60 and [int(w[0]) for w in rows] == want["values"]["i"][:, 0].tolist()
    got = np.array([[float(v) for v in w[3:]] for w in rows])
    assert got.shape == (60, 5) and got.tobytes() == want["values"]["d"].tobytes()
    # two systems: the difference lines, the second file in another line order
    r = run("bootstrap_ci.py", *flags, "--scores-b", str(d / "scores_b"), scores, trials)
    assert r.returncode == 0, r.stderr[-2000:]
    _, cols_b = calibration.read_score_files([os.path.join(GOLD, "scores_snorm")])
    both = B.bootstrap_compare(cols[0], cols_b[0], lab, ua, ub, replicates=60, seed=5, max_degenerate=1.0, units=len(names))
    assert r.stdout.splitlines() == B.report_lines(both["a"], both["diff"])
    assert [l.split(":")[0] for l in r.stdout.splitlines()[4:]] == ["EER(A-B)", "minDCF(A-B, p-target=0.01)", "minDCF(A-B, p-target=0.001)"]
    assert all(" P(<0)=" in l for l in r.stdout.splitlines()[4:])
    # without a map every id is its own unit
    r = run("bootstrap_ci.py", "--replicates", "20", scores, trials)
    assert r.returncode == 0 and ("(%d units" % len(ids)) in r.stdout.splitlines()[-1], r.stderr[-2000:]


def test_script_errors(files, tmp_path):
    d, scores, trials, ids = files
    lines = open(os.path.join(GOLD, "scores")).read().splitlines()
    (tmp_path / "short").write_text("\n".join(lines[:-1]) + "\n")
    for flags, words in ((["--utt2spk", str(d / "utt2spk_short"), scores, trials], [ids[0], "not assigned to any speaker"]),
                         (["--utt2spk", str(d / "nowhere"), scores, trials], ["nowhere"]),
                         (["--replicates", "1", scores, trials], ["--replicates"]),
                         (["--p-target", "1.5", scores, trials], ["p_target"]),
                         (["--alpha", "0", "--replicates", "10", scores, trials], ["alpha"]),
                         (["--scores-b", str(tmp_path / "short"), "--replicates", "10", scores, trials], ["is missing from the second"]),
                         (["--utt2spk", str(d / "two_utt2spk"), "--replicates", "50", str(d / "two_scores"), str(d / "two_trials")], ["degenerate"]),
                         ([scores, str(d / "nowhere")], ["nowhere"])):
        r = run("bootstrap_ci.py", *flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and "Traceback" not in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    r = run("bootstrap_ci.py", "--backend", "cuda", scores, trials)
    assert r.returncode == 2 and "--backend" in r.stderr
    # the same two-speaker files pass once the share is allowed, and say how many replicates were left out
    r = run("bootstrap_ci.py", "--utt2spk", str(d / "two_utt2spk"), "--replicates", "50", "--max-degenerate", "1", str(d / "two_scores"),
            str(d / "two_trials"))
    assert r.returncode == 0 and re.search(r"degenerate replicates: (1[5-9]|2\d|3[0-5]) of 50 \(2 units", r.stdout), r.stdout + r.stderr


def test_test_sh_hook(B, files, tmp_path):
    """without SPK_BOOTSTRAP every file is what it was and no _ci file appears; with it stage 13 adds <report>_ci"""
    d, scores, trials, ids = files
    outs = {}
    for name, env in (("plain", {}), ("ci", {"SPK_BOOTSTRAP": "40"}),
                      ("spk", {"SPK_BOOTSTRAP": "40", "SPK_BOOTSTRAP_UTT2SPK": str(d / "utt2spk")}),
                      ("short", {"SPK_BOOTSTRAP": "40", "SPK_BOOTSTRAP_UTT2SPK": str(d / "utt2spk_short")})):
        w = tmp_path / name
        w.mkdir()
        for f in ("mean.vec", "test.iv", "trials"):
            shutil.copy(os.path.join(GOLD, f), str(w / f))
        r = run("test.sh", str(w), str(w), "cosine", "12", str(w / "trials"), env=env)
        outs[name] = (r, {f: open(str(w / f), "rb").read() for f in sorted(os.listdir(str(w))) if os.path.isfile(str(w / f))})
    r, plain = outs["plain"]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(plain) == ["eer_cosine", "mean.vec", "scores_cosine", "test.iv", "trials"]
    assert plain["eer_cosine"] == open(os.path.join(GOLD, "eer_cosine"), "rb").read()
    r, ci = outs["ci"]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(set(ci) - set(plain)) == ["eer_cosine_ci"] and all(ci[f] == plain[f] for f in plain)
    assert r.stdout == outs["plain"][0].stdout + ci["eer_cosine_ci"].decode()
    want = run("bootstrap_ci.py", "--replicates", "40", str(tmp_path / "ci" / "scores_cosine"), trials)
    assert want.returncode == 0 and ci["eer_cosine_ci"].decode() == want.stdout and want.stdout.startswith("EER: ")
    r, spk = outs["spk"]
    assert r.returncode == 0 and "(4 units" in spk["eer_cosine_ci"].decode() and spk["eer_cosine_ci"] != ci["eer_cosine_ci"]
    # an id without a speaker: the script refuses and test.sh stops with its status
    r, short = outs["short"]
    assert r.returncode == 2 and all(short[f] == plain[f] for f in plain)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ["spkb_limit", "spkb_pitch", "spkb_group", "spkb_pack", "spkb_sweep_ws_elems", "spkb_sweep"]


def test_exports_are_declared_bound_and_exported():
    """the bootstrap entries have a header of their own, include/spkboot.h, a binding table of their own and a prefix of their own:
    every name the header declares is bound with as many parameters and exported, none is an spk_* or spkw_* name, and the other four
    tables count what they counted"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spkboot.h")).read(), flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|long long)\s+([a-z][a-z0-9_]*)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(decl) == sorted(NEW) == sorted(hip.boot_symbols()) == sorted(hip._BOOT_SIGS)
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    others = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("spkhip.h", "spkder.h", "spkcal.h", "spkwav.h"))
    for name in NEW:
        assert name.startswith("spkb_") and not re.match(r"spk_[a-z0-9_]+$|spkw_", name), name
        assert hasattr(hip.lib(), name) and re.search(r" T %s$" % name, nm, re.M), name
        params = [p for p in decl[name][1].split(",") if p.strip() != "void"]
        assert len(params) == len(hip._BOOT_SIGS[name]), name
        assert (decl[name][0] == "long long") == (getattr(hip.lib(), name).restype is ctypes.c_longlong), name
        assert name not in hip.exported_symbols() + hip.der_symbols() + hip.cal_symbols() + hip.wav_symbols(), name
        assert not re.search(r"\b%s\b" % name, others), name
    assert set(re.findall(r" T (spkb_[a-z0-9_]+)$", nm, re.M)) == set(NEW)
    assert (len(hip.exported_symbols()), len(hip.der_symbols()), len(hip.cal_symbols()), len(hip.wav_symbols())) == (128, 7, 9, 2)
    assert set(re.findall(r" T (spk_[a-z0-9_]+)$", nm, re.M)) == set(hip.exported_symbols()) | set(hip.der_symbols()) | set(hip.cal_symbols())
    assert set(re.findall(r" T (spkw_[a-z0-9_]+)$", nm, re.M)) == set(hip.wav_symbols())
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "include/spkboot.h" in readme and "(128 exports)" in readme


def test_limits_and_group_sizes():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    tile, max_u, max_c, max_p, max_g, threads = (lib.spkb_limit(i) for i in range(6))
    assert (max_u, max_c, max_p) == (65535, 65535, 8) and tile % threads == 0 and threads % 64 == 0 and lib.spkb_limit(6) < 0
    assert lib.spkb_group(1) == max_g >= 2 and lib.spkb_group(1251) == max_g and lib.spkb_group(65535) == 1
    assert lib.spkb_group(0) < 0 and lib.spkb_group(65536) < 0 and lib.spkb_pitch(0) < 0 and lib.spkb_pitch(65536) < 0
    last = max_g
    for U in range(1, 65536):
        g, pitch = lib.spkb_group(U), lib.spkb_pitch(U)
        assert pitch >= U and pitch % 8 == 0 and pitch - U < 8 and 1 <= g <= last
        assert g == 1 or 2 * g * pitch <= 65536                  # two workgroups' rows fit the 160 KiB of a CU beside the scratch
        assert 2 * g * pitch <= 131072
        last = g
    nb = lambda T: -(-T // tile)                                                         # noqa: E731
    for T, P, Pa, Rc in ((2, 0, 0, 1), (tile, 2, 2, 16), (tile + 1, 8, 8, 5), (10 ** 7, 2, 2, 112)):
        assert lib.spkb_sweep_ws_elems(T, P, Pa, Rc) == Rc * (2 * (nb(T) + 1) + 4 * (1 + P) * nb(T) + 2 * Pa)
    for bad in ((1, 0, 0, 1), (2, 9, 0, 1), (2, 0, 9, 1), (2, -1, 0, 1), (2, 0, 0, 0)):
        assert lib.spkb_sweep_ws_elems(*bad) < 0


def test_calls_are_refused_on_the_host_before_any_launch():
    """no device is needed: a refused call launches nothing and touches no pointer"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    lib, D = hip.lib(), 4096
    eta, costs = np.array([0.0, 1.0]), np.array([0.01, 1.0, 1.0, 0.001, 1.0, 1.0])

    def refused(rc, name, words=""):
        assert rc < 0 and name.encode() in lib.spk_last_error() and words.encode() in lib.spk_last_error(), (name, rc, lib.spk_last_error())

    def pack(T=10, U=5, P=2, null=None, e=eta.ctypes.data):
        p = [None if i == null else D for i in range(7)]
        return lib.spkb_pack(p[0], p[1], p[2], p[3], p[4], e, P, p[5], p[6], T, U, None)
    for kw in (dict(T=1), dict(T=0), dict(T=-3), dict(U=0), dict(U=65536), dict(P=9), dict(P=-1), dict(e=None), dict(null=6)) + tuple(
            dict(null=i) for i in range(6)):
        refused(pack(**kw), "spkb_pack")
    nan = np.array([0.0, np.nan])
    refused(pack(e=nan.ctypes.data), "spkb_pack", "NaN")

    def sweep(T=10, U=5, Rc=3, cmax=5, P=2, Pa=2, ws=1 << 24, null=None, c=costs.ctypes.data, a=costs.ctypes.data, counts=D, q=D):
        p = [None if i == null else D for i in range(4)]
        return lib.spkb_sweep(p[0], counts, U, Rc, cmax, c, P, a, q, Pa, p[1], p[2], p[3], ws, T, 0, None)
    need = lib.spkb_sweep_ws_elems(10, 2, 2, 3)
    bad_costs = np.array([0.01, 1.0, 1.0, 1.0, 1.0, 1.0])
    for kw in (dict(T=1), dict(U=0), dict(U=65536), dict(Rc=0), dict(Rc=65535 * lib.spkb_group(5) + 1), dict(cmax=65536), dict(cmax=-1),
               dict(P=9), dict(Pa=9), dict(P=-1), dict(c=None), dict(a=None), dict(q=None), dict(counts=None), dict(counts=D + 8),
               dict(ws=need - 1), dict(c=bad_costs.ctypes.data), dict(a=bad_costs.ctypes.data)) + tuple(dict(null=i) for i in range(4)):
        refused(sweep(**kw), "spkb_sweep")
    refused(sweep(T=2097217, cmax=65535, ws=1 << 40), "spkb_sweep", "2^53")
    refused(sweep(T=1 << 30, cmax=2897, ws=1 << 40), "spkb_sweep", "2^53")              # 2897^2 * 2^30 >= 2^53 > 2896^2 * 2^30
