"""Speaker-level bootstrap of the error-rate sweep on the device (csrc/boot.hip): the `hip` back end against the
host back end on every double and every integer of every replicate.  Every comparison is bit equality.  The shapes sit on the edges the
library exports: the tile (positions per workgroup), the replicates per workgroup G(U) and the chunk of replicates per launch."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "backend")
COSTS = [(0.01, 1.0, 1.0), (0.05, 10.0, 2.0)]
ACT = [(0.5, 1.0, 1.0), (0.3, 1.0, 2.0)]
EIGHT = [(p, 1.0, 1.0) for p in (0.5, 0.3, 0.1, 0.05, 0.01, 0.005, 0.001, 0.0001)]


@pytest.fixture(scope="module")
def B():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import bootstrap
    return bootstrap


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


def tied_case(T, U, seed, zero_unit=None, tile=None):
    """scores of a few values (minima tie across threads and tiles), already sorted with +0.0 and -0.0 among them, so a position of
    the sorted list is an index here; with zero_unit: the trials that open the list, straddle the first tile boundary and close the
    list are same-unit trials of that unit, so a row with count 0 there gives runs of weight 0 at those places"""
    rng = np.random.RandomState(seed)
    s = np.sort(rng.randint(-3, 4, size=T) / 2.0)
    s[s == 0.0] = np.where(rng.rand(int((s == 0.0).sum())) < 0.5, -0.0, 0.0)
    lab = (rng.rand(T) < 0.4).astype(np.uint8)
    top = U if zero_unit is None else U - 1                      # (the zero unit is the last one; no other trial touches it)
    ua, ub = rng.randint(0, max(top, 1), size=T).astype(np.int32), rng.randint(0, max(top, 1), size=T).astype(np.int32)
    same = rng.rand(T) < 0.3
    ub[same] = ua[same]
    if zero_unit is not None:
        runs = [(0, min(5, T - 2)), (T - min(4, T - 2), T)]
        if tile is not None and T > tile + 4:
            runs.append((tile - 3, tile + 4))
        for lo, hi in runs:
            ua[lo:hi] = ub[lo:hi] = zero_unit
    free = np.flatnonzero(ua != (-1 if zero_unit is None else zero_unit))
    if len(free) >= 2:
        lab[free[0]], lab[free[-1]] = 1, 0                       # both classes outside the zero runs
    else:
        lab[0], lab[-1] = 1, 0
    return s, lab, ua, ub


def assert_same(B, s, lab, ua, ub, counts, costs=COSTS, act=ACT, chunk=None):
    host = B.bootstrap_replicates(s, lab, ua, ub, counts, costs, act)
    dev = B.bootstrap_replicates(s, lab, ua, ub, counts, costs, act, backend="hip", chunk=chunk)
    assert dev["d"].shape == host["d"].shape and dev["i"].shape == host["i"].shape
    bad = np.flatnonzero((dev["i"] != host["i"]).any(1) | (dev["d"].view(np.int64) != host["d"].view(np.int64)).any(1))
    assert bad.size == 0, (bad[:5], dev["i"][bad[:2]], host["i"][bad[:2]], dev["d"][bad[:2]], host["d"][bad[:2]])
    return host, dev


def test_trials_at_the_tile_edges(B, ops):
    tile = ops.boot_sizes()[0]
    U = 7
    G = ops.boot_sizes(U)[0]
    for T in (2, tile - 1, tile, tile + 1, 3 * tile + 1):
        s, lab, ua, ub = tied_case(T, U, T, zero_unit=U - 1, tile=tile)
        counts = B.bootstrap_counts(U, G + 1, T)
        counts[::2, U - 1] = 0                                    # runs of weight 0 that open, close and straddle
        counts[1, :] = 1
        host, _ = assert_same(B, s, lab, ua, ub, counts)
        assert (~host["degenerate"]).sum() >= 2
        if T > 12:
            assert (host["eer_index"][0::2][~host["degenerate"][0::2]] >= 5).all()      # never inside the opening run of weight 0


def test_replicates_at_the_group_and_chunk_edges(B, ops):
    tile = ops.boot_sizes()[0]
    for U, T in ((7, tile + 1), (4000, 300)):
        G = ops.boot_sizes(U)[0]
        assert G >= 2
        s, lab, ua, ub = tied_case(T, U, U)
        table = B.bootstrap_counts(U, 2 * G + 1, 11)
        for n in (1, G - 1, G, G + 1):
            assert_same(B, s, lab, ua, ub, table[:n])
        assert_same(B, s, lab, ua, ub, table[:G + 1], chunk=G)              # one replicate past a chunk
        assert_same(B, s, lab, ua, ub, table, chunk=2 * G)
        assert_same(B, s, lab, ua, ub, table[:5], chunk=3)                  # chunks that are no whole groups


def test_units_at_the_edges(B, ops):
    tile, max_u = ops.boot_sizes()[:2]
    T = tile + 1
    # one unit: every trial is a same-unit trial; a count of 0 leaves nothing
    s, lab, ua, ub = tied_case(T, 1, 1)
    host, _ = assert_same(B, s, lab, ua, ub, np.array([[1], [0], [3], [0]]))
    assert host["degenerate"].tolist() == [False, True, False, True]
    host, _ = assert_same(B, s, lab, ua, ub, np.zeros((3, 1), dtype=np.int64))
    assert host["degenerate"].all()
    s, lab, ua, ub = tied_case(T, 2, 2)
    assert_same(B, s, lab, ua, ub, np.array([[1, 1], [2, 0], [0, 2], [1, 1]]))
    # the largest U of every group size and the one above it
    steps = [U for U in range(1, max_u) if ops.boot_sizes(U)[0] != ops.boot_sizes(U + 1)[0]]
    assert len(steps) == ops.boot_sizes(1)[0] - 1 and ops.boot_sizes(steps[-1] + 1)[0] == 1
    for U in [u for step in steps for u in (step, step + 1)] + [max_u]:
        G = ops.boot_sizes(U)[0]
        s, lab, ua, ub = tied_case(T, U, U)
        ua[:3], ub[:3] = (0, U - 1, U - 1), (U - 1, 0, U - 1)
        counts = B.bootstrap_counts(U, G + 1, U)
        counts[0, U - 1] = max(counts[0, U - 1], 2)
        assert_same(B, s, lab, ua, ub, counts, costs=COSTS[:1], act=ACT[:1])


def test_placement_does_not_matter(B, ops):
    tile = ops.boot_sizes()[0]
    U, T = 40, 2 * tile + 5
    G = ops.boot_sizes(U)[0]
    s, lab, ua, ub = tied_case(T, U, 5, zero_unit=U - 1, tile=tile)
    counts = B.bootstrap_counts(U, 2 * G + 3, 5)
    counts[3] = 0
    counts[3, 0] = U                                               # a degenerate row among the others
    host, dev = assert_same(B, s, lab, ua, ub, counts)
    again = B.bootstrap_replicates(s, lab, ua, ub, counts, COSTS, ACT, backend="hip")
    assert again["d"].tobytes() == dev["d"].tobytes() and again["i"].tobytes() == dev["i"].tobytes()
    perm = np.random.RandomState(1).permutation(counts.shape[0])
    moved = B.bootstrap_replicates(s, lab, ua, ub, counts[perm], COSTS, ACT, backend="hip", chunk=G + 1)
    assert moved["d"].tobytes() == dev["d"][perm].tobytes() and moved["i"].tobytes() == dev["i"][perm].tobytes()


def test_all_ones_row_is_the_existing_device_report(B, ops):
    import torch
    from pytorch_kaldi_resnet_amd import calibration
    tile = ops.boot_sizes()[0]
    U, T = 9, 2 * tile + 77
    s, lab, ua, ub = tied_case(T, U, 8)
    sd, ld = torch.from_numpy(s).cuda(), torch.from_numpy(lab).cuda()
    order = ops.sort_trials(sd)
    ones = np.ones((3, U), dtype=np.int64)
    # act costs whose Bayes thresholds lie below every score (q = 0), inside, and above every score (q = T)
    act = [(0.999, 1.0, 1.0), (0.5, 1.0, 1.0), (0.001, 1.0, 1.0)]
    assert calibration.bayes_threshold(*act[0]) < s.min() and calibration.bayes_threshold(*act[2]) > s.max()
    for costs, acts in (((), ()), (EIGHT, EIGHT), (COSTS, act)):
        P, Pa = len(costs), len(acts)
        rep = B.bootstrap_replicates(sd, lab, ua, ub, ones, costs, acts, backend="hip")
        out_d, out_i = ops.error_sweep(sd, ld, order, costs)
        d, i = out_d.cpu().numpy(), out_i.cpu().numpy()
        eta = [calibration.bayes_threshold(*c) for c in acts]
        cd, ci = (x.cpu().numpy() for x in ops.cal_cllr(sd, ld, acts, eta))
        for r in range(3):
            assert rep["eer"][r].tobytes() == d[0].tobytes() and rep["eer_index"][r] == i[0]
            assert (rep["n_target"][r], rep["n_nontarget"][r]) == (i[1], i[2]) == (ci[0], ci[1])
            assert rep["min_dcf"][r].tobytes() == d[1::2].tobytes() and rep["min_dcf_index"][r].tolist() == i[3:].tolist()
            assert rep["act_dcf"][r].tobytes() == cd[2:].tobytes()
            assert rep["miss"][r].tolist() == ci[2:2 + Pa].tolist() and rep["fa"][r].tolist() == ci[2 + Pa:].tolist()
        assert_same(B, s, lab, ua, ub, ones, costs, acts)
    assert rep["miss"][0, 0] == 0 and rep["fa"][0, 0] == T - lab.sum() and rep["miss"][0, 2] == lab.sum() and rep["fa"][0, 2] == 0


def test_counts_of_65535(B, ops):
    s, lab = np.array([0.5, -0.5]), np.array([1, 0])
    ua, ub = np.array([0, 0]), np.array([0, 1])
    counts = np.array([[65535, 65535], [65535, 1], [1, 65535], [65535, 0]])
    host, _ = assert_same(B, s, lab, ua, ub, counts)
    assert host["n_nontarget"].tolist() == [65535 ** 2, 65535, 65535, 0]
    T = 700                                                        # 65 535^2 * 700 < 2^53: sums far above 2^32
    s, lab, ua, ub = tied_case(T, 3, 3)
    counts = np.array([[65535, 65535, 65535], [65535, 1, 0], [1, 65535, 2], [0, 0, 65535]])
    host, _ = assert_same(B, s, lab, ua, ub, counts)
    assert host["n_target"][0] + host["n_nontarget"][0] > 2 ** 40
    with pytest.raises(ValueError, match="2\\^53"):
        B.bootstrap_replicates(np.zeros(2097217), np.arange(2097217) % 2, np.zeros(2097217, int), np.zeros(2097217, int),
                               np.array([[65535]]), backend="hip")


def test_report_and_script_are_the_hosts(B, tmp_path):
    from pytorch_kaldi_resnet_amd import calibration
    scores, trials = os.path.join(GOLD, "scores"), os.path.join(GOLD, "trials")
    pairs, cols = calibration.read_score_files([scores])
    lab = calibration.trial_labels(pairs, trials)
    ua, ub, names = B.trial_units(pairs, {u: u.split("-")[0] for p in pairs for u in p})
    kw = dict(costs=COSTS, act_costs=ACT, replicates=70, seed=2, max_degenerate=1.0, units=len(names))
    host, dev = B.bootstrap_report(cols[0], lab, ua, ub, **kw), B.bootstrap_report(cols[0], lab, ua, ub, backend="hip", **kw)
    assert host["values"]["d"].tobytes() == dev["values"]["d"].tobytes() and host["values"]["i"].tobytes() == dev["values"]["i"].tobytes()
    for key in ("eer", "min_dcf", "act_dcf", "degenerate", "replicates", "units"):
        assert host[key] == dev[key], key
    assert B.report_lines(host) == B.report_lines(dev)
    (tmp_path / "utt2spk").write_text("".join("%s %s\n" % (u, u.split("-")[0]) for u in sorted({u for p in pairs for u in p})))
    outs = []
    for backend in ("host", "hip"):
        env = dict(os.environ, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bootstrap_ci.py"), "--backend", backend, "--utt2spk",
                            str(tmp_path / "utt2spk"), "--replicates", "70", "--seed", "2", "--max-degenerate", "1", "--llr",
                            "--scores-b", os.path.join(GOLD, "scores_snorm"), "--write-replicates", str(tmp_path / backend), scores, trials],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append((r.stdout, open(str(tmp_path / backend), "rb").read()))
    assert outs[0] == outs[1] and outs[0][0].startswith("EER: ") and "EER(A-B): " in outs[0][0]
