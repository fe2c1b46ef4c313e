"""Diarization back end, host side: tests/diar_ref.py against scipy where it imports, the host back ends of
diarize.score_dense and diarize.cluster against diar_ref, make_rttm on hand-written cases, the errors of scripts/diarize.py and the
exports of csrc/diar.hip in the C ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 3, 17, 64, 65, 130, 257]


@pytest.fixture(scope="module")
def diarize():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


# ---- the reference against scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_ref_matches_scipy(n):
    hier = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    x, planted, S = R.planted(n, 3, seed=n)
    d = squareform(-S.astype(np.float64), checks=False)
    Z = hier.linkage(d, "average")
    labels, merges, costs = R.ahc_ref(S, 1)
    assert len(merges) == n - 1 and np.all(np.diff(costs) >= 0)               # average linkage on a metric: no inversions here
    assert np.allclose(costs, Z[:, 2], rtol=1e-12, atol=0)
    for k in (1, 2, 3):
        if k <= n:
            got, _, _ = R.ahc_ref(S, k)
            assert R.same_partition(got, hier.fcluster(Z, k, "maxclust")), (n, k)
    if n >= 3:
        t = 0.5 * (costs[-2] + costs[-1])                                      # between the last two merge costs
        got, _, cs = R.ahc_ref(S, 1, threshold=-t)
        assert len(cs) == n - 2 and R.same_partition(got, hier.fcluster(Z, t, "distance")), n
    if n >= 17:
        assert (R.ahc_ref(S, 3)[0] == planted).all()


# ---- host back ends against the reference ----------------------------------------------------------------------------------------
def _tie_matrix(n, seed):
    s = np.random.RandomState(seed).randint(-2, 3, size=(n, n)).astype(np.float32)
    return np.triu(s, 1) + np.triu(s, 1).T


def _line_matrix(n):
    p = 1.01 ** np.arange(n)
    return (-np.abs(p[:, None] - p[None, :])).astype(np.float32)


def _flat(mats):
    rec_off = np.concatenate([[0], np.cumsum([m.shape[0] for m in mats])]).astype(np.int64)
    return np.concatenate([m.ravel() for m in mats]).astype(np.float32), rec_off


def check_cluster(got, mats, rec_off, minc, thr):
    labels, merges, cost, nm = got
    for r, S in enumerate(mats):
        lab, mer, cs = R.ahc_ref(S, minc[r], None if thr[r] == -np.inf else thr[r])
        lo = int(rec_off[r])
        assert nm[r] == len(mer), (r, nm[r], len(mer))
        assert merges[lo:lo + len(mer)].tolist() == [list(p) for p in mer], r
        assert cost[lo:lo + len(mer)].view(np.int64).tolist() == np.array(cs, dtype=np.float64).view(np.int64).tolist(), r
        assert labels[lo:lo + S.shape[0]].tolist() == lab.tolist(), r


def test_host_cluster_matches_the_reference(diarize):
    mats = [R.planted(n, 3, seed=n)[2] for n in [1] + SIZES[:-1]] + [_tie_matrix(65, 1), _line_matrix(130), _tie_matrix(9, 2)]
    scores, rec_off = _flat(mats)
    Rn = len(mats)
    for minc, thr in [(np.ones(Rn, int), np.full(Rn, -np.inf)), (np.full(Rn, 2), np.full(Rn, -np.inf)),
                      (np.full(Rn, 10 ** 6), np.full(Rn, -np.inf)), (np.ones(Rn, int), np.full(Rn, -1.5)),
                      (np.full(Rn, 3), np.full(Rn, -40.0)), (np.ones(Rn, int), np.full(Rn, 1e9))]:
        got = diarize.cluster(scores, rec_off, threshold=thr, num_speakers=minc, backend="host")
        check_cluster(got, mats, rec_off, minc, thr)
    labels = diarize.cluster(scores, rec_off, num_speakers=3)[0]
    for r, n in enumerate([1] + SIZES[:-1]):
        if n >= 17:
            assert (labels[rec_off[r]:rec_off[r + 1]] == R.planted(n, 3, seed=n)[1]).all()


def test_host_cluster_ignores_nan_and_refuses_bad_arguments(diarize):
    S = R.planted(6, 2, seed=4)[2].copy()
    S[0, 1] = S[1, 0] = np.nan
    got = diarize.cluster(S.ravel(), [0, 6], backend="host")
    check_cluster(got, [S], [0, 6], [1], [-np.inf])
    assert got[3][0] < 5                                                # the NaN pair can never merge: the loop ends early
    for bad in ([1, 6], [0, 0, 6], [0, 7, 6]):
        with pytest.raises(ValueError):
            diarize.cluster(S.ravel(), bad)
    with pytest.raises(ValueError):
        diarize.cluster(S.ravel(), [0, 6], num_speakers=0)


@pytest.mark.parametrize("D", [1, 5, 24])
def test_host_score_dense_matches_the_reference(diarize, D):
    rng = np.random.RandomState(D)
    ns = [1, 17, 2, 33]
    rec_off = np.concatenate([[0], np.cumsum(ns)])
    L = max(1, D - 2)
    emb = rng.randn(rec_off[-1], D).astype(np.float32)
    transform = rng.randn(L, D + 1)
    psi = np.abs(rng.randn(L)) * 3
    psi[0] = 0.0
    model = (rng.randn(L) * 0.1, np.eye(L) + 0.1 * rng.randn(L, L), psi)
    mean = rng.randn(D) * 0.1
    for kind, extra in [("cosine", {}), ("plda", dict(transform=transform, plda=model, smoothing=0.1))]:
        U, q, g, K = diarize.dense_inputs(emb, kind, mean=mean, backend="host", **extra)
        got, mat_off = diarize.score_dense(emb, rec_off, kind, mean=mean, backend="host", **extra)
        assert got.dtype == np.float32 and mat_off.tolist() == np.concatenate([[0], np.cumsum(np.square(ns))]).tolist()
        for r, n in enumerate(ns):
            u, qq = U[rec_off[r]:rec_off[r + 1]], q[rec_off[r]:rec_off[r + 1]]
            ref, bound, _ = R.dense_ref(u, qq, g, K)
            s = got[mat_off[r]:mat_off[r + 1]].reshape(n, n)
            assert (np.abs(s.astype(R.LD) - ref) <= bound).all(), (kind, r)
            assert (s.view(np.int32) == s.T.view(np.int32)).all()
            if kind == "cosine":
                x = emb[rec_off[r]:rec_off[r + 1]].astype(np.float64) - mean.astype(np.float32)
                x = x.astype(np.float32).astype(np.float64)
                cos = (x @ x.T) / np.outer(np.linalg.norm(x, axis=1), np.linalg.norm(x, axis=1))
                assert np.allclose(s, cos, atol=1e-6)
    # the dense PLDA form is Plda::LogLikelihoodRatio(u_i, 1, u_j)
    U = rng.randn(7, L)
    g, k, K = R.plda_terms(psi)
    dense = (U * g) @ U.T + R.plda_q(U, k)[:, None] + R.plda_q(U, k)[None, :] + K
    assert np.allclose(dense, R.llr_direct(U, psi), rtol=1e-12, atol=1e-12)
    gg, kk, KK = diarize.plda_dense_terms(psi)
    assert np.array_equal(gg, g) and np.array_equal(kk, k) and KK == K


# ---- RTTM -------------------------------------------------------------------------------------------------------------------------
def test_rttm_overlap_is_cut_at_its_midpoint(diarize):
    seg = [("a", "rec", 0.0, 4.0), ("b", "rec", 3.0, 7.0)]
    assert diarize.make_rttm(seg, [1, 2]) == ["SPEAKER rec 0 0.000 3.500 <NA> <NA> 1 <NA> <NA>",
                                              "SPEAKER rec 0 3.500 3.500 <NA> <NA> 2 <NA> <NA>"]
    assert diarize.make_rttm(seg, {"b": 2, "a": 1}, channel=1)[0].startswith("SPEAKER rec 1 0.000 3.500")


def test_rttm_three_windows_of_one_label_are_merged(diarize):
    seg = [("a", "rec", 0.0, 2.0), ("b", "rec", 1.0, 3.0), ("c", "rec", 3.0, 5.0), ("d", "rec", 5.5, 6.0)]
    assert diarize.make_rttm(seg, [4, 4, 4, 4]) == ["SPEAKER rec 0 0.000 5.000 <NA> <NA> 4 <NA> <NA>",
                                                    "SPEAKER rec 0 5.500 0.500 <NA> <NA> 4 <NA> <NA>"]


def test_rttm_a_swallowed_window_is_dropped(diarize):
    seg = [("a", "rec", 0.0, 4.0), ("b", "rec", 1.0, 3.0), ("c", "rec", 2.0, 6.0)]
    lines = diarize.make_rttm(seg, [1, 2, 1])
    assert lines == R.rttm_ref(seg, [1, 2, 1])
    assert lines == ["SPEAKER rec 0 0.000 2.500 <NA> <NA> 1 <NA> <NA>", "SPEAKER rec 0 2.500 3.500 <NA> <NA> 1 <NA> <NA>"]


def test_rttm_two_recordings_interleaved(diarize):
    seg = [("x1", "x", 2.0, 4.0), ("y0", "y", 0.0, 1.0), ("x0", "x", 0.0, 2.5), ("y1", "y", 0.5, 1.5)]
    lab = [2, 1, 1, 1]
    lines = diarize.make_rttm(seg, lab)
    assert lines == R.rttm_ref(seg, lab)
    assert lines == ["SPEAKER x 0 0.000 2.250 <NA> <NA> 1 <NA> <NA>", "SPEAKER x 0 2.250 1.750 <NA> <NA> 2 <NA> <NA>",
                     "SPEAKER y 0 0.000 1.500 <NA> <NA> 1 <NA> <NA>"]


def test_rttm_random_cases_match_the_reference(diarize):
    rng = np.random.RandomState(0)
    for _ in range(20):
        seg, lab = [], []
        for reco in ("r0", "r1", "r2"):
            for w in range(rng.randint(1, 12)):
                s = w * 0.5 + rng.randint(0, 3) * 0.25
                seg.append(("%s-%d" % (reco, w), reco, s, s + 0.25 * rng.randint(1, 8)))
                lab.append(int(rng.randint(1, 4)))
        order = rng.permutation(len(seg))
        seg, lab = [seg[i] for i in order], [lab[i] for i in order]
        assert diarize.make_rttm(seg, lab) == R.rttm_ref(seg, lab)


# ---- scripts/diarize.py -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def script_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("diarize_cli")
    rng = np.random.RandomState(5)
    keys, lines = [], []
    for reco, n in (("recA", 6), ("recB", 4)):
        for w in range(n):
            k = "%s-%08d-%08d" % (reco, 20 * w, 20 * w + 40)
            keys.append(k)
            lines.append("%s %s %.3f %.3f\n" % (k, reco, 0.2 * w, 0.2 * w + 0.4))
    centres = rng.randn(2, 16) * 4
    vec = {k: centres[i % 2] + 0.1 * rng.randn(16) for i, k in enumerate(keys)}

    def write(name, ks):
        with open(str(d / name), "w") as f:
            for k in ks:
                f.write(k + " [ " + " ".join("%.6f" % v for v in vec[k]) + " ]\n")
        return str(d / name)

    def text(name, body):
        with open(str(d / name), "w") as f:
            f.write(body)
        return str(d / name)

    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def run(*flags):
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "diarize.py")] + list(flags)
        return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)

    return {"dir": d, "emb": write("emb", keys), "emb_short": write("emb_short", keys[:-1]), "keys": keys,
            "seg": text("segments", "".join(lines)), "seg_short": text("segments_short", "".join(lines[1:])),
            "num": text("reco2num", "recA 2\nrecB 2\n"), "num_extra": text("reco2num_extra", "recA 2\nrecB 2\nrecC 1\n"),
            "recs": text("recordings", "recA\nrecB\nrecD\n"), "run": run}


def test_script_host_run(script_case):
    c = script_case
    out = str(c["dir"] / "out")
    r = c["run"]("--embeddings", c["emb"], "--segments", c["seg"], "--reco2num-spk", c["num"], "--out-dir", out, "--write-scores")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lab = dict(l.split() for l in open(os.path.join(out, "labels")))
    assert sorted(lab) == sorted(c["keys"])
    assert [lab[k] for k in c["keys"]] == ["1", "2"] * 5                 # the two planted centres alternate
    assert np.loadtxt(os.path.join(out, "scores.recA")).shape == (6, 6)
    rttm = R.parse_rttm(open(os.path.join(out, "rttm")).read().splitlines())
    assert sorted(rttm) == ["recA", "recB"]
    r = c["run"]("--embeddings", c["emb"], "--segments", c["seg"], "--threshold", "0.0", "--out-dir", out + "_t")
    assert r.returncode == 0, r.stderr[-2000:]
    assert dict(l.split() for l in open(os.path.join(out + "_t", "labels"))) == lab


def test_script_errors(script_case):
    c = script_case
    base = ["--embeddings", c["emb"], "--segments", c["seg"], "--out-dir", str(c["dir"] / "never")]
    cases = [
        (base, ["--threshold", "--reco2num-spk"]),
        (base + ["--threshold", "0", "--reco2num-spk", c["num"]], ["--threshold", "--reco2num-spk"]),
        (base + ["--threshold", "0", "--backend-score", "plda"], ["--plda", "--transform"]),
        (["--embeddings", c["emb_short"], "--segments", c["seg"], "--out-dir", "x", "--threshold", "0"],
         ["without an embedding", c["keys"][-1]]),
        (["--embeddings", c["emb"], "--segments", c["seg_short"], "--out-dir", "x", "--threshold", "0"],
         ["without a line in the segments file", c["keys"][0]]),
        (base + ["--reco2num-spk", c["num_extra"]], ["absent", "recC"]),
        (base + ["--threshold", "0", "--recordings", c["recs"]], ["no window", "recD"]),
    ]
    for flags, words in cases:
        r = c["run"](*flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    assert not os.path.exists(str(c["dir"] / "never"))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NEW = ["spk_diar_tables", "spk_score_dense_q", "spk_score_dense", "spk_ahc_threads", "spk_ahc_max_n", "spk_ahc_batch"]


def test_exports_are_declared_bound_and_exported():
    from helpers import header_params
    from pytorch_kaldi_resnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        params = [p for p in header_params(name) if p != "void"]
        assert len(params) == len(hip._SIGS[name]), name


def test_batches_are_refused_on_the_host_before_any_launch():
    """the argument checks need no device: with every device pointer NULL a good batch gets as far as the pointer check"""
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    assert lib.spk_ahc_max_n() >= 8192 and lib.spk_ahc_threads() % 64 == 0

    def dense(rec_off, Ntot, D=4):
        ro = np.asarray(rec_off, dtype=np.int64)
        rc = lib.spk_score_dense(None, ro.ctypes.data, None, None, None, 0.0, None, Ntot, D, len(rec_off) - 1, None)
        return rc, lib.spk_last_error().decode()

    def ahc(rec_off, Ntot, ws_elems):
        ro = np.asarray(rec_off, dtype=np.int64)
        rc = lib.spk_ahc_batch(None, ro.ctypes.data, None, None, None, None, ws_elems, None, None, None, None, Ntot, len(rec_off) - 1,
                               None)
        return rc, lib.spk_last_error().decode()

    for ro, N, word in [([1, 5], 5, "rec_off"), ([0, 2, 2, 5], 5, "empty"), ([0, 3, 2, 5], 5, "empty"), ([0, 2, 4], 5, "rec_off"),
                        ([0, 46341], 46341, "2^31"), ([0, 40000, 80000], 80000, "2^31")]:
        for rc, msg in (dense(ro, N), ahc(ro, N, 1 << 40)):
            assert rc < 0 and word in msg, (ro, msg)
    for D in (0, 513):
        rc, msg = dense([0, 5], 5, D)
        assert rc < 0 and "D=" in msg
    rc, msg = dense([0, 1, 18], 18)
    assert rc < 0 and "null device pointer" in msg
    rc, msg = ahc([0, 8193], 8193, 1 << 40)
    assert rc < 0 and "cap" in msg
    rc, msg = ahc([0, 3, 8], 8, 33)
    assert rc < 0 and "workspace" in msg
    rc, msg = ahc([0, 3, 8], 8, 34)
    assert rc < 0 and "null device pointer" in msg
    tab = np.zeros((3, 4), dtype=np.int64)
    ro = np.array([0, 1, 18, 50], dtype=np.int64)
    assert lib.spk_diar_tables(ro.ctypes.data, 3, 50, tab.ctypes.data) == 0
    assert tab.tolist() == [[0, 1, 18, 50], [0, 1, 290, 1314], [0, 1, 4, 7]]
