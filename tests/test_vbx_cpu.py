"""VBx resegmentation, host side: the properties of tests/vbx_ref.py on planted data, the host back end of
diarize.vbx against the longdouble reference under the tolerance rule of section 6o, the initialisation and label rules, argument
errors, scripts/diarize.py --vbx on files and the exports of the VB-HMM in the C ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import vbx_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vbx")
GRID = [c + p for c in V.CASES for p in V.PARAMS]
SEPARATED = [c for c in V.CASES if c[0] >= 130]          # the cases in which VBx prunes the S states down to the K planted speakers


@pytest.fixture(scope="module")
def diarize():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


# ---- the reference's own properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,S,K,Fa,Fb,loopP", GRID)
def test_ref_properties(T, D, S, K, Fa, Fb, loopP):
    c = V.planted_case(T, D, S, K, Fa, Fb, loopP)
    y = c["y"]
    assert y.n_iters == 10 and y.same_length
    # S entries, each no further from the truth than the float64 run of the same restatement is from this longdouble run
    assert float(np.abs(y.gamma.sum(axis=1) - 1).max()) <= S * (y.e64["gamma"] + V.FLOOR)
    assert float(np.abs(y.pi.sum() - 1)) <= S * (y.e64["pi"] + V.FLOOR)
    steps = np.diff(y.elbo)
    assert (steps >= -1e-12 * np.abs(y.elbo[1:])).all(), steps.min()
    if (T, D, S, K) in SEPARATED:
        lab = V.labels_of(y.gamma)
        assert V.same_partition(lab, c["truth"]) and len(set(lab.tolist())) == K
        assert V.top_two_gap(y.gamma) >= 1e-3
    # the O(S) form of the recursions against the S x S form, both restated here, to the yardstick.  A float64 run in log space has
    # a rounding history of its own of the yardstick's size (the exponentials of sums of the size of lfw), so it is held to the
    # rule's ceiling for M, not to the M chosen for the product code
    g, p, e = V.vbx_ref(c["X"], c["Phi"], c["gamma0"], c["pi0"], Fa, Fb, loopP, 10, -np.inf, np.float64, linear=True)
    y.check(g, p, e, "ref O(S) form (%d,%d,%d,%d) Fa=%g" % (T, D, S, K, Fa), M=V.M_CEILING)


def test_ref_early_stopping_steps_are_far_from_epsilon():
    eps = V.EARLY["epsilon"]
    stops = []
    for c in V.early_cases():
        steps = np.diff(np.array(c["elbo"], dtype=np.float64))
        assert len(c["elbo"]) < V.EARLY["max_iters"] and steps[-1] < eps and (steps[:-1] >= eps).all()
        assert ((steps < eps / 100) | (steps > 100 * eps)).all(), steps
        stops.append(len(c["elbo"]))
    assert len(set(stops)) > 1, stops


# ---- the host back end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,S,K,Fa,Fb,loopP", GRID)
def test_host_matches_the_reference(diarize, T, D, S, K, Fa, Fb, loopP):
    c = V.planted_case(T, D, S, K, Fa, Fb, loopP)
    r = diarize.vbx(c["X"], c["Phi"], [0, T], gamma=c["gamma0"], pi=c["pi0"][None, :], Fa=Fa, Fb=Fb, loop_prob=loopP, max_iters=10,
                    epsilon=-np.inf, backend="host")
    assert r["n_iters"].tolist() == [10] and r["gamma"].shape == (T, S) and r["pi"].shape == (1, S)
    c["y"].check(r["gamma"], r["pi"][0], r["elbo"][0], "host (%d,%d,%d,%d) Fa=%g" % (T, D, S, K, Fa))
    if V.top_two_gap(c["y"].gamma) >= 1e-3:
        assert r["labels"].tolist() == V.labels_of(c["y"].gamma).tolist()


def test_host_batch_early_stopping_and_padding(diarize):
    cs = V.early_cases()
    Smax, E = 6, V.EARLY
    rec_off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in cs])])
    X = np.concatenate([c["X"] for c in cs])
    ns = [c["gamma0"].shape[1] for c in cs]
    gamma = np.full((len(X), Smax), np.nan)                                # columns at or beyond n_states are not read
    pi = np.full((len(cs), Smax), np.nan)
    for r, c in enumerate(cs):
        gamma[rec_off[r]:rec_off[r + 1], :ns[r]] = c["gamma0"]
        pi[r, :ns[r]] = c["pi0"]
    got = diarize.vbx(X, cs[0]["Phi"], rec_off, gamma=gamma, pi=pi, n_states=ns, Fa=E["Fa"], Fb=E["Fb"], loop_prob=E["loopP"],
                      max_iters=E["max_iters"], epsilon=E["epsilon"])
    assert got["n_iters"].tolist() == [len(c["elbo"]) for c in cs]
    assert np.isfinite(got["gamma"]).all() and np.isfinite(got["pi"]).all()
    for r, c in enumerate(cs):
        n = len(c["elbo"])
        assert np.isnan(got["elbo"][r, n:]).all() and not np.isnan(got["elbo"][r, :n]).any()
        assert (got["gamma"][rec_off[r]:rec_off[r + 1], ns[r]:] == 0).all() and (got["pi"][r, ns[r]:] == 0).all()
        assert c["y"].same_length
        c["y"].check(got["gamma"][rec_off[r]:rec_off[r + 1], :ns[r]], got["pi"][r, :ns[r]], got["elbo"][r, :n], "host early stop %d" % r)


def test_host_zero_prior_and_one_hot_start(diarize):
    T, D, S, K = 65, 5, 4, 3
    X, Phi, truth, first = V.planted(T, D, S, K, seed=3)
    hot = (first[:, None] == np.arange(S)[None, :]).astype(np.float64)
    hot[:, 3] = 0
    hot[hot.sum(axis=1) == 0, 0] = 1                                       # state 3 is empty: N_s = 0, invL = 1, alpha = 0
    pi0 = np.array([0.5, 0.0, 0.25, 0.25])
    y = V.Yardstick(X, Phi, hot, pi0, 0.3, 17.0, 0.99, 5, -np.inf)
    r = diarize.vbx(X, Phi, [0, T], gamma=hot, pi=pi0[None, :], max_iters=5, epsilon=-np.inf)
    assert np.isfinite(r["gamma"]).all() and np.isfinite(r["elbo"]).all()
    assert (r["gamma"][:, 1] == 0).all() and r["pi"][0, 1] == 0 and (np.asarray(y.gamma[:, 1], dtype=np.float64) == 0).all()
    y.check(r["gamma"], r["pi"][0], r["elbo"][0], "host zero prior")


# ---- initialisation, labels, arguments ----------------------------------------------------------------------------------------------
def test_initialisation_rule(diarize):
    lab = np.array([3, 3, 7, 3, 9, 2, 2, 2])
    gamma, pi, ns = diarize.vbx_init(lab, [0, 5, 8])
    assert ns.tolist() == [3, 1] and gamma.shape == (8, 3) and pi.tolist() == [[1 / 3] * 3, [1, 0, 0]]
    hi, lo = np.exp(7.0) / (np.exp(7.0) + 2), 1 / (np.exp(7.0) + 2)
    want = np.full((5, 3), lo)
    want[[0, 1, 3], 0] = hi                                                # label 3 is the smallest: state 0
    want[2, 1] = hi
    want[4, 2] = hi
    assert np.allclose(gamma[:5], want, rtol=1e-15, atol=0) and (gamma[5:] == [1, 0, 0]).all()
    g2 = diarize.vbx_init(lab, [0, 5, 8], init_smoothing=0.0)[0]
    assert np.allclose(g2[:5], 1 / 3)
    assert np.allclose(gamma[:5], V.init_gamma(np.array([0, 0, 1, 0, 2]), 3))


def test_label_rule(diarize):
    gamma = np.array([[0.2, 0.5, 0.3], [0.2, 0.5, 0.3], [0.4, 0.4, 0.2], [0.1, 0.1, 0.8],          # argmax 1 1 0 (tie) 2
                      [0.0, 0.3, 0.7], [0.5, 0.5, 9.0], [0.9, 0.1, 0.0]])                            # two states: 1 0 (tie) 0
    got = diarize.vbx_labels(gamma, [0, 4, 7], [3, 2])
    assert got.tolist() == [1, 1, 2, 3, 1, 2, 2] and got.dtype == np.int32
    assert diarize.vbx_labels(gamma[:4], [0, 4], [3]).tolist() == V.labels_of(gamma[:4]).tolist()


def test_argument_errors(diarize):
    X, Phi, _, first = V.planted(12, 3, 3, 2, seed=1)
    ok = dict(init_labels=first)
    for bad in (dict(Fa=0.0), dict(Fb=-1.0), dict(Fa=np.inf), dict(loop_prob=0.0), dict(loop_prob=1.0), dict(max_iters=0),
                dict(epsilon=np.nan), dict(epsilon=np.inf), dict(init_labels=None), dict(gamma=np.ones((12, 3)) / 3),
                dict(init_labels=first[:-1]), dict(pi=np.ones((1, 3)) / 3), dict(n_states=[3])):
        with pytest.raises(ValueError):
            diarize.vbx(X, Phi, [0, 12], **dict(ok, **bad))
    g = np.ones((12, 3)) / 3
    for bad in (dict(gamma=g[:-1]), dict(gamma=g, n_states=[4]), dict(gamma=g, n_states=[0]), dict(gamma=g, pi=np.ones((2, 3)) / 3),
                dict(gamma=g, rec_off=[0, 5]), dict(gamma=g, Phi=-Phi), dict(gamma=g, Phi=Phi[:-1])):
        kw = dict(X=X, Phi=Phi, rec_off=[0, 12])
        kw.update(bad)
        with pytest.raises(ValueError):
            diarize.vbx(**kw)
    with pytest.raises(ValueError):
        diarize.diarize({"a": np.zeros(3)}, [("a", "r", 0.0, 1.0)], "cosine", threshold=0.0, vbx={})
    with pytest.raises(ValueError):
        diarize.diarize({"a": np.zeros(3)}, [("a", "r", 0.0, 1.0)], "plda", threshold=0.0, vbx={"loop": 0.5}, plda=None, transform=None)


# ---- scripts/diarize.py --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def script_case(tmp_path_factory):
    """the two recordings of test_diar_cpu.py's script case (the same generator and seed) and a small PLDA trained on the host"""
    from pytorch_kaldi_resnet_amd import plda
    d = tmp_path_factory.mktemp("vbx_cli")
    rng = np.random.RandomState(5)
    keys, lines = [], []
    for reco, n in (("recA", 6), ("recB", 4)):
        for w in range(n):
            k = "%s-%08d-%08d" % (reco, 20 * w, 20 * w + 40)
            keys.append(k)
            lines.append("%s %s %.3f %.3f\n" % (k, reco, 0.2 * w, 0.2 * w + 0.4))
    centres = rng.randn(2, 16) * 4
    vec = {k: centres[i % 2] + 0.1 * rng.randn(16) for i, k in enumerate(keys)}
    paths = {k: str(d / k) for k in ("emb", "segments", "lda", "plda", "num")}
    with open(paths["emb"], "w") as f:
        for k in keys:
            f.write(k + " [ " + " ".join("%.6f" % v for v in vec[k]) + " ]\n")
    with open(paths["segments"], "w") as f:
        f.write("".join(lines))
    with open(paths["num"], "w") as f:
        f.write("recA 3\nrecB 3\n")
    train, utt2spk = {}, {}
    for spk in range(24):
        centre = rng.randn(16) * 4
        for u in range(6):
            train["s%02d-u%d" % (spk, u)] = (centre + 0.1 * rng.randn(16)).astype(np.float32)
            utt2spk["s%02d-u%d" % (spk, u)] = "s%02d" % spk
    mean = np.mean(np.stack(list(train.values())).astype(np.float64), axis=0).astype(np.float32)
    transform, _ = plda.compute_lda(train, utt2spk, dim=6, mean=mean, backend="host")
    model = plda.compute_plda(train, utt2spk, transform, mean=mean, backend="host")
    plda.write_transform(paths["lda"], transform)
    plda.write_plda(paths["plda"], *model)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def run(*flags):
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "diarize.py"), "--embeddings", paths["emb"], "--segments", paths["segments"]]
        return subprocess.run(cmd + list(flags), env=env, capture_output=True, text=True, timeout=300)

    return {"dir": d, "keys": keys, "paths": paths, "run": run,
            "plda_flags": ["--backend-score", "plda", "--transform", paths["lda"], "--plda", paths["plda"]]}


def test_script_without_vbx_writes_what_it_wrote_before(script_case):
    """tests/golden/vbx holds the files the script wrote for these inputs before it knew --vbx"""
    c = script_case
    for name, flags in (("cosine", ["--threshold", "0.0"]), ("plda", c["plda_flags"] + ["--reco2num-spk", c["paths"]["num"]])):
        out = str(c["dir"] / ("plain_" + name))
        r = c["run"]("--out-dir", out, *flags)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(out)) == ["labels", "rttm"]
        for f in ("labels", "rttm"):
            assert open(os.path.join(out, f), "rb").read() == open(os.path.join(GOLDEN, "%s.%s" % (name, f)), "rb").read(), (name, f)


def test_script_with_vbx(script_case, diarize):
    from pytorch_kaldi_resnet_amd import plda, scoring
    c = script_case
    out = str(c["dir"] / "vbx")
    r = c["run"]("--out-dir", out, "--reco2num-spk", c["paths"]["num"], "--vbx", "--vbx-max-iters", "15", "--vbx-loop-prob", "0.8",
                 *c["plda_flags"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["labels", "labels.ahc", "rttm"]
    first = [l.split() for l in open(os.path.join(out, "labels.ahc"))]
    final = [l.split() for l in open(os.path.join(out, "labels"))]
    assert [k for k, _ in first] == c["keys"] == [k for k, _ in final]
    plain = str(c["dir"] / "plain_for_vbx")
    assert c["run"]("--out-dir", plain, "--reco2num-spk", c["paths"]["num"], *c["plda_flags"]).returncode == 0
    assert open(os.path.join(out, "labels.ahc")).read() == open(os.path.join(plain, "labels")).read()
    assert sorted({v for _, v in first[:6]}) == ["1", "2", "3"]                       # the first pass was told three speakers
    table = scoring.read_embeddings(c["paths"]["emb"])
    emb = table.mat[[table.index[k] for k in c["keys"]]]
    X, Phi = diarize.vbx_inputs(emb, None, plda.read_transform(c["paths"]["lda"]), plda.read_plda(c["paths"]["plda"]))
    res = diarize.vbx(X, Phi, [0, 6, 10], init_labels=np.array([int(v) for _, v in first]), max_iters=15, loop_prob=0.8)
    assert [int(v) for _, v in final] == res["labels"].tolist()
    assert [int(v) for _, v in final] == [1, 2] * 5                                   # VBx prunes the third speaker: the two centres
    segs = diarize.read_segments(c["paths"]["segments"])
    assert open(os.path.join(out, "rttm")).read().splitlines() == diarize.make_rttm(segs, res["labels"].tolist())


def test_script_parser_errors(script_case):
    c = script_case
    never = str(c["dir"] / "never")
    for flags, words in [(["--threshold", "0", "--vbx"], ["--vbx", "plda"]),
                         (["--threshold", "0", "--vbx", "--vbx-loop-prob", "1.5"] + c["plda_flags"], ["loop_prob"]),
                         (["--threshold", "0", "--vbx", "--vbx-max-iters", "0"] + c["plda_flags"], ["max_iters"]),
                         (["--threshold", "0", "--vbx", "--vbx-fa", "x"] + c["plda_flags"], ["--vbx-fa"])]:
        r = c["run"]("--out-dir", never, *flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    assert not os.path.exists(never)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ["spk_vbx_threads", "spk_vbx_max_states", "spk_vbx_ws_elems", "spk_vbx_batch"]


def test_exports_are_declared_bound_and_exported():
    from helpers import header_params
    from pytorch_kaldi_resnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        if name == "spk_vbx_ws_elems":                                      # the one export that returns long long
            m = re.search(r"\blong long\s+%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
            params = m.group(1).split(",")
        else:
            params = [p for p in header_params(name) if p != "void"]
        assert len(params) == len(hip._SIGS[name]), name


def test_batches_are_refused_on_the_host_before_any_launch():
    """the argument checks need no device: with every device pointer NULL a good batch gets as far as the pointer check"""
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    assert lib.spk_vbx_max_states() == 64 and lib.spk_vbx_threads() % 64 == 0

    def need(rec_off, Smax, D):
        ro = np.asarray(rec_off, dtype=np.int64)
        return lib.spk_vbx_ws_elems(ro.ctypes.data, ro.size - 1, Smax, D)

    def vbx(rec_off=(0, 3, 8), Ntot=8, D=4, Smax=5, n_states=(5, 1), Fa=0.3, Fb=17.0, loopP=0.99, iters=3, eps=1e-6, ws=None):
        ro = np.asarray(rec_off, dtype=np.int64)
        ns = np.asarray(n_states, dtype=np.int32)
        ws = 8 * (3 + 2 * Smax) + (ro.size - 1) * Smax * D if ws is None else ws
        rc = lib.spk_vbx_batch(None, None, ro.ctypes.data, None, ns.ctypes.data, None, None, None, Fa, Fb, loopP, iters, eps, None, ws,
                               None, None, Ntot, D, ro.size - 1, Smax, None)
        return rc, lib.spk_last_error().decode()

    assert need([0, 3, 8], 5, 4) == 8 * 13 + 2 * 5 * 4
    rc, msg = vbx()
    assert rc < 0 and "spk_vbx_batch: null device pointer" in msg
    for kw, word in [(dict(rec_off=(1, 8)), "rec_off"), (dict(rec_off=(0, 3, 3, 8), n_states=(1, 1, 1)), "empty"),
                     (dict(rec_off=(0, 9, 8)), "empty"), (dict(Ntot=9), "rec_off"), (dict(D=0), "D="), (dict(D=513), "D="),
                     (dict(Smax=65, n_states=(65, 1)), "Smax"), (dict(Smax=0), "Smax"), (dict(n_states=(6, 1)), "n_states"),
                     (dict(n_states=(5, 0)), "n_states"), (dict(rec_off=(0, 8193), Ntot=8193, n_states=(1,)), "cap"),
                     (dict(ws=8 * 13 + 2 * 5 * 4 - 1), "workspace"), (dict(Fa=0.0), "Fa"), (dict(Fa=np.nan), "Fa"), (dict(Fb=np.inf), "Fb"),
                     (dict(Fb=-1.0), "Fb"), (dict(loopP=0.0), "loopP"), (dict(loopP=1.0), "loopP"), (dict(loopP=np.nan), "loopP"),
                     (dict(iters=0), "max_iters"), (dict(eps=np.nan), "epsilon"), (dict(eps=np.inf), "epsilon")]:
        rc, msg = vbx(**kw)
        assert rc < 0 and msg.startswith("spk_vbx_batch") and word in msg, (kw, msg)
    rc, msg = vbx(eps=-np.inf)
    assert rc < 0 and "null device pointer" in msg
    assert need([0, 8193], 4, 4) < 0 and "spk_vbx_ws_elems" in lib.spk_last_error().decode()
    assert need([0, 3, 8], 65, 4) < 0 and need([0, 3, 8], 5, 513) < 0 and need([0, 3, 2], 5, 4) < 0
