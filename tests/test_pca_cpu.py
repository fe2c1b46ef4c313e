"""Per-recording PCA of the dense PLDA scores, host side: the properties of tests/pca_ref.py on planted data, the
host back end of diarize.pca_rows / score_dense(target_energy=) against the longdouble reference under the tolerance rule, the skips
and the clamps, argument errors, scripts/diarize.py --target-energy on files and the new exports of the C ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import diar_ref as DR
import pca_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vbx")
LD = np.longdouble
GRID = [c + (E,) for c in P.CASES for E in P.ENERGIES]


@pytest.fixture(scope="module")
def diarize():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


_YARD = {}


def yard(n, L, K, E):
    """the longdouble and float64 references of one case, computed once per module"""
    if (n, L, K, E) not in _YARD:
        z, _, model = P.planted(n, L, K)
        _YARD[(n, L, K, E)] = (z, model, P.Yardstick(z, model, E))
    return _YARD[(n, L, K, E)]


# ---- the reference's own properties -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,K,E", GRID)
def test_ref_properties(n, L, K, E):
    z, model, y = yard(n, L, K, E)
    P.assert_conditions(y.hi, E, (n, L, E))
    assert y.same_dim and not y.skip
    hi, d = y.hi, y.dim
    # dim against a direct statement of the rule
    s = hi["s"]
    frac = np.array([s[:k].sum() for k in range(1, L + 1)]) / s.sum()
    k = 1 + int(np.argmax(frac > E))
    assert d == min(k + 1, L, n - 1) and (k == 1 or frac[k - 2] <= E)
    # A_r W A_r^T = I and A_r B A_r^T = diag(psi_r): e64 is the distance between the float64 and the longdouble run of each product
    lo = y.lo
    _, _, W, B = P.project_model(hi["P"][:, :d].T, model, LD)
    _, _, W64, B64 = P.project_model(lo["P"][:, :d].T, model, np.float64)
    for Mh, Ml, want, scale in ((W, W64, np.eye(d), 1.0), (B, B64, np.diag(hi["psi_r"]), float(hi["psi_r"].max()))):
        qh, ql = hi["A"] @ Mh @ hi["A"].T, (lo["A"] @ Ml @ lo["A"].T).astype(LD)
        e64 = float(np.abs(qh - ql).max())
        assert float(np.abs(qh - want).max()) <= P.M * e64 + 16 * P.ULP * scale, (n, L, E)
        assert float(np.abs(ql - want).max()) <= P.M * e64 + 16 * P.ULP * scale, (n, L, E)
    # the scores do not depend on the sign or the order of the eigenvectors
    perm = np.random.RandomState(n).permutation(d)
    sign = np.where(np.random.RandomState(L).rand(d) < 0.5, -1.0, 1.0).astype(LD)
    Pr = (hi["P"][:, :d].T * sign[:, None])[perm]
    psi2, A2, _, _ = P.project_model(Pr, model, LD)
    _, S2 = P.rows_and_scores(z, A2, -(A2 @ model[0].astype(LD)), psi2, d, LD)
    assert float(np.abs(S2 - hi["S"]).max()) <= P.M * y.e64["S"] + y.floor["S"]
    U = np.linalg.qr(np.random.RandomState(K).randn(d, d))[0].astype(LD)          # nor on the basis of the retained subspace
    psi3, A3, _, _ = P.project_model(U @ hi["P"][:, :d].T, model, LD)
    _, S3 = P.rows_and_scores(z, A3, -(A3 @ model[0].astype(LD)), psi3, d, LD)
    assert float(np.abs(S3 - hi["S"]).max()) <= P.M * y.e64["S"] + y.floor["S"]


# ---- the host back end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,L,K,E", GRID)
def test_host_matches_the_reference(diarize, n, L, K, E):
    z, model, y = yard(n, L, K, E)
    r = diarize.pca_rows(z, [0, n], model, E, backend="host")
    d = int(r["dim"][0])
    assert d == y.dim and r["info"].tolist() == [0]
    assert (r["U"][:, d:] == 0).all() and (r["psi_r"][0, d:] == 0).all() and (r["g"][0, d:] == 0).all()
    ratios = y.check(r["s"][0], r["psi_r"][0], P.scores_fp64(r["U"], r["psi_r"][0], d), ("host", n, L, E))
    print("host (%d, %d) E=%g: err / (e64 + floor) %s" % (n, L, E, {k: "%.3f" % v for k, v in ratios.items()}))


def _emb_case(ns, L, seed=3):
    """recordings of ns rows as embeddings whose projection (mean 0, identity transform) the scoring sees"""
    model = P.planted(8, L, 1, seed=50)[2]
    emb = np.concatenate([P.planted(n, L, min(3, n), seed=seed + i)[0] for i, n in enumerate(ns)]).astype(np.float64)
    return emb, np.concatenate([[0], np.cumsum(ns)]), dict(mean=np.zeros(L), transform=np.eye(L), plda=model)


def test_skips_clamps_and_the_global_scores(diarize):
    L = 6
    emb, ro, args = _emb_case([1, 5, 2, 9], L)
    emb[1:6] = emb[1]                                                      # a recording of identical rows
    p = diarize.pca_inputs(emb, ro, 0.5, **args)
    assert p["dim"].tolist()[:3] == [L, L, 1] and 2 <= p["dim"][3] <= L
    assert (p["psi_r"][0] == args["plda"][2]).all() and (p["psi_r"][1] == args["plda"][2]).all()
    got, mo = diarize.score_dense(emb, ro, "plda", target_energy=0.5, **args)
    plain, mo2 = diarize.score_dense(emb, ro, "plda", **args)
    assert (mo == mo2).all()
    # skipped recordings: section 6n's expression on the global rows, within its derived bound (diar_ref.dense_ref)
    U, q, g, K = diarize.dense_inputs(emb, "plda", **args)
    for r in (0, 1):
        n = int(ro[r + 1] - ro[r])
        ref, bound, _ = DR.dense_ref(U[ro[r]:ro[r + 1]], q[ro[r]:ro[r + 1]], g, K)
        for S in (got, plain):
            assert (np.abs(S[mo[r]:mo[r + 1]].reshape(n, n).astype(LD) - ref) <= bound).all(), r
    assert not np.array_equal(got[mo[3]:], plain[mo[3]:])
    S = got[mo[3]:mo[4]].reshape(9, 9)
    assert (S == S.T).all()
    # the clamps at E = 0.999: n - 1 on (17, 16), L on (33, 17)
    for (n, L2, K), want in (((17, 16, 3), 16), ((33, 17, 3), 17)):
        z, _, model = P.planted(n, L2, K)
        y = P.Yardstick(z, model, 0.999)
        r = diarize.pca_rows(z, [0, n], model, 0.999)
        assert r["dim"].tolist() == [want] == [y.dim]
        y.check(r["s"][0], r["psi_r"][0], P.scores_fp64(r["U"], r["psi_r"][0], want), ("host clamp", n, L2))
    z, _, model = P.planted(2, 4, 1)
    assert diarize.pca_rows(z, [0, 2], model, 0.9)["dim"].tolist() == [1]
    assert diarize.pca_rows(z[:1], [0, 1], model, 0.9)["dim"].tolist() == [4]


def test_no_target_energy_is_todays_path(diarize):
    emb, ro, args = _emb_case([4, 7], 5)
    a, mo = diarize.score_dense(emb, ro, "plda", **args)
    b, _ = diarize.score_dense(emb, ro, "plda", target_energy=None, **args)
    U, q, g, K = diarize.dense_inputs(emb, "plda", **args)
    want = diarize._score_rows(U, q, g, K, ro.astype(np.int64), "host", False)
    assert a.tobytes() == b.tobytes() == want.tobytes()
    keys = ["k%d" % i for i in range(11)]
    segs = [(k, "a" if i < 4 else "b", 0.2 * i, 0.2 * i + 0.4) for i, k in enumerate(keys)]
    res = diarize.diarize({k: emb[i] for i, k in enumerate(keys)}, segs, "plda", threshold=0.0, **args)
    assert "pca_dim" not in res
    res = diarize.diarize({k: emb[i] for i, k in enumerate(keys)}, segs, "plda", threshold=0.0, target_energy=0.5, **args)
    assert len(res["pca_dim"]) == 2 and all(isinstance(d, int) for d in res["pca_dim"])


def test_argument_errors(diarize):
    emb, ro, args = _emb_case([4, 7], 5)
    for E in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="target_energy"):
            diarize.score_dense(emb, ro, "plda", target_energy=E, **args)
    with pytest.raises(ValueError, match="plda"):
        diarize.score_dense(emb, ro, "cosine", target_energy=0.5)
    with pytest.raises(ValueError, match="plda"):
        diarize.diarize({"a": np.zeros(3)}, [("a", "r", 0.0, 1.0)], "cosine", threshold=0.0, target_energy=0.5)
    with pytest.raises(ValueError, match="target_energy"):
        diarize.diarize({"a": np.zeros(3)}, [("a", "r", 0.0, 1.0)], "plda", threshold=0.0, target_energy=2.0, **args)
    with pytest.raises(ValueError, match="dimensions"):
        diarize.pca_rows(np.zeros((3, 4), dtype=np.float32), [0, 3], args["plda"], 0.5)


def test_a_failed_cholesky_names_the_recording(diarize, monkeypatch):
    """W = Ti Ti^T of an invertible T is positive definite, so an indefinite W_r is handed to the per-recording step directly"""
    emb, ro, args = _emb_case([4, 7], 5)
    z = emb.astype(np.float32)
    dim, s, psi_r, A, b, info = diarize._pca_rec_host(z[:4], -np.eye(5), np.eye(5), args["plda"], 0.9)
    assert info == 2 and 1 <= dim <= 3 and not A.any() and not b.any() and not psi_r.any() and np.isfinite(s).all()
    host = diarize._pca_rec_host
    monkeypatch.setattr(diarize, "_pca_rec_host", lambda zr, W, B, model, E: host(zr, -W if len(zr) == 7 else W, B, model, E))
    with pytest.raises(ValueError, match=r"recording 1 \(info = 2"):
        diarize.pca_rows(z, ro, args["plda"], 0.9)


# ---- scripts/diarize.py --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def script_case(tmp_path_factory):
    """the files of test_vbx_cpu.py's script case (the same generator and seed): tests/golden/vbx holds what the script wrote for
    them before it knew --vbx or --target-energy"""
    from pytorch_kaldi_resnet_amd import plda
    d = tmp_path_factory.mktemp("pca_cli")
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


def test_script_with_and_without_target_energy(script_case, diarize):
    from pytorch_kaldi_resnet_amd import plda, scoring
    c = script_case
    plain = str(c["dir"] / "plain")
    r = c["run"]("--out-dir", plain, "--reco2num-spk", c["paths"]["num"], "--write-scores", *c["plda_flags"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(plain)) == ["labels", "rttm", "scores.recA", "scores.recB"]
    for f in ("labels", "rttm"):                                           # byte for byte what the parent's code path wrote
        assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(GOLDEN, "plda.%s" % f), "rb").read(), f
    out = str(c["dir"] / "pca")
    r = c["run"]("--out-dir", out, "--reco2num-spk", c["paths"]["num"], "--write-scores", "--target-energy", "0.5", *c["plda_flags"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted(os.listdir(out)) == ["labels", "pca_dim", "rttm", "scores.recA", "scores.recB"]
    table = scoring.read_embeddings(c["paths"]["emb"])
    emb = table.mat[[table.index[k] for k in c["keys"]]]
    args = dict(transform=plda.read_transform(c["paths"]["lda"]), plda=plda.read_plda(c["paths"]["plda"]))
    p = diarize.pca_inputs(emb, [0, 6, 10], 0.5, **args)
    assert open(os.path.join(out, "pca_dim")).read() == "recA %d\nrecB %d\n" % tuple(p["dim"])
    want, mo = diarize.score_dense(emb, [0, 6, 10], "plda", target_energy=0.5, **args)
    got = np.loadtxt(os.path.join(out, "scores.recA"))
    assert np.array_equal(got.astype(np.float32).ravel(), want[:36])
    assert not np.array_equal(got, np.loadtxt(os.path.join(plain, "scores.recA")))


def test_script_parser_errors(script_case):
    c = script_case
    never = str(c["dir"] / "never")
    for flags, words in [(["--threshold", "0", "--target-energy", "0.5"], ["--target-energy", "plda"]),
                         (["--threshold", "0", "--target-energy", "1.0"] + c["plda_flags"], ["--target-energy", "between"]),
                         (["--threshold", "0", "--target-energy", "0"] + c["plda_flags"], ["--target-energy", "between"]),
                         (["--threshold", "0", "--target-energy", "x"] + c["plda_flags"], ["--target-energy"])]:
        r = c["run"]("--out-dir", never, *flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    assert not os.path.exists(never)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ["spk_syevj_max_dim", "spk_syevj_max_sweeps", "spk_syevj_threads", "spk_syevj_ws_elems", "spk_syevj_batch", "spk_pca_plda_ws_elems",
       "spk_pca_plda_batch", "spk_pca_score_terms", "spk_affine_lennorm_rec", "spk_score_dense_q_rec", "spk_score_dense_rec"]


def test_exports_are_declared_bound_and_exported():
    from helpers import header_params
    from pytorch_kaldi_resnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        if name.endswith("_ws_elems"):                                     # the exports that return long long
            m = re.search(r"\blong long\s+%s\s*\(([^)]*)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
            params = m.group(1).split(",")
        else:
            params = [p for p in header_params(name) if p != "void"]
        assert len(params) == len(hip._SIGS[name]), name


def test_batches_are_refused_on_the_host_before_any_launch():
    """the argument checks need no device: with every device pointer NULL a good batch gets as far as the pointer check"""
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    assert lib.spk_syevj_max_dim() == 256 and lib.spk_syevj_max_sweeps() >= 8 and lib.spk_syevj_threads() % 64 == 0

    def pca(rec_off=(0, 3, 8), Ntot=8, L=4, E=0.5, ws=None):
        ro = np.asarray(rec_off, dtype=np.int64)
        R = ro.size - 1
        ws = R * (9 * (L + (L & 1)) ** 2 + L) + (R + 1) // 2 if ws is None else ws
        rc = lib.spk_pca_plda_batch(None, ro.ctypes.data, None, None, None, None, None, None, E, None, ws, None, None, None, None, None,
                                    None, Ntot, L, R, None)
        return rc, lib.spk_last_error().decode()

    def need(rec_off, L):
        ro = np.asarray(rec_off, dtype=np.int64)
        return lib.spk_pca_plda_ws_elems(ro.ctypes.data, ro.size - 1, L)

    assert need([0, 3, 8], 4) == 2 * (9 * 16 + 4) + 1 and need([0, 3, 8], 5) == 2 * (9 * 36 + 5) + 1
    rc, msg = pca()
    assert rc < 0 and "spk_pca_plda_batch: null device pointer" in msg
    for kw, word in [(dict(rec_off=(1, 8)), "rec_off"), (dict(rec_off=(0, 3, 3, 8)), "empty"), (dict(rec_off=(0, 9, 8)), "empty"),
                     (dict(Ntot=9), "rec_off"), (dict(L=0), "L="), (dict(L=257), "L="), (dict(E=0.0), "E="), (dict(E=1.0), "E="),
                     (dict(E=float("nan")), "E="), (dict(ws=2 * (9 * 16 + 4)), "workspace")]:
        rc, msg = pca(**kw)
        assert rc < 0 and msg.startswith("spk_pca_plda_batch") and word in msg, (kw, msg)
    assert need([0, 3, 2], 4) < 0 and "spk_pca_plda_ws_elems" in lib.spk_last_error().decode() and need([0, 3], 257) < 0

    def syevj(orders=(3, 4), ld=4, R=2, ws=None):
        od = np.asarray(orders, dtype=np.int32)
        rc = lib.spk_syevj_batch(None, od.ctypes.data, None, None, 2 * R * (ld + (ld & 1)) ** 2 if ws is None else ws, None, None, None,
                                 None, R, ld, None)
        return rc, lib.spk_last_error().decode()

    rc, msg = syevj()
    assert rc < 0 and "spk_syevj_batch: null device pointer" in msg
    for kw, word in [(dict(ld=0), "ld="), (dict(ld=257), "ld="), (dict(orders=(0, 4)), "orders"), (dict(orders=(3, 5)), "orders"),
                     (dict(R=0), "R="), (dict(ws=63), "workspace")]:
        rc, msg = syevj(**kw)
        assert rc < 0 and msg.startswith("spk_syevj_batch") and word in msg, (kw, msg)

    assert lib.spk_pca_score_terms(None, None, None, None, None, 2, 4, None) < 0
    assert "spk_pca_score_terms: null device pointer" in lib.spk_last_error().decode()
    for R, L in ((0, 4), (2, 0), (2, 513)):
        assert lib.spk_pca_score_terms(None, None, None, None, None, R, L, None) < 0
        assert lib.spk_last_error().decode().startswith("spk_pca_score_terms: " + ("R=" if R == 0 else "L="))

    ro = np.array([0, 3, 8], dtype=np.int64)
    for name, call in [("spk_affine_lennorm_rec", lambda r, L: lib.spk_affine_lennorm_rec(None, r.ctypes.data, None, None, None, None,
                                                                                          None, 1, None, 8, L, r.size - 1, None)),
                       ("spk_score_dense_q_rec", lambda r, L: lib.spk_score_dense_q_rec(None, r.ctypes.data, None, None, -0.5, None, 8, L,
                                                                                        r.size - 1, None)),
                       ("spk_score_dense_rec", lambda r, L: lib.spk_score_dense_rec(None, r.ctypes.data, None, None, None, None, None, 8, L,
                                                                                    r.size - 1, None))]:
        assert call(ro, 4) < 0 and (name + ": null device pointer") in lib.spk_last_error().decode()
        assert call(np.array([0, 8, 8], dtype=np.int64), 4) < 0 and lib.spk_last_error().decode().startswith(name)
        assert call(ro, 0) < 0 and lib.spk_last_error().decode().startswith(name)
