"""The PLDA back end on the host (no GPU): plda.py's `host` back end, the three scripts, the two file formats and test.sh against
the independent restatement (tests/plda_ref.py) on its seeded synthetic set.

Rows of eigenvector matrices have no defined sign, so only invariants are compared; the Plda object's are pulled back through the
LDA matrix (whose row signs are as free) into the input space.  Tolerances: a quantity that both sides compute in fp64 from the same
float32 stage values is held to 1e-10 relative (fp64 roundings times the condition of 24 x 24 factorisations); a quantity behind a
float32 stage rounding is held to d = max |rounded restatement - all-fp64 restatement|, the restatement's own sensitivity to those
roundings - the host back end rounds the same stages, and a different fp64 summation order can at most move single roundings."""
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import hip, plda, scoring

import plda_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def S():
    return R.synthetic()


@pytest.fixture(scope="module")
def ref(S):
    return R.stage(S, True), R.stage(S, False)


@pytest.fixture(scope="module")
def files(S, tmp_path_factory):
    d = tmp_path_factory.mktemp("plda")
    R.write_text_ark(str(d / "train.iv"), S["train_keys"], S["train"])
    R.write_text_ark(str(d / "test.iv"), S["test_keys"], S["test"])
    (d / "mean.vec").write_text(" [ " + " ".join(map(str, S["mean"])) + " ]\n")
    (d / "utt2spk").write_text("".join("%s %s\n" % kv for kv in S["utt2spk"].items()))
    (d / "trials").write_text("".join("%s %s %s\n" % t for t in S["trials"]))
    return d


@pytest.fixture(scope="module")
def host(S, files):
    d = str(files)
    tr, te = scoring.read_embeddings(os.path.join(d, "train.iv")), scoring.read_embeddings(os.path.join(d, "test.iv"))
    T, ev = plda.compute_lda(tr, S["utt2spk"], R.LDA_DIM, mean=S["mean"])
    P = plda.compute_plda(tr, S["utt2spk"], T, R.EM_ITERS, S["mean"])
    scores, labels = plda.plda_score(te, te, os.path.join(d, "trials"), S["mean"], T, P)
    return {"train": tr, "test": te, "lda": T, "lda_ev": ev, "plda": P, "scores": scores, "labels": labels}


def pulled(lda, P):
    A = np.asarray(lda, dtype=np.float64)[:, :-1]
    psi, g1, g2 = R.invariants(P)
    return psi, A.T @ g1 @ A, A.T @ g2 @ A


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def test_the_synthetic_set_is_well_posed(S, ref):
    _, f = ref
    psi, ev = f["plda"][2], f["lda_ev"][:R.LDA_DIM]
    assert S["train"].shape == (136, 24) and S["train"].dtype == np.float32 and len(set(S["utt2spk"].values())) == 40
    assert np.min(-np.diff(psi) / psi[:-1]) > 1e-3 and np.min(-np.diff(ev) / ev[:-1]) > 1e-2
    T = f["plda"][1]
    assert np.abs(T @ f["W"] @ T.T - np.eye(len(T))).max() < 1e-10            # the restatement itself gives about 2e-15
    A = f["lda"][:, :-1]
    assert np.abs(A @ f["within"] @ A.T - np.eye(R.LDA_DIM)).max() < 1e-10


def test_lda_against_the_restatement(host, ref):
    r, _ = ref
    assert rel(host["lda_ev"][:R.LDA_DIM], r["lda_ev"][:R.LDA_DIM]) < 1e-10
    A = host["lda"].astype(np.float64)
    assert host["lda"].dtype == np.float32 and A.shape == (R.LDA_DIM, R.D + 1)
    # float32 rounding of A: 2^-24 relative per element, D terms per product
    assert np.abs(A[:, :-1] @ r["within"] @ A[:, :-1].T - np.eye(R.LDA_DIM)).max() < 1e-5
    assert rel(A[:, :-1].T @ A[:, :-1], r["lda"][:, :-1].T @ r["lda"][:, :-1]) < 1e-6
    assert rel(np.abs(A[:, -1]), np.abs(r["lda"][:, -1])) < 1e-6


def test_plda_against_the_restatement(S, host, ref):
    r, f = ref
    d_psi = float((np.abs(r["plda"][2] - f["plda"][2]) / f["plda"][2]).max())
    got, want, full = pulled(host["lda"], host["plda"]), pulled(r["lda"], r["plda"]), pulled(f["lda"], f["plda"])
    print("psi: host vs rounded restatement %.2e of d = %.2e" % (float((np.abs(got[0] - want[0]) / want[0]).max()) / d_psi, d_psi))
    assert float((np.abs(got[0] - want[0]) / want[0]).max()) <= d_psi
    for k in (1, 2):
        d = rel(want[k], full[k])
        print("invariant %d: %.2e of d = %.2e" % (k, rel(got[k], want[k]) / d, d))
        assert rel(got[k], want[k]) <= d
    assert host["plda"][0].shape == (R.LDA_DIM,)
    # the estimator's own invariant, on the host back end's W: retrain on the restatement's z and compare W through the transform
    x0 = R.center(S["train"], S["mean"])
    z = R.project(x0, r["lda"])
    _, T, psi, W, B = R.plda_train(S["train_keys"], z, S["utt2spk"], R.EM_ITERS)
    P = plda.compute_plda(host["train"], S["utt2spk"], r["lda"], R.EM_ITERS, S["mean"])
    assert rel(P[2], psi) < 1e-10 and rel(P[1].T @ P[1], T.T @ T) < 1e-10 and rel(P[0], r["plda"][0]) < 1e-10
    assert np.abs(P[1] @ W @ P[1].T - np.eye(R.LDA_DIM)).max() < 1e-10
    assert np.abs(P[1] @ B @ P[1].T - np.diag(psi)).max() < 1e-10 * psi.max()


def test_scores_and_report_against_the_restatement(S, host, ref, files):
    r, f = ref
    d = float(np.abs(r["scores"] - f["scores"]).max())
    err = float(np.abs(host["scores"].astype(np.float64) - r["scores"]).max())
    print("scores: |host - rounded restatement| = %.2e, d = %.2e, range %.1f ... %.1f" % (err, d, f["scores"].min(), f["scores"].max()))
    assert host["scores"].dtype == np.float32 and err <= d
    lab = [t[2] == "target" for t in S["trials"]]
    assert np.array_equal(host["labels"], np.array(lab, dtype=int))
    rep = scoring.score_and_report(host["test"], host["test"], str(files / "trials"), S["mean"], plda=host["plda"], transform=host["lda"])
    want = R.error_rates(r["scores"], lab)
    assert (rep["eer"], rep["min_dcf"][0][0], rep["min_dcf"][1][0]) == pytest.approx(want, abs=1e-15)
    assert 0 < want[0] < 0.5


@pytest.mark.parametrize("kw", [dict(smoothing=0.1), dict(num_utts=3), dict(simple=True), dict(normalize_length=False),
                                dict(num_utts=3, smoothing=0.1)], ids=str)
def test_scoring_options_against_the_formula(S, host, ref, files, kw):
    r, f = ref
    num = {k: (3 if i % 2 else 1) for i, k in enumerate(S["test_keys"])} if "num_utts" in kw else None
    rkw = dict(kw)
    rkw.pop("num_utts", None)
    args = (S["test_keys"], S["test"], S["test_keys"], S["test"], S["trials"], S["mean"], r["lda"], r["plda"])
    want = R.score(*args, num_utts=num, rounded=True, **rkw)
    d = float(np.abs(want - R.score(*args, num_utts=num, rounded=False, **rkw)).max())
    got, _ = plda.plda_score(host["test"], host["test"], str(files / "trials"), S["mean"], r["lda"], r["plda"], num_utts=num,
                             normalize_length=kw.get("normalize_length", True), simple_length_normalization=kw.get("simple", False),
                             smoothing=kw.get("smoothing", 0.0))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("%s: err %.2e d %.2e" % (kw, err, d))
    assert err <= d
    assert float(np.abs(want - r["scores"]).max()) > 100 * d          # the option is not a no-op


def test_smoothing_zero_is_the_identity(host):
    m, T, psi = plda.smooth(host["plda"], 0.0)
    assert m is host["plda"][0] and T is host["plda"][1] and psi is host["plda"][2]
    m, T, psi = plda.smooth(host["plda"], 0.1)
    c = 1 + 0.1 * host["plda"][2]
    assert np.array_equal(psi, host["plda"][2] / c) and np.allclose(T, host["plda"][1] / np.sqrt(c)[:, None], rtol=1e-15, atol=0)


def test_a_zero_vector_stays_zero_and_scores_finite(host, S, files):
    A = host["lda"][:, :-1]                                     # without the offset column a zero input projects to zero
    x0 = np.zeros((3, R.D), dtype=np.float32)
    x0[1] = 1.0
    z = plda.project(x0, A)
    assert not z[0].any() and not z[2].any() and np.isfinite(z).all()
    assert abs(float(np.linalg.norm(z[1].astype(np.float64))) - np.sqrt(R.LDA_DIM)) < 1e-5
    u = plda._side_host(z, host["plda"], np.ones(3), True, False)
    assert np.isfinite(u).all()
    P0 = (np.zeros(R.LDA_DIM), host["plda"][1], host["plda"][2])           # mean 0: the zero vector transforms to zero
    assert not plda._side_host(z, P0, np.ones(3), True, False)[0].any()


def test_speaker_without_vectors_and_utterance_without_speaker(S, host, ref, capfd, tmp_path):
    u2s = dict(S["utt2spk"])
    u2s["ghost-u0"] = "ghost"                                   # a speaker without a vector: skipped
    gone = S["train_keys"][5]
    del u2s[gone]                                               # an utterance without a speaker: skipped with a warning
    T, ev = plda.compute_lda(host["train"], u2s, R.LDA_DIM, mean=S["mean"])
    assert "WARNING: %s has no speaker" % gone in capfd.readouterr().err
    x0 = R.center(S["train"], S["mean"])
    Tr, evr, _ = R.lda(S["train_keys"], x0, u2s, R.LDA_DIM)
    assert rel(ev[:R.LDA_DIM], evr[:R.LDA_DIM]) < 1e-10
    assert rel(ev[:R.LDA_DIM], ref[0]["lda_ev"][:R.LDA_DIM]) > 1e-6       # the dropped utterance shows
    P = plda.compute_plda(host["train"], u2s, Tr, R.EM_ITERS, S["mean"])
    want = R.plda_train(S["train_keys"], R.project(x0, Tr), u2s, R.EM_ITERS)
    assert rel(P[2], want[2]) < 1e-10 and rel(P[0], want[0]) < 1e-10
    with pytest.raises(ValueError, match="no utterance"):
        plda.compute_lda(host["train"], {}, R.LDA_DIM)
    (tmp_path / "trials").write_text("%s %s target\n" % (S["test_keys"][0], S["test_keys"][1]))      # the second key is not in `train`
    with pytest.raises(KeyError):
        plda.plda_score(host["test"], host["train"], str(tmp_path / "trials"), S["mean"], T, P)


def test_without_a_mean_the_archive_mean_is_subtracted(S, host):
    T0, ev0 = plda.compute_lda(host["train"], S["utt2spk"], R.LDA_DIM)
    x0 = R.center(S["train"], None)
    _, evr, _ = R.lda(S["train_keys"], x0, S["utt2spk"], R.LDA_DIM)
    assert rel(ev0[:R.LDA_DIM], evr[:R.LDA_DIM]) < 1e-10


def test_transform_file_bytes(tmp_path):
    M = np.array([[1.5, -2.0, 0.25], [3.0, 4.0, -0.125]])
    p = str(tmp_path / "transform.mat")
    plda.write_transform(p, M)
    want = b"\0BFM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", 3) + struct.pack("<6f", 1.5, -2.0, 0.25, 3.0, 4.0, -0.125)
    assert open(p, "rb").read() == want
    assert np.array_equal(plda.read_transform(p), M)
    (tmp_path / "t.txt").write_text(" [\n  1.5 -2 0.25 \n  3 4 -0.125 ]\n")
    assert np.array_equal(plda.read_transform(str(tmp_path / "t.txt")), M)


def test_plda_file_bytes_and_text_form(tmp_path):
    mean, T, psi = np.array([0.5, -1.0]), np.array([[2.0, 0.0], [0.25, 4.0]]), np.array([3.0, 0.0])
    p = str(tmp_path / "plda")
    plda.write_plda(p, mean, T, psi)
    want = (b"\0B<Plda> " + b"DV \x04" + struct.pack("<i", 2) + struct.pack("<2d", 0.5, -1.0)
            + b"DM \x04" + struct.pack("<i", 2) + b"\x04" + struct.pack("<i", 2) + struct.pack("<4d", 2.0, 0.0, 0.25, 4.0)
            + b"DV \x04" + struct.pack("<i", 2) + struct.pack("<2d", 3.0, 0.0) + b"</Plda> ")
    assert open(p, "rb").read() == want
    got = plda.read_plda(p)
    assert all(np.array_equal(a, b) for a, b in zip(got, (mean, T, psi)))
    (tmp_path / "plda.txt").write_text("<Plda>  [ 0.5 -1 ]\n [\n  2 0 \n  0.25 4 ]\n [ 3 0 ]\n</Plda> \n")
    got = plda.read_plda(str(tmp_path / "plda.txt"))
    assert all(np.array_equal(a, b) for a, b in zip(got, (mean, T, psi)))
    (tmp_path / "bad").write_bytes(want.replace(b"DM ", b"FM "))
    with pytest.raises(Exception, match="expected"):
        plda.read_plda(str(tmp_path / "bad"))


def _run(args, cwd, env=None):
    return subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)


def test_scripts_and_test_sh_end_to_end_on_host(S, host, ref, files, tmp_path):
    d = str(tmp_path)
    for f in ("train.iv", "test.iv", "mean.vec", "utt2spk", "trials"):
        shutil.copy(str(files / f), d)
    # the model is missing: the message names the two scripts and says why Kaldi's binaries are not called
    p = _run(["bash", os.path.join(ROOT, "test.sh"), d, d, "plda", "12", os.path.join(d, "trials")], d)
    assert p.returncode == 1 and "compute_lda.py" in p.stderr and "compute_plda.py" in p.stderr and "DESIGN.md section 7" in p.stderr
    assert not os.path.exists(os.path.join(d, "scores_plda"))
    py = sys.executable
    p = _run([py, os.path.join(ROOT, "scripts", "compute_lda.py"), "--dim", str(R.LDA_DIM), "--total-covariance-factor", "0.0",
              "--mean", "mean.vec", "train.iv", "utt2spk", "transform.mat"], d)
    assert p.returncode == 0, p.stderr
    p = _run([py, os.path.join(ROOT, "scripts", "compute_plda.py"), "--num-em-iters", str(R.EM_ITERS), "--mean", "mean.vec", "train.iv",
              "utt2spk", "transform.mat", "plda"], d)
    assert p.returncode == 0, p.stderr
    assert np.array_equal(plda.read_transform(os.path.join(d, "transform.mat")), host["lda"].astype(np.float64))
    assert all(np.array_equal(a, b) for a, b in zip(plda.read_plda(os.path.join(d, "plda")), host["plda"]))
    p = _run(["bash", os.path.join(ROOT, "test.sh"), d, d, "plda", "12", os.path.join(d, "trials")], d)
    assert p.returncode == 0, p.stderr
    lines = open(os.path.join(d, "scores_plda")).read().splitlines()
    assert [tuple(l.split()[:2]) for l in lines] == [t[:2] for t in S["trials"]]
    got = np.array([np.float32(l.split()[2]) for l in lines])
    assert np.array_equal(got, host["scores"])                  # float32's digits are kept: the file round-trips
    lab = [t[2] == "target" for t in S["trials"]]
    e, d1, d2 = R.error_rates(ref[0]["scores"], lab)
    report = "EER: {0:.2%}%\nminDCF(p-target=0.01): {1:.4f}\nminDCF(p-target=0.001): {2:.4f}\n".format(e, d1, d2)
    assert open(os.path.join(d, "eer_plda")).read() == report
    assert p.stdout.endswith("backend: plda\n" + report)
    # an unknown key is an error, as in cosine_score.py
    with open(os.path.join(d, "trials"), "a") as f:
        f.write("nobody %s target\n" % S["test_keys"][0])
    p = _run([py, os.path.join(ROOT, "scripts", "plda_score.py"), "--mean", "mean.vec", "--transform", "transform.mat", "--plda", "plda",
              "--enroll", "test.iv", "--test", "test.iv", "--trials", "trials", "--score-file", "s"], d)
    assert p.returncode != 0 and "nobody" in p.stderr


def test_new_exports_are_declared_bound_and_exported():
    names = ["spk_scatter_f64", "spk_scatter_f64_workspace", "spk_scatter_slab_rows", "spk_segment_sum_f64", "spk_affine_lennorm",
             "spk_plda_posterior_rows", "spk_plda_llr"]
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
        assert re.search(r" T %s$" % name, nm, re.M), name
    for name in names:
        if name in hip._SIGS:
            from helpers import header_params
            assert len(header_params(name)) == len(hip._SIGS[name]), name
    lib = hip.lib()
    # argument validation happens on the host before any launch
    assert lib.spk_scatter_f64(None, 0, 0, None, None, None, None, 1, 1, None) < 0 and b"spk_scatter_f64" in lib.spk_last_error()
    assert lib.spk_scatter_f64_workspace(1, 513) == 0 and lib.spk_scatter_f64_workspace(5, 3) == 72
    R1 = lib.spk_scatter_slab_rows(1)
    assert R1 >= 4 and R1 % 4 == 0 and lib.spk_scatter_f64_workspace(3 * R1 - 1, 2) == 3 * 32
    assert lib.spk_scatter_f64_workspace(R1 + 1, 2) == 2 * 32
