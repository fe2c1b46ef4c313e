"""The scoring stage after the cosine scores, on the host (no GPU): speaker-mean cohort, adaptive S-norm, EER / minDCF sweep,
the two new scripts and test.sh, against fixtures the reference's own programs wrote (tools/make_backend_golden.py).  Everything
is compared exactly: bytes for files, == for doubles."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import scoring

import backend_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = R.GOLD


def _read(path):
    return open(path).read()


def test_speaker_mean_reproduces_the_reference_file_byte_for_byte(tmp_path):
    keys, mat = R.read_text_ark(os.path.join(GOLD, "train.iv"))
    want = _read(os.path.join(GOLD, "spk_mean.vec"))
    assert R.speaker_mean_text(R.speaker_mean(keys, mat, R.read_utt2spk(os.path.join(GOLD, "utt2spk")))) == want
    out = str(tmp_path / "spk_mean.vec")
    means = scoring.speaker_mean(scoring.read_embeddings(os.path.join(GOLD, "train.iv")), os.path.join(GOLD, "utt2spk"), out)
    assert _read(out) == want
    assert list(means) == [l.split()[0] for l in want.splitlines()]          # order of first appearance in the archive
    assert all(v.dtype == np.float32 for v in means.values())
    # a plain dict of vectors gives the same as the EmbTable
    again = scoring.speaker_mean(dict(zip(keys, mat)), os.path.join(GOLD, "utt2spk"))
    assert all(np.array_equal(again[k], means[k]) for k in means)


def test_speaker_mean_rejects_an_utterance_without_speaker(tmp_path):
    lines = open(os.path.join(GOLD, "utt2spk")).read().splitlines()
    gone = lines.pop(3).split()[0]
    (tmp_path / "utt2spk").write_text("\n".join(lines) + "\n")
    with pytest.raises(Exception, match="%s not specified to any speaker" % gone):
        scoring.speaker_mean(scoring.read_embeddings(os.path.join(GOLD, "train.iv")), str(tmp_path / "utt2spk"))


def test_adaptive_snorm_reproduces_the_reference_file_byte_for_byte(tmp_path):
    stats = scoring.read_mean_std(os.path.join(GOLD, "topk_mean_std"))
    scoring.adaptive_snorm(stats, stats, os.path.join(GOLD, "scores"), str(tmp_path / "snorm"))
    want = _read(os.path.join(GOLD, "scores_snorm"))
    assert _read(str(tmp_path / "snorm")) == want
    names = list(stats)
    trials = [l.split() for l in open(os.path.join(GOLD, "scores"))]
    mu = np.array([stats[k][0] for k in names])
    sd = np.array([stats[k][1] for k in names])
    ia = [names.index(a) for a, _, _ in trials]
    ib = [names.index(b) for _, b, _ in trials]
    ref = R.snorm([float(s) for _, _, s in trials], ia, ib, mu, sd, mu, sd)
    assert "".join("{} {} {}\n".format(a, b, v) for (a, b, _), v in zip(trials, ref.tolist())) == want


def test_sweep_equals_the_reference_doubles():
    cases = R.golden_sweep_cases()
    assert len(cases) >= 30
    for s, lab, costs, exp in cases:
        eer, _, dcf = R.sweep(s, lab, costs)
        assert [eer] + [v for d, t, _ in dcf for v in (d, t)] == exp.tolist()
        if len(s) <= 64:
            assert R.sweep_loop(s.tolist(), lab.tolist(), costs) == (eer, _, dcf)
        rep = scoring.error_rates(s, lab, costs)
        assert [rep["eer"]] + [v for d, t, _ in rep["min_dcf"] for v in (d, t)] == exp.tolist()
        assert rep["eer_index"] == _ and [p for _d, _t, p in rep["min_dcf"]] == [p for _d, _t, p in dcf]
        assert rep["n_target"] == int(lab.sum()) and rep["n_nontarget"] == len(lab) - int(lab.sum())
        assert scoring.min_dcf(s, lab, *costs[2]) == (exp[5], exp[6])
        assert scoring.compute_eer(s, lab) == exp[0]                      # the existing function agrees


def test_sweep_edges():
    assert scoring.error_rates([0.1, 0.2, 0.8, 0.9], [1, 1, 0, 0])["eer"] == 1.0
    assert scoring.error_rates([0.9, 0.8, 0.1, 0.0], [1, 1, 0, 0])["eer"] == 0.0
    # the minimum cost is attained at several positions: the first one is reported, with its threshold
    # (costs 0.25, 0.5, 0.25, 0.5 at the four positions)
    rep = scoring.error_rates([0.0, 1.0, 2.0, 3.0], [0, 1, 0, 1], ((0.5, 1, 1),))
    assert rep["min_dcf"] == R.sweep_loop([0.0, 1.0, 2.0, 3.0], [0, 1, 0, 1], ((0.5, 1, 1),))[2] == [(0.5, 0.0, 0)]
    # -0.0 and +0.0 are one threshold, taken in list order; the threshold keeps the sign of the original score
    rep = scoring.error_rates([0.0, -0.0, -0.0, 0.0], [0, 1, 0, 1], ((0.5, 1, 1),))
    assert rep == scoring.error_rates([0.0, 0.0, 0.0, 0.0], [0, 1, 0, 1], ((0.5, 1, 1),))


def test_sweep_argument_errors():
    with pytest.raises(ValueError):
        scoring.error_rates([0.1, 0.2], [1, 1])
    with pytest.raises(ValueError):
        scoring.error_rates([0.1, 0.2], [0, 0])
    with pytest.raises(ValueError, match="NaN"):
        scoring.error_rates([0.1, float("nan")], [0, 1])
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="--p-target must be greater than 0 and less than 1"):
            scoring.min_dcf([0.1, 0.2], [0, 1], p_target=bad)
    with pytest.raises(ValueError, match="--c-miss must be greater than 0"):
        scoring.min_dcf([0.1, 0.2], [0, 1], c_miss=0)
    with pytest.raises(ValueError, match="--c-fa must be greater than 0"):
        scoring.min_dcf([0.1, 0.2], [0, 1], c_fa=-1)
    with pytest.raises(ValueError):
        scoring.error_rates([0.1, 0.2, 0.3], [0, 1])


def _run(args, cwd):
    p = subprocess.run(args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr
    return p


@pytest.fixture()
def stage_dir(tmp_path):
    d = tmp_path / "backend"
    d.mkdir()
    for f in ("train.iv", "test.iv", "utt2spk", "mean.vec", "trials", "topk_mean_std", "scores"):
        shutil.copy(os.path.join(GOLD, f), str(d / f))
    return d


def test_scripts_print_what_the_reference_prints(stage_dir):
    d = str(stage_dir)
    p = _run([sys.executable, os.path.join(ROOT, "scripts", "compute_speaker_mean.py"), "train.iv", "utt2spk", "spk_mean.vec"], d)
    assert p.stdout == _read(os.path.join(GOLD, "spk_mean.stdout"))
    assert _read(os.path.join(d, "spk_mean.vec")) == _read(os.path.join(GOLD, "spk_mean.vec"))
    p = _run([sys.executable, os.path.join(ROOT, "scripts", "compute_min_dcf.py"), "--p-target", "0.01", "scores", "trials"], d)
    assert p.stdout == _read(os.path.join(GOLD, "min_dcf_0.01_eer_cosine.stdout"))
    assert "minDCF is %s at threshold " % p.stdout.strip() in p.stderr and "(p-target=0.01, c-miss=1,c-fa=1)" in p.stderr
    p = _run([sys.executable, os.path.join(ROOT, "scripts", "compute_min_dcf.py"), "--p-target", "0.05", "--c-miss", "10", "--c-fa", "2",
              "scores", "trials"], d)
    assert p.stdout == _read(os.path.join(GOLD, "min_dcf_0.05_10_2.stdout"))
    # a scored pair that the trial list does not hold
    with open(os.path.join(d, "scores"), "a") as f:
        f.write("nobody nothing 0.5\n")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_min_dcf.py"), "scores", "trials"], cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode != 0 and "Missing entry for nobody and nothing scores" in p.stderr


def test_test_sh_writes_the_reference_reports(stage_dir):
    d = str(stage_dir)
    for backend, report in (("cosine", "eer_cosine"), ("snorm", "eer_snorm_adapt_snorm")):
        p = _run(["bash", os.path.join(ROOT, "test.sh"), d, d, backend, "12", os.path.join(d, "trials")], d)
        assert _read(os.path.join(d, report)) == _read(os.path.join(GOLD, report))
        assert p.stdout.endswith("backend: %s\n" % backend + _read(os.path.join(GOLD, report)))
    assert _read(os.path.join(d, "eer_cosine")).startswith("EER: 16.67%%\n")           # the reference's literal `EER: $eer%`
    p = subprocess.run(["bash", os.path.join(ROOT, "test.sh"), d, d, "plda", "12"], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode != 0 and "DESIGN.md section 7" in p.stderr


def test_score_and_report_is_the_stage_in_one_call(stage_dir):
    d = str(stage_dir)
    emb = scoring.read_embeddings(os.path.join(d, "test.iv"))
    from pytorch_kaldi_resnet_amd import kaldi_io
    mean = kaldi_io.read_vec_flt(os.path.join(d, "mean.vec"))
    scores, labels = scoring.cosine_score(emb, emb, os.path.join(d, "trials"), mean)
    rep = scoring.score_and_report(emb, emb, os.path.join(d, "trials"), mean)
    assert rep == scoring.error_rates(scores.astype(np.float64), labels)
    stats = scoring.read_mean_std(os.path.join(d, "topk_mean_std"))
    rep = scoring.score_and_report(emb, emb, os.path.join(d, "trials"), mean, stats, stats, score_path=os.path.join(d, "sn"))
    got = np.array([float(l.split()[2]) for l in open(os.path.join(d, "sn"))])
    assert rep == scoring.error_rates(got, labels)
    names = list(stats)
    trials = [l.split()[:2] for l in open(os.path.join(d, "trials"))]
    mu, sd = np.array([stats[k][0] for k in names]), np.array([stats[k][1] for k in names])
    ref = R.snorm(scores.tolist(), [names.index(a) for a, _ in trials], [names.index(b) for _, b in trials], mu, sd, mu, sd)
    assert np.array_equal(got, ref)
