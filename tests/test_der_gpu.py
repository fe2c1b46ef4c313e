"""Diarization scoring on the device (csrc/der.hip): the `hip` back end against the host back end and against the
tick-by-tick restatement in tests/der_ref.py, everything bit-equal - the cases of tests/test_der_cpu.py, piece counts at the wave and
block edges, label counts up to spk_der_max_hyp(), 64 reference speakers, C on both sides of the LDS / workspace switch, batch
position and split, an empty job between full ones, the refusals, spk_ahc_cut_batch against cluster(backend="hip") and the sweep of
scripts/diarize.py.  With -s every case prints its jobs, pieces and label counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import der_cases as X
import der_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def D():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


def five(p):
    return (p["scored"], p["miss"], p["fa"], p["conf"], p["opt"])


def both_backends(D, c, want=None, tag=""):
    """one case on `hip` and on `host`: the same integers and DER, each mapping one-to-one and attaining opt; and the reference's where given"""
    args = dict(uem=None if c["uem"] is None else {"r": c["uem"]}, collar=c["collar"], ignore_overlap=c["ignore_overlap"], tick=X.TICK)
    hyp = {"r": c["hyp"]} if c["hyp"] else {}
    g = D.der({"r": c["ref"]}, hyp, backend="hip", **args)
    h = D.der({"r": c["ref"]}, hyp, backend="host", **args)
    gp, hp = g["per_recording"]["r"], h["per_recording"]["r"]
    print("%s: 1 job, %d pieces, %d labels, %d reference speakers -> %s" % (tag, len(c["hyp"]), len(set(t[0] for t in c["hyp"])),
                                                                             len(set(t[0] for t in c["ref"])), five(gp)))
    assert five(gp) == five(hp) and g["host_jobs"] == 0, (tag, five(gp), five(hp))
    assert gp["der"] == hp["der"] or (gp["der"] != gp["der"] and hp["der"] != hp["der"])
    if want is not None:
        assert five(gp) == der_ref.five(want), (tag, five(gp), der_ref.five(want))
        for m in (gp["mapping"], hp["mapping"]):
            assert len(set(m.values())) == len(m)
            assert sum(int(want["C"][want["ref_names"].index(a), want["hyp_names"].index(b)]) for a, b in m.items()) == want["opt"], (tag, m)
    return gp


def reference_of(c):
    return der_ref.der(c["ref"], c["hyp"], c["uem"], c["collar"], c["ignore_overlap"], X.TICK)


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.CASES))
def test_hip_matches_host_and_reference(D, name):
    X.check_case(D, name, "hip")
    both_backends(D, X.CASES[name], X.reference(name), name)


@pytest.mark.parametrize("pieces", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_piece_counts_at_wave_and_block_edges(D, pieces):
    c = X.random_case(200 + pieces, 3, min(pieces, 5), 12, pieces, ignore_overlap=pieces % 2 == 0)
    both_backends(D, c, reference_of(c), "pieces=%d" % pieces)


@pytest.mark.parametrize("Sr,Sh", [(2, 1), (3, 64), (3, 65), (7, None), (64, 70), (64, 64), (64, 65), (65, 3)])
def test_label_and_speaker_counts(D, ops, Sr, Sh):
    """Sh = None: spk_der_max_hyp().  64 x 64 entries of C fill LDS exactly, 64 x 65 lie in the job's workspace tile; 65 reference
    speakers are over the device limit: the job is the host's and the result says so"""
    max_ref, max_hyp, _ = ops.der_limits()
    Sh = max_hyp if Sh is None else Sh
    c = X.random_case(300 + Sr + Sh, Sr, Sh, 3 * Sr, Sh + 40, T=20.0)
    want = reference_of(c) if (min(Sr, Sh) <= 6 or der_ref.HAVE_SCIPY) else None
    if Sr > max_ref:
        g = D.der({"r": c["ref"]}, {"r": c["hyp"]}, collar=c["collar"], tick=X.TICK, backend="hip")
        assert g["host_jobs"] == 1 and (want is None or five(g["per_recording"]["r"]) == der_ref.five(want))
        return
    both_backends(D, c, want, "Sr=%d Sh=%d" % (Sr, Sh))


def _jobs(D, cases):
    preps, jobs = [], []
    for r, c in enumerate(cases):
        preps.append(D.der_reference(c["ref"], c["uem"], c["collar"], c["ignore_overlap"], X.TICK))
        lab, _, s, e = D._turn_ticks(c["hyp"], X.TICK)
        jobs.append((r, lab * 7 + 3, s, e))                                    # (labels that are not consecutive)
    return preps, jobs


def test_batch_position_split_and_an_empty_job(D):
    cases = [X.random_case(401, 4, 9, 12, 300), X.case(X.CASES["hand"]["ref"], []), X.random_case(402, 64, 65, 130, 200),
             X.random_case(403, 2, 3, 5, 65)]
    preps, jobs = _jobs(D, cases)
    host = D.score_jobs(preps, jobs, "host")
    base = D.score_jobs(preps, jobs, "hip")
    print("batch: %d jobs, pieces %s" % (len(jobs), [len(j[1]) for j in jobs]))
    assert np.array_equal(base[0], host[0]) and base[2] == 0
    assert base[0][1].tolist()[1:] == [base[0][1][0], 0, 0, 0] and base[1][1] == []      # the empty job: all miss
    for x, c in enumerate(cases):
        if min(len(preps[x]["speakers"]), len(set(t[0] for t in c["hyp"]))) <= 6 or der_ref.HAVE_SCIPY:
            assert tuple(base[0][x]) == der_ref.five(reference_of(c)), x
    order = [2, 3, 0, 1]
    moved = D.score_jobs(preps, [jobs[x] for x in order], "hip")
    assert np.array_equal(moved[0], base[0][order]) and moved[1] == [base[1][x] for x in order]
    split = D.score_jobs(preps, jobs, "hip", ws_budget_bytes=64)               # every job in a launch of its own
    assert np.array_equal(split[0], base[0]) and split[1] == base[1]
    twice = D.score_jobs(preps, jobs + jobs, "hip", ws_budget_bytes=8 * 700)
    assert np.array_equal(twice[0], np.concatenate([base[0], base[0]]))


def test_over_limit_shapes_are_refused_and_nothing_is_written(ops):
    import torch
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    max_ref, max_hyp, max_turns = ops.der_limits()
    n = max_turns + 1
    dev = torch.device("cuda")
    lab, ps, pe = torch.ones(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev), torch.ones(n, dtype=torch.int64, device=dev)
    out, mp = torch.full((1, 5), -7, dtype=torch.int64, device=dev), torch.full((1, max_ref), -7, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 17, dtype=torch.int64, device=dev)
    cells = torch.tensor([[0, 10, 1]], dtype=torch.int64, device=dev)
    for rec_tab, job in (([[0, 1, 1, 0]], [[0, 0, n, 1, 0, 0]]), ([[0, 1, 1, 0]], [[0, 0, 8, max_hyp + 1, 0, 0]]),
                         ([[0, 1, max_ref + 1, 0]], [[0, 0, 8, 1, 0, 0]]), ([[0, 2, 1, 0]], [[0, 0, 8, 1, 0, 0]]),
                         ([[0, 1, 1, 0]], [[0, 0, 8, 1, (1 << 17) - 3, 0]])):
        rt, jt = np.array(rec_tab, dtype=np.int64), np.array(job, dtype=np.int64)
        rc = lib.spk_der_batch(rt.ctypes.data, torch.from_numpy(rt).to(dev).data_ptr(), cells.data_ptr(), 1, 1, jt.ctypes.data,
                               torch.from_numpy(jt).to(dev).data_ptr(), 1, lab.data_ptr(), ps.data_ptr(), pe.data_ptr(), n, ws.data_ptr(),
                               ws.numel(), out.data_ptr(), mp.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc < 0 and b"spk_der_batch" in lib.spk_last_error(), (rec_tab, job)
        assert (out == -7).all() and (mp == -7).all()
    with pytest.raises(RuntimeError, match="spk_der"):
        ops.der_batch([[0, 1, 1, 0]], cells.cpu().numpy(), [[0, 0, 8, max_hyp + 1]], lab, ps, pe)
    cap = ops.ahc_max_n()
    labels = torch.full((1, 4), -7, dtype=torch.int32, device=dev)
    ro = np.array([0, cap + 1], dtype=np.int64)
    rc = lib.spk_ahc_cut_batch(lab.data_ptr(), ws.data_ptr(), lab.data_ptr(), ro.ctypes.data, ws.data_ptr(), ws.data_ptr(), 1, labels.data_ptr(),
                               cap + 1, 1, None)
    torch.cuda.synchronize()
    assert rc < 0 and b"spk_ahc_cut_batch" in lib.spk_last_error() and (labels == -7).all()


# ---- cutting the merge list -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def merged(D):
    sizes = [1, 2, 65, 1025]
    return (sizes,) + X.merge_case(D, sizes, 21, "hip")


@pytest.mark.parametrize("K", [1, 41])
def test_cut_batch_equals_cluster_on_the_device(D, merged, K):
    sizes, scores, rec_off, merges, cost, nm = merged
    th = X.cut_thresholds(cost, rec_off, nm, 41)[:K] if K > 1 else X.cut_thresholds(cost, rec_off, nm)[-1:]
    got = D.cut_merges(merges, cost, nm, rec_off, th, "hip")
    print("cut: %d recordings of %s windows, K = %d" % (len(sizes), sizes, K))
    assert got.dtype == np.int32 and got.shape == (K, rec_off[-1])
    assert np.array_equal(got, D.cut_merges(merges, cost, nm, rec_off, th, "host"))
    for k, t in enumerate(th):
        assert np.array_equal(got[k], D.cluster(scores, rec_off, threshold=t, backend="hip")[0]), (k, t)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
def _planted():
    recs = {"recA": [(0, 0.0, 9.0), (1, 9.0, 18.0), (0, 18.0, 24.0), (2, 24.0, 30.0)], "recB": [(1, 0.0, 6.0), (0, 6.0, 15.0)]}
    segs, emb, ref = [], [], {}
    for i, (reco, turns) in enumerate(recs.items()):
        s, e, ref[reco] = X.planted_recording(reco, turns, 40 + i)
        segs += s
        emb.append(e)
    return segs, np.concatenate(emb), ref


def test_tune_threshold_on_the_device(D):
    segs, emb, ref = _planted()
    rec_off = np.array([0, sum(s[1] == "recA" for s in segs), len(segs)], dtype=np.int64)
    scores = D.score_dense(emb, rec_off, "cosine")[0]
    th = np.round(np.arange(-1.0, 1.0001, 0.05), 6)                             # K = 41
    h = D.tune_threshold(scores, segs, ref, th, backend="host")
    g = D.tune_threshold(scores, segs, ref, th, backend="hip")
    print("sweep: %d jobs of %s pieces, labels %s .. %s" % (2 * th.size, np.diff(rec_off).tolist(), g["labels"].max(axis=1).min(), g["labels"].max()))
    assert g["table"] == h["table"] and g["best_threshold"] == h["best_threshold"] and g["host_jobs"] == 0
    assert np.array_equal(g["per_recording"], h["per_recording"]) and np.array_equal(g["labels"], h["labels"])
    assert np.array_equal(g["prefix"], h["prefix"])
    small = D.tune_threshold(scores, segs, ref, th, backend="hip", ws_budget_bytes=8 * 100)
    assert small["table"] == g["table"]


def test_tune_threshold_counts_the_jobs_left_to_the_host(D, ops):
    """a recording of more windows than spk_der_max_hyp(): at a threshold of +inf every window is a label of its own"""
    n = ops.der_limits()[1] + 60
    rng = np.random.RandomState(9)
    who = (np.arange(n) // 90) % 2
    emb = np.eye(8)[who * 3] * 4 + 0.05 * rng.randn(n, 8)
    segs = [("w%05d" % i, "rec", round(0.1 * i, 2), round(0.1 * i + 0.2, 2)) for i in range(n)]
    ref = {"rec": [("s%d" % (b % 2), round(9.0 * b, 2), 9.0) for b in range(n // 90 + 1)]}
    scores = D.score_dense(emb, [0, n], "cosine", backend="hip", return_device=True)[0]
    th = [np.inf, 0.5, -np.inf]
    merges = D.cluster(scores, [0, n], backend="hip")[1:]                       # (one clustering, on the device, for both sweeps)
    g = D.tune_threshold(merges, segs, ref, th, backend="hip")
    h = D.tune_threshold(merges, segs, ref, th, backend="host")
    print("sweep: 3 jobs of %d pieces, labels %s, %d on the host" % (n, g["labels"].max(axis=1).tolist(), g["host_jobs"]))
    assert g["host_jobs"] == 1 and h["host_jobs"] == 0 and g["table"] == h["table"] and g["best_index"] == 1


def test_script_sweep_writes_the_same_bytes_on_both_back_ends(tmp_path):
    segs, emb, ref = _planted()
    d = tmp_path
    with open(str(d / "emb"), "w") as f:
        for s, v in zip(segs, emb):
            f.write(s[0] + " [ " + " ".join("%.6f" % x for x in v) + " ]\n")
    (d / "segments").write_text("".join("%s %s %.3f %.3f\n" % s for s in segs))
    (d / "ref.rttm").write_text("".join("SPEAKER %s 0 %.3f %.3f <NA> <NA> %s <NA> <NA>\n" % (r, s, dur, spk) for r, t in ref.items() for spk, s, dur in t))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    for backend in ("host", "hip"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "diarize.py"), "--embeddings", str(d / "emb"), "--segments",
                            str(d / "segments"), "--tune-threshold=-1:1:0.05", "--ref-rttm", str(d / "ref.rttm"), "--backend", backend,
                            "--out-dir", str(d / backend)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    for name in ("threshold_der", "best_threshold", "der", "labels", "rttm"):
        assert open(str(d / "host" / name), "rb").read() == open(str(d / "hip" / name), "rb").read(), name
    assert len(open(str(d / "host" / "threshold_der")).read().splitlines()) == 41
