"""Diarization scoring, host side: diarize.der, cut_merges and tune_threshold on the host back end against the
tick-by-tick restatement in tests/der_ref.py (the five integers equal), the RTTM / UEM readers' errors, scripts/compute_der.py and
scripts/diarize.py --ref-rttm --tune-threshold on files, and the exports of csrc/der.hip in the C ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import der_cases as X
import der_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def D():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


# ---- the rule -------------------------------------------------------------------------------------------------------------------------
def test_reference_on_the_hand_computed_case():
    assert der_ref.five(X.reference("hand")) == X.HAND_FIVE and X.reference("hand")["der"] == 0.375


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_host_matches_the_reference(D, name):
    got = X.check_case(D, name, "host")
    if name == "hand":
        p = got["per_recording"]["rec"]
        assert (p["scored"], p["miss"], p["fa"], p["conf"], p["opt"]) == X.HAND_FIVE and p["mapping"] == {"A": "x", "B": "y"}
    if name == "nothing_scored":
        assert got["per_recording"]["rec"]["scored"] == 0 and np.isnan(got["per_recording"]["rec"]["der"]) and np.isnan(got["total"]["der"])
    if name == "empty_hyp":
        p = got["per_recording"]["rec"]
        assert p["miss"] == p["scored"] > 0 and p["fa"] == p["conf"] == 0 and p["mapping"] == {}
    if name == "hyp_outside_S":
        assert got["per_recording"]["rec"]["fa"] == 0 and got["per_recording"]["rec"]["opt"] == 0
    if name == "tie_two_by_two":
        assert got["per_recording"]["rec"]["opt"] == 200 and got["per_recording"]["rec"]["conf"] == 200


@pytest.mark.parametrize("Sr,Sh", [(7, 9), (12, 8), (9, 30)])
def test_host_assignment_beyond_brute_force(D, Sr, Sh):
    if not der_ref.HAVE_SCIPY:
        pytest.skip("the reference solves min(Sr, Sh) > 6 with scipy")
    c = X.random_case(100 + Sr, Sr, Sh, 3 * Sr, 4 * Sh)
    want = der_ref.der(c["ref"], c["hyp"], None, c["collar"], False, X.TICK)
    p = D.der({"r": c["ref"]}, {"r": c["hyp"]}, collar=c["collar"], tick=X.TICK)["per_recording"]["r"]
    assert (p["scored"], p["miss"], p["fa"], p["conf"], p["opt"]) == der_ref.five(want)


def test_totals_and_recordings_of_one_file_only(D):
    ref = {"a": X.CASES["hand"]["ref"], "b": X.CASES["ref_overlap"]["ref"]}
    hyp = {"a": X.CASES["hand"]["hyp"]}
    got = D.der(ref, hyp, collar=0.0, tick=X.TICK)
    b = got["per_recording"]["b"]
    assert got["recordings"] == ["a", "b"] and b["miss"] == b["scored"] > 0 and b["fa"] == 0
    assert got["total"]["scored"] == X.HAND_FIVE[0] + b["scored"] and got["total"]["miss"] == 100 + b["miss"]
    assert got["total"]["der"] == (got["total"]["miss"] + 200) / got["total"]["scored"]
    with pytest.raises(ValueError, match="reference lacks.*zzz"):
        D.der(ref, {"zzz": [("x", 0.0, 1.0)]}, tick=X.TICK)
    got = D.der(ref, {"zzz": [("x", 0.0, 1.0)]}, uem={"zzz": [(0.0, 2.0)], "a": [(0.0, 8.0)], "b": [(0.0, 8.0)]}, collar=0.0, tick=X.TICK)
    z = got["per_recording"]["zzz"]
    assert (z["scored"], z["miss"], z["fa"], z["conf"]) == (0, 0, 100, 0)


def test_tick_is_a_parameter(D):
    c = X.CASES["hand"]
    a = D.der({"r": c["ref"]}, {"r": c["hyp"]}, collar=0.0, tick=0.01)["total"]
    b = D.der({"r": c["ref"]}, {"r": c["hyp"]}, collar=0.0, tick=1e-7)["total"]        # (no cost grows with 1 / tick)
    assert b["scored"] == 100000 * a["scored"] and b["conf"] == 100000 * a["conf"] and a["der"] == b["der"]
    assert D.to_ticks([0.0005, 0.00049, 1.2345], 0.001).tolist() == [1, 0, 1235]        # floor(t / tick + 0.5)


# ---- the readers ----------------------------------------------------------------------------------------------------------------------
def test_read_rttm_and_uem(D, tmp_path):
    f = tmp_path / "x.rttm"
    f.write_text("SPEAKER recA 0 0.100 1.500 <NA> <NA> 2 <NA> <NA>\n\nSPKR-INFO recA 0 <NA> <NA> <NA> unknown 2 <NA>\n"
                 "SPEAKER recB 1 3.000 0.250 <NA> <NA> spk <NA>\nSPEAKER recA 0 2.0 1.0 <NA> <NA> 1 <NA> <NA>\n")
    assert D.read_rttm(str(f)) == {"recA": [("2", 0.1, 1.5), ("1", 2.0, 1.0)], "recB": [("spk", 3.0, 0.25)]}
    for text, words in (("SPEAKER recA 0 0.1 1.5 <NA> <NA> 2 <NA> <NA>\nSPEAKER recA 0 0.1\n", ["x.rttm:2"]),
                        ("SPEAKER recA 0 zero 1.5 <NA> <NA> 2 <NA> <NA>\n", ["x.rttm:1", "numbers"]),
                        ("\nSPEAKER recA 0 1.0 -0.5 <NA> <NA> 2 <NA> <NA>\n", ["x.rttm:2", "negative"]),
                        ("SPEAKER recA 0 nan 0.5 <NA> <NA> 2 <NA> <NA>\n", ["x.rttm:1", "finite"])):
        f.write_text(text)
        with pytest.raises(ValueError) as e:
            D.read_rttm(str(f))
        assert all(w in str(e.value) for w in words), str(e.value)
    u = tmp_path / "x.uem"
    u.write_text("recA 1 0.0 10.5\nrecB 1 1.0 2.0\n\nrecA 1 20 30\n")
    assert D.read_uem(str(u)) == {"recA": [(0.0, 10.5), (20.0, 30.0)], "recB": [(1.0, 2.0)]}
    for text, words in (("recA 1 0.0\n", ["x.uem:1"]), ("recA 1 0 1\nrecA 1 a b\n", ["x.uem:2", "numbers"]),
                        ("recA 1 5.0 1.0\n", ["x.uem:1", "before it starts"])):
        u.write_text(text)
        with pytest.raises(ValueError) as e:
            D.read_uem(str(u))
        assert all(w in str(e.value) for w in words), str(e.value)


# ---- cutting the merge list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [[1], [2], [1, 7, 2], [33, 65]])
def test_cut_merges_equals_cluster_at_every_threshold(D, sizes):
    scores, rec_off, merges, cost, nm = X.merge_case(D, sizes, 7 + len(sizes))
    th = X.cut_thresholds(cost, rec_off, nm)
    got = D.cut_merges(merges, cost, nm, rec_off, th, "host")
    assert got.dtype == np.int32 and got.shape == (th.size, rec_off[-1])
    for k, t in enumerate(th):
        want = D.cluster(scores, rec_off, threshold=t)[0]
        assert np.array_equal(got[k], want), (k, t)
        for r in range(len(sizes)):
            a, b = rec_off[r], rec_off[r + 1]
            replay = der_ref.cut([tuple(m) for m in merges[a:a + nm[r]]], cost[a:a + nm[r]], sizes[r], t)
            assert got[k, a:b].tolist() == replay, (k, t, r)
    assert np.array_equal(got[-1], got[-2])                                  # the same threshold twice
    assert (got[2] == np.concatenate([np.arange(1, n + 1) for n in sizes])).all()                  # +inf: no merge
    with pytest.raises(ValueError, match="NaN"):
        D.cut_merges(merges, cost, nm, rec_off, [0.0, float("nan")])


def test_hypothesis_of_a_cut_equals_the_rttm_read_back(D):
    """windows on the 10 ms grid, tick = 1 ms: the pieces of cut_pieces cover, speaker by speaker, the ticks of read_rttm(make_rttm)"""
    rng = np.random.RandomState(3)
    for trial in range(20):
        W, t0, wins = int(rng.choice([50, 100, 150])), 0, []                  # frames of 10 ms: sliding windows over speech segments,
        P = int(rng.choice([W, W // 2, 3 * W // 5]))                         # the last window of a segment shortened to its end;
                                                                             # period >= half the window (section 6r)
        for seg in range(rng.randint(1, 4)):
            t0 += rng.randint(0, 300)
            end = t0 + rng.randint(20, 900)
            while True:
                wins.append((t0, min(t0 + W, end)))
                if t0 + W >= end:
                    break
                t0 += P
            t0 = end
        n = len(wins)
        segs = [("w%03d" % i, "rec", a / 100.0, b / 100.0) for i, (a, b) in enumerate(wins)]
        lab = rng.randint(1, 4, size=n)
        rttm = D.parse_rttm(D.make_rttm(segs, lab.tolist())).get("rec", [])
        ws, we = D.to_ticks([s[2] for s in segs]), D.to_ticks([s[3] for s in segs])
        ps, pe = D.cut_pieces(ws, we, lab)
        assert [(int(l), int(a), int(b)) for l, a, b in zip(lab, ps, pe)] == der_ref.pieces(list(zip(ws.tolist(), we.tolist())), lab.tolist())
        T = int(we.max()) + 1
        for spk in (1, 2, 3):
            a, b = np.zeros(T, bool), np.zeros(T, bool)
            for l, s, e in zip(lab, ps, pe):
                if l == spk:
                    a[s:e] = True
            for name, s, d in rttm:
                if name == str(spk):
                    b[der_ref.tick(s, 0.001):der_ref.tick(s, 0.001) + der_ref.tick(d, 0.001)] = True
            assert np.array_equal(a, b), (trial, spk)


# ---- the sweep --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    recs = {"recA": [(0, 0.0, 9.0), (1, 9.0, 18.0), (0, 18.0, 24.0), (2, 24.0, 30.0)], "recB": [(1, 0.0, 6.0), (0, 6.0, 15.0)]}
    segs, emb, ref = [], [], {}
    for i, (reco, turns) in enumerate(recs.items()):
        s, e, ref[reco] = X.planted_recording(reco, turns, 40 + i)
        segs += s
        emb.append(e)
    return segs, np.concatenate(emb), ref


def test_tune_threshold_finds_the_planted_range(D, planted):
    """(tick = 1 ms: the midpoints of 10 ms-grid windows are whole ticks, so a cut's hypothesis is its RTTM tick for tick)"""
    segs, emb, ref = planted
    rec_off = np.array([0, sum(s[1] == "recA" for s in segs), len(segs)], dtype=np.int64)
    scores = D.score_dense(emb, rec_off, "cosine")[0]
    th = np.round(np.arange(-1.0, 1.0001, 0.1), 6)
    tt = D.tune_threshold(scores, segs, ref, th)
    assert len(tt["table"]) == th.size and tt["host_jobs"] == 0
    err = [row[1] + row[2] + row[3] for row in tt["table"]]
    assert tt["best_index"] == int(np.argmin(err)) and tt["best_threshold"] == th[tt["best_index"]]
    assert 0.0 <= tt["best_threshold"] <= 0.8, tt["table"]                      # same speaker ~ 1, different speakers < 0
    assert err[0] > min(err) and err[-1] > min(err) and tt["table"][tt["best_index"]][2] == 0
    merges = D.cluster(scores, rec_off)[1:]
    t2 = D.tune_threshold(merges, segs, ref, th)                   # the merge list in place of the scores
    assert t2["table"] == tt["table"] and np.array_equal(t2["labels"], tt["labels"])
    for k in (0, tt["best_index"], th.size - 1):                               # a row of the table is der() of that cut's RTTM
        hyp = D.parse_rttm(D.make_rttm(segs, tt["labels"][k].tolist()))
        tot = D.der(ref, hyp)["total"]
        assert (tot["miss"], tot["fa"], tot["conf"], tot["scored"]) == tt["table"][k][1:5]
    assert D.tune_threshold(scores, segs, ref, [0.3, 0.3, 0.2])["best_index"] == 0      # ties: the first
    with pytest.raises(ValueError, match="reference lacks.*recB"):
        D.tune_threshold(scores, segs, {"recA": ref["recA"]}, th)


# ---- the scripts ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory, planted):
    segs, emb, ref = planted
    d = tmp_path_factory.mktemp("der_cli")
    with open(str(d / "emb"), "w") as f:
        for s, v in zip(segs, emb):
            f.write(s[0] + " [ " + " ".join("%.6f" % x for x in v) + " ]\n")
    (d / "segments").write_text("".join("%s %s %.3f %.3f\n" % s for s in segs))
    (d / "ref.rttm").write_text("".join("SPEAKER %s 0 %.3f %.3f <NA> <NA> %s <NA> <NA>\n" % (r, s, dur, spk) for r, t in ref.items() for spk, s, dur in t))
    (d / "uem").write_text("recA 0 0.0 30.0\nrecB 0 0.0 15.0\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def run(script, *flags):
        return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(flags), env=env, capture_output=True, text=True,
                              timeout=300)

    def read(out, name):
        with open(os.path.join(str(d / out), name), "rb") as f:
            return f.read()
    return {"dir": d, "run": run, "read": read, "base": ["--embeddings", str(d / "emb"), "--segments", str(d / "segments")]}


def test_scripts_end_to_end(D, files, planted):
    c, d = files, files["dir"]
    r = c["run"]("diarize.py", *c["base"], "--threshold", "0.3", "--out-dir", str(d / "plain"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(str(d / "plain"))) == ["labels", "rttm"]             # without the new flags: the files there were
    r = c["run"]("diarize.py", *c["base"], "--threshold", "0.3", "--out-dir", str(d / "scored"), "--ref-rttm", str(d / "ref.rttm"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert c["read"]("scored", "labels") == c["read"]("plain", "labels") and c["read"]("scored", "rttm") == c["read"]("plain", "rttm")
    r2 = c["run"]("compute_der.py", str(d / "ref.rttm"), str(d / "scored" / "rttm"))
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert r2.stdout.encode() == c["read"]("scored", "der")
    lines = r2.stdout.splitlines()
    assert [l.split()[0] for l in lines] == ["recA", "recB", "OVERALL"]
    want = D.der(str(d / "ref.rttm"), str(d / "scored" / "rttm"))
    assert [int(v) for v in lines[-1].split()[1:5]] == [want["total"][k] for k in ("miss", "fa", "conf", "scored")]
    assert float(lines[-1].split()[5]) == float("%.2f" % (100 * want["total"]["der"]))
    r3 = c["run"]("compute_der.py", str(d / "ref.rttm"), str(d / "scored" / "rttm"), "--uem", str(d / "uem"), "--collar", "0", "--ignore-overlap",
                  "--tick", "0.01")
    assert r3.returncode == 0 and r3.stdout != r2.stdout, r3.stderr[-2000:]
    # the sweep: the grid holds 0.3, every file is that of the best threshold
    r = c["run"]("diarize.py", *c["base"], "--tune-threshold=-1:1:0.1", "--out-dir", str(d / "tuned"), "--ref-rttm", str(d / "ref.rttm"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(str(d / "tuned"))) == ["best_threshold", "der", "labels", "rttm", "threshold_der"]
    table = [l.split() for l in c["read"]("tuned", "threshold_der").decode().splitlines()]
    best = float(c["read"]("tuned", "best_threshold"))
    assert len(table) == 21 and 0.0 <= best <= 0.8
    errs = [int(t[1]) + int(t[2]) + int(t[3]) for t in table]
    assert float(table[int(np.argmin(errs))][0]) == best
    r = c["run"]("diarize.py", *c["base"], "--threshold", "%.9g" % best, "--out-dir", str(d / "at_best"), "--ref-rttm", str(d / "ref.rttm"))
    assert r.returncode == 0, r.stderr[-2000:]
    for name in ("labels", "rttm", "der"):
        assert c["read"]("tuned", name) == c["read"]("at_best", name), name
    res = D.diarize({s[0]: v for s, v in zip(planted[0], planted[1])}, planted[0], threshold=best)
    tun = D.diarize({s[0]: v for s, v in zip(planted[0], planted[1])}, planted[0], ref=planted[2], tune=[-0.5, best, 0.95])
    assert tun["best_threshold"] == best and np.array_equal(tun["labels"], res["labels"]) and tun["rttm"] == res["rttm"]
    assert np.array_equal(tun["merges"], res["merges"]) and np.array_equal(tun["merge_cost"], res["merge_cost"])
    assert np.array_equal(tun["n_merges"], res["n_merges"]) and "der" in tun and "der" not in res and len(tun["der_table"]) == 3


def test_script_without_the_new_flags_writes_what_it_wrote_before(tmp_path):
    """tests/golden/vbx holds what scripts/diarize.py wrote for these inputs (tests/test_vbx_cpu.py's) before it could score: a plain
    run still writes those bytes and no other file, and --ref-rttm adds `der` without touching them"""
    rng = np.random.RandomState(5)
    keys, lines = [], []
    for reco, n in (("recA", 6), ("recB", 4)):
        for w in range(n):
            keys.append("%s-%08d-%08d" % (reco, 20 * w, 20 * w + 40))
            lines.append("%s %s %.3f %.3f\n" % (keys[-1], reco, 0.2 * w, 0.2 * w + 0.4))
    centres = rng.randn(2, 16) * 4
    vec = {k: centres[i % 2] + 0.1 * rng.randn(16) for i, k in enumerate(keys)}
    (tmp_path / "emb").write_text("".join(k + " [ " + " ".join("%.6f" % v for v in vec[k]) + " ]\n" for k in keys))
    (tmp_path / "segments").write_text("".join(lines))
    (tmp_path / "ref.rttm").write_text("SPEAKER recA 0 0.000 1.400 <NA> <NA> a <NA> <NA>\nSPEAKER recB 0 0.000 1.000 <NA> <NA> b <NA> <NA>\n")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    golden = os.path.join(ROOT, "tests", "golden", "vbx")
    for out, flags, names in (("plain", [], ["labels", "rttm"]), ("scored", ["--ref-rttm", str(tmp_path / "ref.rttm")], ["der", "labels", "rttm"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "diarize.py"), "--embeddings", str(tmp_path / "emb"), "--segments",
                            str(tmp_path / "segments"), "--threshold", "0.0", "--out-dir", str(tmp_path / out)] + flags, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert sorted(os.listdir(str(tmp_path / out))) == names
        for f in ("labels", "rttm"):
            assert open(str(tmp_path / out / f), "rb").read() == open(os.path.join(golden, "cosine." + f), "rb").read(), (out, f)


def test_script_errors(files):
    c, d = files, files["dir"]
    out = ["--out-dir", str(d / "never")]
    for script, flags, words in (
            ("diarize.py", c["base"] + out + ["--tune-threshold=0:1:0.1"], ["--tune-threshold", "--ref-rttm"]),
            ("diarize.py", c["base"] + out + ["--tune-threshold=0:1:0.1", "--threshold", "0", "--ref-rttm", str(d / "ref.rttm")], ["--tune-threshold", "--threshold"]),
            ("diarize.py", c["base"] + out + ["--tune-threshold=0:1", "--ref-rttm", str(d / "ref.rttm")], ["LO:HI:STEP"]),
            ("diarize.py", c["base"] + out + ["--threshold", "0", "--der-ignore-overlap"], ["--der-ignore-overlap", "--ref-rttm"]),
            ("diarize.py", c["base"] + out, ["--threshold", "--reco2num-spk"]),
            ("compute_der.py", [str(d / "ref.rttm"), str(d / "segments")[:-1] + "x"], ["segmentx"]),
            ("compute_der.py", [str(d / "ref.rttm"), str(d / "ref.rttm"), "--collar", "-1"], ["--collar"]),
            ("compute_der.py", [str(d / "ref.rttm"), str(d / "ref.rttm"), "--tick", "0"], ["--tick"])):
        r = c["run"](script, *flags)
        assert r.returncode == 2, (flags, r.stdout[-1000:] + r.stderr[-1000:])
        assert "error:" in r.stderr and all(w in r.stderr for w in words), (words, r.stderr)
    assert not os.path.exists(str(d / "never"))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
NEW = ["spk_ahc_cut_batch", "spk_der_pieces", "spk_der_max_ref", "spk_der_max_hyp", "spk_der_max_turns", "spk_der_ws_elems", "spk_der_batch"]


def test_exports_are_declared_bound_and_exported():
    """the scoring entries have a header of their own, include/spkder.h, and a binding table of their own: every name it declares is
    bound with as many parameters and exported, and include/spkhip.h and its count are as they were"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spkder.h")).read(), flags=re.S)
    decl = {m.group(2): (m.group(1), m.group(3)) for m in re.finditer(r"\b(int|long long)\s+(spk_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(decl) == sorted(NEW) == sorted(hip.der_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    main = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    for name in NEW:
        assert hasattr(hip.lib(), name) and re.search(r" T %s$" % name, nm, re.M), name
        params = [p for p in decl[name][1].split(",") if p.strip() != "void"]
        assert len(params) == len(hip._DER_SIGS[name]), name
        assert (decl[name][0] == "long long") == (getattr(hip.lib(), name).restype is ctypes.c_longlong), name
        assert name not in hip.exported_symbols() and not re.search(r"\b%s\s*\(" % name, main), name
    lib = hip.lib()
    assert lib.spk_der_max_ref() >= 64 and lib.spk_der_max_hyp() >= 1024 and lib.spk_der_max_turns() >= 8192
    assert "include/spkder.h" in open(os.path.join(ROOT, "README.md")).read()


def test_batches_are_refused_on_the_host_before_any_launch():
    """no device is needed: a refused call launches nothing and touches no pointer"""
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    lib, P = hip.lib(), 16
    arr = lambda v: np.ascontiguousarray(v, dtype=np.int64)
    ro = arr([0, 3, 5])
    assert lib.spk_ahc_cut_batch(P, P, P, arr([0, 3, 3]).ctypes.data, P, P, 1, P, 3, 2, None) < 0 and b"spk_ahc_cut_batch" in lib.spk_last_error()
    assert lib.spk_ahc_cut_batch(P, P, P, arr([0, lib.spk_ahc_max_n() + 1]).ctypes.data, P, P, 1, P, lib.spk_ahc_max_n() + 1, 1, None) < 0
    assert lib.spk_ahc_cut_batch(P, P, P, ro.ctypes.data, P, P, 0, P, 5, 2, None) < 0
    assert lib.spk_ahc_cut_batch(P, P, P, ro.ctypes.data, P, None, 1, P, 5, 2, None) < 0
    assert lib.spk_der_pieces(P, P, P, arr([0, 3, 2]).ctypes.data, P, 1, P, P, 2, 2, None) < 0 and b"spk_der_pieces" in lib.spk_last_error()
    assert lib.spk_der_pieces(P, None, P, ro.ctypes.data, P, 1, P, P, 5, 2, None) < 0
    mr, mh, mt = lib.spk_der_max_ref(), lib.spk_der_max_hyp(), lib.spk_der_max_turns()
    assert lib.spk_der_ws_elems(mt, mr, mh) == mt + mt // 2 + mr * mh and lib.spk_der_ws_elems(3, 2, 2) == 5
    for bad in ((mt + 1, 1, 1), (1, mr + 1, 1), (1, 1, mh + 1), (-1, 1, 1)):
        assert lib.spk_der_ws_elems(*bad) < 0, bad

    def der(rec_tab, jobs, ncells=4, npieces=10, ws=1 << 20, null=None):
        rt, jt = arr(rec_tab), arr(jobs)
        ptrs = [None if i == null else P for i in range(8)]
        return lib.spk_der_batch(rt.ctypes.data, ptrs[0], ptrs[1], ncells, len(rec_tab), jt.ctypes.data, ptrs[2], len(jobs), ptrs[3], ptrs[4],
                                 ptrs[5], npieces, ptrs[6], ws, ptrs[7], P, None)
    good_r, good_j = [[0, 4, 2, 0]], [[0, 0, 10, 3, 0, 0]]
    for rec_tab, jobs, kw in (([[0, 5, 2, 0]], good_j, {}), ([[0, 4, mr + 1, 0]], good_j, {}), (good_r, [[1, 0, 10, 3, 0, 0]], {}),
                              (good_r, [[0, 1, 10, 3, 0, 0]], {}), (good_r, [[0, 0, mt + 1, 3, 0, 0]], {"npieces": mt + 1}),
                              (good_r, [[0, 0, 10, mh + 1, 0, 0]], {}), (good_r, good_j, {"ws": 14}), (good_r, [[0, 0, 10, 3, -1, 0]], {}),
                              (good_r, good_j, {"null": 0}), (good_r, good_j, {"null": 3}), (good_r, good_j, {"null": 6}),
                              (good_r, good_j, {"null": 7})):
        assert der(rec_tab, jobs, **kw) < 0, (rec_tab, jobs, kw)
        assert b"spk_der_batch" in lib.spk_last_error()
