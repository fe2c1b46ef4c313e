"""Speech segments, host side: ingest.segments_from_vad against the frame-by-frame state machine of
tests/segment_ref.py on every edge of the rule, the consequences the rule implies, ingest.plan_segment_windows against plan_windows
per segment and a brute-force lister, the time rounding and the errors of decode.py --segments, decode.py's parser errors,
scripts/vad_to_segments.py --backend host, the export in the C ABI, and the synthetic recording of the end-to-end GPU test under
tests/frontend_ref.py's fbank + VAD (so that the GPU test's expectation is not vacuous)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import frontend_ref as FR
import segment_ref as S
from helpers import header_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")


@pytest.fixture(scope="module")
def ingest():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ingest
    return ingest


@pytest.fixture(scope="module")
def features():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    return features


def opts_of(features, pgm):
    return features.SegmentOptions(padding=pgm[0], max_gap=pgm[1], min_length=pgm[2])


def as_lists(res):
    assert all(a.dtype == np.int64 and a.ndim == 1 for a in res)
    return tuple(a.tolist() for a in res)


# ---- segments_from_vad ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pgm", S.OPTS)
def test_edge_rows_match_the_loop(ingest, features, pgm):
    rows = S.edge_rows()
    o = opts_of(features, pgm)
    for name, v, T in rows:                                     # one row at a time: [Tcap] and a scalar T
        want = S.segments_loop(v, T, *pgm)
        got = as_lists(ingest.segments_from_vad(v, T, o))
        assert got == ([0] * len(want), [s for s, _ in want], [e for _, e in want]), (name, pgm)
        S.check_consequences(want, min(max(T, 0), len(v)), pgm[1])
    v, T = S.pad_rows(rows)                                     # and all of them as one padded batch
    assert as_lists(ingest.segments_from_vad(v, T, o)) == S.segments_batch(v, T, *pgm)


def test_the_designed_edges_are_what_they_claim():
    """the rows built for DESIGN do hit the edges: the loop reference on them gives the segments worked out by hand"""
    p, g, m = S.DESIGN
    rows = {name: (v, T) for name, v, T in S.edge_rows()}
    loop = lambda name: S.segments_loop(*rows[name], p, g, m)
    assert loop("both_ends") == [(0, 8), (42, 50)]                              # padding clipped at 0 and at T
    assert loop("gap_g_joins") == [(7, 30 + 2 * p + g + 20 + p)]                # a - b = g: one segment
    assert loop("gap_g1_splits") == [(7, 33), (30 + p + g + 1, 30 + 2 * p + g + 1 + 20 + p)]
    assert loop("padded_overlap") == [(7, 43)]
    assert loop("exactly_m") == [(27, 27 + m)] and loop("m_minus_1") == []
    assert loop("dropped_between") == [(7, 43), (107, 153)]                     # the one-frame run in the middle: 7 frames, dropped
    assert loop("dropped_first_last") == [(47, 93)]
    assert loop("other_values") == [(2, 33), (57, 103)]
    assert loop("three_chunks") == [(47, 50 + 3 * 64 + 5 + p), (297, 333)]
    assert loop("voiced_past_T") == [(0, 700)] and loop("T_beyond_Tcap") == [(7, 100)] and loop("T_negative") == []
    assert len(S.segments_loop(*rows["alt1025"], 0, 0, 1)) == 513 == -(-1025 // 2)       # the count bound is attained
    assert S.segments_loop(*rows["voiced64"], p, g, m) == [(0, 64)] and S.segments_loop(*rows["voiced1"], 0, 0, 1) == [(0, 1)]


def test_random_rows_match_the_loop(ingest, features):
    rng = np.random.RandomState(17)
    rows = S.random_rows(200, seed=4)
    nonempty = 0
    for name, v, T in rows:
        pgm = (int(rng.choice([0, 1, 7])), int(rng.choice([0, 1, 30])), int(rng.choice([1, 2, 50])))
        want = S.segments_loop(v, T, *pgm)
        got = as_lists(ingest.segments_from_vad(v, T, opts_of(features, pgm)))
        assert got[1:] == ([s for s, _ in want], [e for _, e in want]), (name, pgm)
        S.check_consequences(want, T, pgm[1])
        nonempty += bool(want)
    assert nonempty > 100
    v, T = S.pad_rows(rows)
    for pgm in ((0, 0, 1), (7, 30, 50), (1, 1, 2)):
        assert as_lists(ingest.segments_from_vad(v, T, opts_of(features, pgm))) == S.segments_batch(v, T, *pgm)


def test_segment_options_and_argument_errors(ingest, features):
    d = features.SegmentOptions()
    assert (d.padding, d.max_gap, d.min_length) == (10, 30, 50)
    for kw in (dict(padding=-1), dict(max_gap=-1), dict(min_length=0)):
        with pytest.raises(ValueError):
            features.SegmentOptions(**kw)
    with pytest.raises(ValueError, match="rows"):
        ingest.segments_from_vad(np.zeros((2, 5)), [5], d)
    with pytest.raises(ValueError):
        ingest.segments_from_vad(np.zeros((2, 5, 1)), [5, 5], d)
    with pytest.raises(ValueError, match="vad"):
        features.Frontend(features.FbankOptions(), vad=None, segments=d)
    row, start, end = ingest.segments_from_vad(np.zeros((0, 7)), [], d)
    assert row.size == start.size == end.size == 0


# ---- plan_segment_windows --------------------------------------------------------------------------------------------------------------
SEG_UTT = [0, 0, 0, 2, 2, 3, 5]
SEG_START = [0, 40, 100, 7, 60, 0, 11]
SEG_END = [40, 55, 230, 60, 64, 1, 300]           # touching segments (40 | 40, 60 | 60), short ones (15, 4, 1 frames), no utterance 1, 4


@pytest.mark.parametrize("W,P,M", [(48, 24, 16), (24, 24, 24), (24, 8, 1), (60, 30, 5), (8, 11, 2)])
def test_plan_segment_windows(ingest, W, P, M):
    p = ingest.plan_segment_windows(SEG_UTT, SEG_START, SEG_END, W, P, M)
    assert all(a.dtype == np.int64 for a in p)
    utt, start, length, seg, skipped = S.segment_windows(SEG_UTT, SEG_START, SEG_END, W, P, M)
    assert (p.utt.tolist(), p.start.tolist(), p.length.tolist(), p.seg.tolist(), p.skipped.tolist()) == (utt, start, length, seg, skipped)
    assert skipped == [j for j in range(len(SEG_UTT)) if SEG_END[j] - SEG_START[j] < M]
    for j in range(len(SEG_UTT)):                    # per segment: plan_windows of its length, plus the offset
        one = ingest.plan_windows([SEG_END[j] - SEG_START[j]], W, P, M)
        sel = p.seg == j
        assert (p.start[sel] - SEG_START[j]).tolist() == one.start.tolist() and p.length[sel].tolist() == one.length.tolist()
        assert (p.utt[sel] == SEG_UTT[j]).all() and (one.skipped.size == 1) == (j in skipped)
        assert (p.start[sel] >= SEG_START[j]).all() and (p.start[sel] + p.length[sel] <= SEG_END[j]).all()
    assert (np.diff(p.seg) >= 0).all() and (np.diff(p.utt) >= 0).all()


def test_plan_segment_windows_refusals(ingest):
    ok = ingest.plan_segment_windows([], [], [], 8, 8, 1)
    assert ok.utt.size == 0 and ok.skipped.size == 0
    for u, s, e, word in (([1, 0], [0, 0], [5, 5], "segment 1"),               # seg_utt decreases
                          ([0, 0], [0, 4], [5, 9], "segment 1"),               # overlap within an utterance
                          ([0, 0], [10, 0], [20, 5], "segment 1"),             # not ascending
                          ([0, 1], [-1, 0], [5, 5], "segment 0"),              # start < 0
                          ([0, 1], [0, 5], [5, 5], "segment 1"),               # end == start
                          ([0, 1], [0, 7], [5, 5], "segment 1")):              # end < start
        with pytest.raises(ValueError, match=word):
            ingest.plan_segment_windows(u, s, e, 8, 8, 1)
    with pytest.raises(ValueError):
        ingest.plan_segment_windows([0], [0, 1], [5], 8, 8, 1)
    with pytest.raises(ValueError):
        ingest.plan_segment_windows([0], [0], [5], 8, 8, 9)                    # plan_windows' own refusal


# ---- decode.py --segments: times, file errors -------------------------------------------------------------------------------------------
def test_time_to_frame_rounds_half_up(ingest):
    for k in range(0, 4000, 7):                      # t = k frames + half a frame, as text and as a float: always k + 1
        text = "%d.%02d5" % (k // 100, k % 100)
        assert ingest.time_to_frame(text, 0.01) == k + 1, text
        assert ingest.time_to_frame(float(text), 0.01) == k + 1, text
        assert ingest.time_to_frame("%d.%02d4999" % (k // 100, k % 100), 0.01) == k
        assert ingest.time_to_frame("%.3f" % (k * 0.01), 0.01) == k           # what decode.py writes reads back as the frame
    assert ingest.time_to_frame("0.03", 0.02) == 2 and ingest.time_to_frame("0.029", 0.02) == 1 and ingest.time_to_frame("0", 0.01) == 0
    assert ingest.time_to_frame("1e-2", 0.01) == 1


def test_read_segments_file(ingest, tmp_path):
    f = tmp_path / "segments"
    f.write_text("b-2 recB 1.005 2.0\n\na-1 recA 0.1 0.5\nb-1 recB 0.0 1.005\n")
    got = ingest.read_segments_file(str(f), ["recA", "recB", "recC"], 0.01)
    assert sorted(got) == ["recA", "recB"]
    assert got["recB"][0].tolist() == [0, 101] and got["recB"][1].tolist() == [101, 200] and got["recA"][0].tolist() == [10]
    for text, words in (("a recA 0.1 0.5\nx recZ 0 1\n", ["segments:2", "recZ"]),
                        ("a recA 0.1 0.5\nb recA 0.494 0.9\n", ["segments:1", "segments:2", "overlap"]),
                        ("a recA 0.1 0.5\nb recA 0.701 0.704\n", ["segments:2", "empty"]),
                        ("a recA 0.5 0.1\n", ["segments:1", "empty"]),
                        ("a recA 0.1\n", ["segments:1"]),
                        ("a recA zero one\n", ["segments:1", "numbers"])):
        f.write_text(text)
        with pytest.raises(ValueError) as e:
            ingest.read_segments_file(str(f), ["recA", "recB"], 0.01)
        assert all(w in str(e.value) for w in words), str(e.value)


# ---- parser errors ----------------------------------------------------------------------------------------------------------------------
def _decode(*flags):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--arch", "resnet18", "--input-dim", "40", "--pooling", "mean+std"]
    return subprocess.run(cmd + list(flags), env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("segment_parser")
    (d / "wav.scp").write_text("recA /nowhere/a.wav\nrecB /nowhere/b.wav\n")
    (d / "good").write_text("a recA 0.0 1.0\n")
    (d / "absent").write_text("a recA 0.0 1.0\nb recQ 0.0 1.0\n")
    (d / "overlap").write_text("a recA 0.0 1.0\nb recB 0.0 1.0\nc recA 0.99 2.0\n")
    (d / "empty").write_text("a recA 0.0 1.0\nb recA 1.001 1.004\n")
    return {k: str(d / k) for k in ("wav.scp", "good", "absent", "overlap", "empty")}


VADCONF = os.path.join(FB, "vad.conf")


@pytest.mark.parametrize("flags,words", [
    (["--vad-segments", "--wav-scp", "WAV", "--window", "24"], ["--vad-segments", "--vad-config"]),
    (["--vad-segments", "--wav-scp", "WAV", "--vad-config", VADCONF], ["--vad-segments", "--window"]),
    (["--vad-segments", "--native-reader", "--pad-batches", "--window", "24"], ["--vad-segments", "--wav-scp"]),
    (["--wav-scp", "WAV", "--vad-config", VADCONF, "--window", "24", "--seg-padding", "3"], ["--seg-padding", "--vad-segments"]),
    (["--wav-scp", "WAV", "--vad-config", VADCONF, "--window", "24", "--seg-max-gap", "3"], ["--seg-max-gap", "--vad-segments"]),
    (["--wav-scp", "WAV", "--window", "24", "--seg-min-length", "3"], ["--seg-min-length", "--vad-segments"]),
    (["--wav-scp", "WAV", "--vad-config", VADCONF, "--window", "24", "--vad-segments", "--seg-min-length", "0"], ["--vad-segments", "min_length"]),
    (["--wav-scp", "WAV", "--vad-config", VADCONF, "--window", "24", "--vad-segments", "--seg-padding", "-1"], ["--vad-segments", "padding"]),
    (["--segments", "GOOD", "--wav-scp", "WAV"], ["--segments", "--window"]),
    (["--segments", "GOOD", "--native-reader", "--pad-batches", "--window", "24"], ["--segments", "--wav-scp"]),
    (["--segments", "GOOD", "--wav-scp", "WAV", "--window", "24", "--vad-config", VADCONF], ["--segments", "--vad-config", "mutually exclusive"]),
    (["--segments", "GOOD", "--wav-scp", "WAV", "--window", "24", "--vad-config", VADCONF, "--vad-segments"],
     ["--segments", "--vad-segments", "mutually exclusive"]),
    (["--segments", "ABSENT", "--wav-scp", "WAV", "--window", "24"], ["--segments", "absent:2", "recQ"]),
    (["--segments", "OVERLAP", "--wav-scp", "WAV", "--window", "24"], ["--segments", "overlap:1", "overlap:3", "recA"]),
    (["--segments", "EMPTY", "--wav-scp", "WAV", "--window", "24"], ["--segments", "empty:2", "empty after rounding"]),
    (["--segments", "/nowhere/segments", "--wav-scp", "WAV", "--window", "24"], ["--segments", "/nowhere/segments"]),
])
def test_decode_parser_errors(files, flags, words):
    sub = {"WAV": files["wav.scp"], "GOOD": files["good"], "ABSENT": files["absent"], "OVERLAP": files["overlap"], "EMPTY": files["empty"]}
    r = _decode(*[sub.get(f, f) for f in flags])
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "error:" in r.stderr and all(w in r.stderr for w in words), r.stderr


def test_decode_help_names_the_new_flags():
    r = _decode("--help")
    assert r.returncode == 0
    text = " ".join(r.stdout.split())
    for flag in ("--vad-segments", "--seg-padding", "--seg-max-gap", "--seg-min-length", "--segments", "speech_segments"):
        assert flag in text, flag


# ---- scripts/vad_to_segments.py --backend host -----------------------------------------------------------------------------------------
def test_vad_to_segments_host(tmp_path):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import kaldi_io
    rows = {"recA": S._row(300, [(20, 90), (100, 130), (200, 280)]), "recB": S._row(120, [(0, 3), (60, 120)]), "recC": np.zeros(80, np.int32)}
    ark, scp = str(tmp_path / "vad.ark"), str(tmp_path / "vad.scp")
    with open(ark, "wb") as f, open(scp, "w") as s:
        for k, v in rows.items():
            f.write((k + " ").encode())
            off = f.tell()
            kaldi_io.write_vec_flt(f, v.astype(np.float32))
            s.write("%s %s:%d\n" % (k, ark, off))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    script = os.path.join(ROOT, "scripts", "vad_to_segments.py")

    def run(out, *flags):
        r = subprocess.run([sys.executable, script, scp, str(tmp_path / out), "--backend", "host"] + list(flags), env=env,
                           capture_output=True, text=True, timeout=300)
        return r, (open(str(tmp_path / out)).read() if r.returncode == 0 else None)

    r, text = run("seg_default")
    assert r.returncode == 0, r.stderr[-1000:]
    # defaults (10, 30, 50): recA's runs pad to [10, 140) (gap 10 - 20 < 30: joined) and [190, 290); recB's [0, 13) is dropped
    assert text == ("recA-00000010-00000140 recA 0.100 1.400\nrecA-00000190-00000290 recA 1.900 2.900\n"
                    "recB-00000050-00000120 recB 0.500 1.200\n")
    assert "3 segments of 3 recordings" in r.stdout
    r, text = run("seg_tight", "--seg-padding", "0", "--seg-max-gap", "9", "--seg-min-length", "3", "--frame-shift", "0.02")
    want = ["recA-%08d-%08d recA %.3f %.3f\n" % (s, e, s * 0.02, e * 0.02) for s, e in S.segments_loop(rows["recA"], 300, 0, 9, 3)]
    want += ["recB-%08d-%08d recB %.3f %.3f\n" % (s, e, s * 0.02, e * 0.02) for s, e in S.segments_loop(rows["recB"], 120, 0, 9, 3)]
    assert text == "".join(want) and len(want) == 5
    r, _ = run("seg_bad", "--seg-min-length", "0")
    assert r.returncode == 2 and "min_length" in r.stderr


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_export_is_declared_bound_and_exported():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import hip
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    name = "spk_vad_segments"
    assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name)
    params = header_params(name)
    assert params == ["vad", "T", "B", "Tcap", "padding", "max_gap", "min_length", "seg", "Scap", "nseg", "stream"]
    assert len(params) == len(hip._SIGS[name])
    assert len(hip.exported_symbols()) == 128 and "(128 exports)" in open(os.path.join(ROOT, "README.md")).read()
    # the refusals need no device: nothing is launched (a refused call touches no pointer)
    lib, P = hip.lib(), 16
    for B, Tcap, p, g, m, Scap in ((-1, 8, 0, 0, 1, 4), (1, -1, 0, 0, 1, 4), (1, 8, -1, 0, 1, 4), (1, 8, 0, -1, 1, 4), (1, 8, 0, 0, 0, 4),
                                   (1, 8, 0, 0, 1, -1)):
        assert lib.spk_vad_segments(P, P, B, Tcap, p, g, m, P, Scap, P, None) < 0, (B, Tcap, p, g, m, Scap)
        assert b"spk_vad_segments" in lib.spk_last_error()
    for null in range(4):
        ptrs = [None if i == null else P for i in range(4)]
        assert lib.spk_vad_segments(ptrs[0], ptrs[1], 1, 8, 0, 0, 1, ptrs[2], 4, ptrs[3], None) < 0, null
    assert lib.spk_vad_segments(None, None, 0, 8, 0, 0, 1, None, 4, None, None) == 0            # B == 0: nothing to do, no launch


# ---- the synthetic recording of the end-to-end GPU test -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.RECORDINGS))
def test_the_synthetic_recording_has_the_planted_runs(features, name):
    lead, tail, seed = S.RECORDINGS[name]
    x, bursts = S.burst_recording(lead, tail, seed)
    assert len(bursts) == S.NBURST == 4 and all(e - s == 120 for s, e in bursts)
    assert all(s1 - e0 == 80 for (_, e0), (s1, _) in zip(bursts, bursts[1:]))
    fb = features.FbankOptions.from_kaldi_config(os.path.join(FB, "fbank.conf"))
    vo = features.VadOptions.from_kaldi_config(VADCONF)
    kw = {k: getattr(fb, k) for k in FR.DEFAULTS}
    L = FR.frame_params(fb.sample_frequency, fb.frame_length, fb.frame_shift)[0]
    T = FR.num_frames(len(x), L, S.SHIFT, fb.snip_edges)
    noise = np.random.RandomState(1).randn(T, L)                 # a dither stream: the silences are noise at amplitude 1, not zeros
    _, loge = FR.fbank(x.astype(np.float64), noise=noise, **kw)
    assert len(loge) == T
    v = FR.vad(loge, vo.vad_energy_threshold, vo.vad_energy_mean_scale, vo.vad_frames_context, vo.vad_proportion_threshold)
    runs = S.segments_loop(v, T, 0, 0, 1)                        # no padding, no joining, no dropping: the voiced runs themselves
    assert len(runs) == len(bursts), (runs, bursts)
    tol = vo.vad_frames_context + 2
    for (s, e), (bs, be) in zip(runs, bursts):
        assert abs(s - bs) <= tol and abs(e - be) <= tol, (runs, bursts)
    # and under the default options every burst is a segment of its own
    d = features.SegmentOptions()
    segs = S.segments_loop(v, T, d.padding, d.max_gap, d.min_length)
    assert len(segs) == 4
    assert all(abs(s - max(bs - d.padding, 0)) <= tol and abs(e - min(be + d.padding, T)) <= tol for (s, e), (bs, be) in zip(segs, bursts))
