"""Speech segments on the GPU (csrc/frontend.hip: spk_vad_segments, features.vad_segments, Engine.predict_windows(segments=...),
decode.py --vad-segments / --segments) against tests/segment_ref.py.

The kernel works on integers only, so every comparison with the frame-by-frame state machine is for equality.  predict_windows:
every row against predict() of its window run alone, by the bar tests/test_window_gpu.py applies (section 6d: 1 - cos < 1e-6,
scale-relative error < 2e-5).  End to end: two synthetic recordings of noise bursts between silences through decode.py; the bursts
are planted, tests/test_segment_cpu.py shows that the reference VAD finds exactly them."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import half_ref as H  # noqa: E402
import segment_ref as S  # noqa: E402
import window_ref as WR  # noqa: E402
from test_half_gpu import make_model  # noqa: E402
from test_masked_predict_gpu import _read_vectors, close  # noqa: E402
from test_window_gpu import same_as_alone  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")
GUARD = -7          # what the output buffers hold before a launch


@pytest.fixture(scope="module")
def pk():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features, hip, ingest
    return {"features": features, "hip": hip, "ingest": ingest}


@pytest.fixture(scope="module")
def rows():
    """every edge row and 60 random ones, as one padded batch on the device"""
    r = S.edge_rows() + S.random_rows(60, seed=9, tmax=1400)
    v, T = S.pad_rows(r)
    return {"rows": r, "v": v, "T": T, "vg": torch.from_numpy(v).cuda(), "tg": torch.from_numpy(T.astype(np.int32)).cuda(), "ref": {}}


def reference(rows, pgm):
    if pgm not in rows["ref"]:
        rows["ref"][pgm] = [S.segments_loop(rows["v"][b], rows["T"][b], *pgm) for b in range(len(rows["rows"]))]
    return rows["ref"][pgm]


def launch(hip, vg, tg, pgm, Scap, tail=16):
    """one launch into buffers pre-filled with GUARD; seg has `tail` guard words behind the [B][Scap][2] array.  -> (rc, seg, nseg)"""
    B, Tcap = vg.shape
    seg = torch.full((B * Scap * 2 + tail,), GUARD, dtype=torch.int32, device="cuda")
    nseg = torch.full((B,), GUARD, dtype=torch.int32, device="cuda")
    rc = hip.lib().spk_vad_segments(hip.ptr(vg), hip.ptr(tg), B, Tcap, pgm[0], pgm[1], pgm[2], hip.ptr(seg), Scap, hip.ptr(nseg),
                                    hip.stream())
    torch.cuda.synchronize()
    return rc, seg.cpu().numpy(), nseg.cpu().numpy()


def check_against(ref, seg, nseg, Scap, tail=16):
    """nseg is the true count; the first min(nseg, Scap) pairs are the reference's; every other word still holds GUARD"""
    B = len(ref)
    assert nseg.tolist() == [len(r) for r in ref]
    body = seg[:B * Scap * 2].reshape(B, Scap, 2)
    for b, r in enumerate(ref):
        n = min(len(r), Scap)
        assert body[b, :n].tolist() == [list(p) for p in r[:n]], b
        assert (body[b, n:] == GUARD).all(), b
    assert (seg[B * Scap * 2:] == GUARD).all() and seg.size == B * Scap * 2 + tail


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pgm", S.OPTS)
def test_kernel_matches_the_loop_in_one_mixed_launch(pk, rows, pgm):
    ref = reference(rows, pgm)
    Scap = max(len(r) for r in ref)
    rc, seg, nseg = launch(pk["hip"], rows["vg"], rows["tg"], pgm, Scap)
    assert rc == 0
    check_against(ref, seg, nseg, Scap)
    if pgm == (0, 0, 1):            # the maximum count: every second frame of 1025 opens a segment of its own
        b = [name for name, _, _ in rows["rows"]].index("alt1025")
        assert nseg[b] == 513 == -(-1025 // 2) <= Scap


@pytest.mark.parametrize("Scap", [0, 1, 3, 64])
def test_capacity_smaller_than_the_count(pk, rows, Scap):
    pgm = (0, 0, 1)
    ref = reference(rows, pgm)
    assert max(len(r) for r in ref) > 64 and min(len(r) for r in ref) == 0
    rc, seg, nseg = launch(pk["hip"], rows["vg"], rows["tg"], pgm, Scap)
    assert rc == 0
    check_against(ref, seg, nseg, Scap)


def test_no_output_array_at_capacity_zero(pk, rows):
    hip, pgm = pk["hip"], S.DESIGN
    B, Tcap = rows["vg"].shape
    nseg = torch.full((B,), GUARD, dtype=torch.int32, device="cuda")
    rc = hip.lib().spk_vad_segments(hip.ptr(rows["vg"]), hip.ptr(rows["tg"]), B, Tcap, *pgm, None, 0, hip.ptr(nseg), hip.stream())
    assert rc == 0 and nseg.cpu().tolist() == [len(r) for r in reference(rows, pgm)]


def test_rows_permuted_split_and_repeated_give_the_same_bits(pk, rows):
    hip, pgm = pk["hip"], S.DESIGN
    Scap = 40
    rc, seg, nseg = launch(hip, rows["vg"], rows["tg"], pgm, Scap, tail=0)
    rc2, seg2, nseg2 = launch(hip, rows["vg"], rows["tg"], pgm, Scap, tail=0)
    assert rc == rc2 == 0 and np.array_equal(seg, seg2) and np.array_equal(nseg, nseg2)          # two runs
    B = len(rows["rows"])
    perm = np.random.RandomState(5).permutation(B)
    pg = torch.from_numpy(perm).cuda()
    seg, seg_p = seg.reshape(B, Scap, 2), np.full((B, Scap, 2), GUARD - 1, dtype=np.int32)
    nseg_p = np.full(B, GUARD - 1, dtype=np.int32)
    for part in (perm[:B // 3], perm[B // 3:]):                                                  # two launches of permuted rows
        sel = torch.from_numpy(part).cuda()
        rc, s, n = launch(hip, rows["vg"][sel].contiguous(), rows["tg"][sel].contiguous(), pgm, Scap, tail=0)
        assert rc == 0
        seg_p[part], nseg_p[part] = s.reshape(len(part), Scap, 2), n
    assert np.array_equal(seg_p, seg) and np.array_equal(nseg_p, nseg) and pg.numel() == B


def test_refusals_touch_nothing(pk, rows):
    hip = pk["hip"]
    vg, tg = rows["vg"][:4].contiguous(), rows["tg"][:4].contiguous()
    B, Tcap = vg.shape
    seg = torch.full((B * 8 * 2,), GUARD, dtype=torch.int32, device="cuda")
    nseg = torch.full((B,), GUARD, dtype=torch.int32, device="cuda")
    P = hip.ptr
    bad = [(P(vg), P(tg), -1, Tcap, 0, 0, 1, P(seg), 8, P(nseg)), (P(vg), P(tg), B, -1, 0, 0, 1, P(seg), 8, P(nseg)),
           (P(vg), P(tg), B, Tcap, -1, 0, 1, P(seg), 8, P(nseg)), (P(vg), P(tg), B, Tcap, 0, -1, 1, P(seg), 8, P(nseg)),
           (P(vg), P(tg), B, Tcap, 0, 0, 0, P(seg), 8, P(nseg)), (P(vg), P(tg), B, Tcap, 0, 0, 1, P(seg), -1, P(nseg)),
           (None, P(tg), B, Tcap, 0, 0, 1, P(seg), 8, P(nseg)), (P(vg), None, B, Tcap, 0, 0, 1, P(seg), 8, P(nseg)),
           (P(vg), P(tg), B, Tcap, 0, 0, 1, None, 8, P(nseg)), (P(vg), P(tg), B, Tcap, 0, 0, 1, P(seg), 8, None)]
    for args in bad:
        assert hip.lib().spk_vad_segments(*args, hip.stream()) < 0, args[2:7]
        assert b"spk_vad_segments" in hip.lib().spk_last_error()
    assert hip.lib().spk_vad_segments(P(vg), P(tg), 0, Tcap, 0, 0, 1, P(seg), 8, P(nseg), hip.stream()) == 0      # B == 0: no launch
    torch.cuda.synchronize()
    assert (seg.cpu() == GUARD).all() and (nseg.cpu() == GUARD).all()
    with pytest.raises(RuntimeError, match=r"spk_vad_segments failed \(rc=-1\)"):
        hip.call("spk_vad_segments", P(vg), P(tg), B, Tcap, 0, 0, 0, P(seg), 8, P(nseg), hip.stream())


# ---- features.vad_segments ------------------------------------------------------------------------------------------------------------
def test_vad_segments_relaunches_for_a_row_with_more_than_the_first_capacity(pk):
    features, ingest = pk["features"], pk["ingest"]
    T = 2 * features.SEGMENT_CAP + 301
    v = np.zeros((3, T), dtype=np.int32)
    v[0, ::2] = 1                                   # 1 0 1 0 ...: ceil(T / 2) segments under (0, 0, 1), more than SEGMENT_CAP
    v[1, 100:400] = 5
    v[2, 7:T:9] = 1
    lengths = [T, 500, T - 64]
    o = features.SegmentOptions(padding=0, max_gap=0, min_length=1)
    got = features.vad_segments(torch.from_numpy(v).cuda(), lengths, o)
    want = ingest.segments_from_vad(v, lengths, o)
    assert all(g.dtype == np.int64 and np.array_equal(g, w) for g, w in zip(got, want))
    assert (got[0] == 0).sum() == -(-T // 2) > features.SEGMENT_CAP and (got[0] == 1).sum() == 1
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist()) == S.segments_batch(v, lengths, 0, 0, 1)
    empty = features.vad_segments(torch.zeros(2, 50, dtype=torch.int32, device="cuda"), [50, 50], o)
    assert all(e.size == 0 and e.dtype == np.int64 for e in empty)
    with pytest.raises(ValueError):
        features.vad_segments(torch.zeros(2, 50, device="cuda"), [50, 50], o)                    # not int32


@pytest.fixture(scope="module")
def recordings():
    """the synthetic recordings of segment_ref: samples, planted bursts, and the batch on the device"""
    rec = {name: S.burst_recording(*S.RECORDINGS[name]) for name in sorted(S.RECORDINGS)}
    names = sorted(rec)
    n = np.array([len(rec[k][0]) for k in names], dtype=np.int64)
    w = np.zeros((len(names), int(n.max())), dtype=np.float32)
    for b, k in enumerate(names):
        w[b, :n[b]] = rec[k][0]
    return {"names": names, "rec": rec, "wave": torch.from_numpy(w).cuda(), "nsamp": n}


def gpu_vad(features, recordings):
    """the VAD decisions the front end makes for the synthetic recordings, as decode.py computes them (seed 0, keyed dither)"""
    fb = features.FbankOptions.from_kaldi_config(os.path.join(FB, "fbank.conf"))
    vo = features.VadOptions.from_kaldi_config(os.path.join(FB, "vad.conf"))
    ids = [features.utt_id(k) for k in recordings["names"]]
    feats, T, loge = features.fbank(recordings["wave"], recordings["nsamp"], fb, ids, seed=0)
    v, _, _ = features.vad(loge, T, vo)
    return fb, vo, np.asarray(T, dtype=np.int64), v


def test_vad_segments_on_a_real_vad(pk, recordings):
    features, ingest = pk["features"], pk["ingest"]
    fb, vo, T, v = gpu_vad(features, recordings)
    for o in (features.SegmentOptions(), features.SegmentOptions(padding=0, max_gap=0, min_length=1)):
        got = features.vad_segments(v, T, o)
        want = ingest.segments_from_vad(v.cpu().numpy(), T, o)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert (got[0] == 0).sum() == (got[0] == 1).sum() == S.NBURST            # the voiced runs are the planted bursts
    # Frontend(segments=...): all frames, the sliding CMN over all of them, lengths = T, and these segments
    cmn = features.CmnOptions(cmn_window=300)
    ids = [features.utt_id(k) for k in recordings["names"]]
    feats, lengths, segs = features.Frontend(fb, vo, cmn, segments=features.SegmentOptions())(recordings["wave"], recordings["nsamp"], ids, 0)
    plain, T2 = features.Frontend(fb, None, cmn)(recordings["wave"], recordings["nsamp"], ids, 0)
    assert np.array_equal(lengths, T) and np.array_equal(T2, T) and torch.equal(feats, plain)
    want = ingest.segments_from_vad(v.cpu().numpy(), T, features.SegmentOptions())
    assert all(np.array_equal(g, w) for g, w in zip(segs, want)) and len(segs[0]) == 2 * S.NBURST
    old = features.Frontend(fb, vo, cmn)(recordings["wave"], recordings["nsamp"], ids, 0)
    assert len(old) == 2 and old[0].shape[2] == int(v.sum(dim=1).max())     # without `segments`: the voiced frames, as before


# ---- predict_windows(segments=...) ----------------------------------------------------------------------------------------------------
LENGTHS = (200, 150, 90)
SEG = ([0, 0, 0, 0, 1], [0, 60, 111, 120, 30], [60, 110, 119, 200, 150])       # several in utterance 0 (one of 8 frames: shorter than M;
W_, P_, M_ = 48, 24, 16                                                         # one ends at lengths[0]), one in 1 (ends at lengths[1]), none in 2


@pytest.fixture(scope="module")
def r18():
    from oracle import weights as OW
    case = H.CASES["r18_s21"]
    m, npst = make_model(case)
    x = torch.from_numpy(OW.make_input(23, 3, case[2], 200, H.SPK_NUM)[0]).clone()
    assert tuple(x.shape) == (3, 40, 200)
    for b, l in enumerate(LENGTHS):
        x[b, :, l:] = float("nan")
    xg = x.cuda()
    with torch.no_grad():
        emb, utt, start, length = m.predict_windows(xg, list(LENGTHS), W_, P_, M_, segments=SEG)
        skipped = m.engine().windows_skipped.tolist()
    return {"m": m, "xg": xg, "emb": emb.cpu(), "plan": (utt, start, length), "skipped": skipped}


def test_predict_windows_in_segments_rows_are_the_windows_run_alone(r18):
    utt, start, length = r18["plan"]
    want = S.segment_windows(*SEG, W_, P_, M_)
    assert (utt.tolist(), start.tolist(), length.tolist()) == want[:3] and r18["skipped"] == want[4] == [2]
    assert all(a.dtype == np.int64 for a in r18["plan"]) and 2 not in utt and (start + length).max() == 200
    emb, m, xg = r18["emb"], r18["m"], r18["xg"]
    assert emb.shape == (len(utt), 256) and bool(torch.isfinite(emb).all())
    with torch.no_grad():
        for i, (b, s, l) in enumerate(zip(utt, start, length)):
            solo = m.predict(xg[b:b + 1, :, s:s + l].contiguous()).cpu()
            assert same_as_alone(emb[i:i + 1], solo), (i, b, s, l)


def test_predict_windows_in_segments_average_half_and_errors(r18):
    m, xg = r18["m"], r18["xg"]
    utt, start, length = r18["plan"]
    with torch.no_grad():
        avg, uu = m.predict_windows(xg, list(LENGTHS), W_, P_, M_, average=True, segments=SEG)
        assert uu.tolist() == [0, 1] and m.engine().windows_skipped.tolist() == [2]
        uniq, first = np.unique(utt, return_index=True)
        want, bound = WR.mean_ref(r18["emb"].numpy(), np.append(first, len(utt)), length)       # all windows of the utterance
        assert (np.abs(avg.cpu().numpy().astype(np.float64) - want) <= bound).all()
        emb16, u16, s16, l16 = m.predict_windows(xg, list(LENGTHS), W_, P_, M_, precision="f16", segments=SEG)
        ovf = m.engine().half_overflow
        assert ovf.dtype == torch.int32 and ovf.cpu().tolist() == [0] * len(utt)                 # one count per window
        assert (u16.tolist(), s16.tolist(), l16.tolist()) == (utt.tolist(), start.tolist(), length.tolist())
        assert bool(torch.isfinite(emb16).all()) and emb16.shape == (len(utt), 256)
        for bad in (([0], [100], [201]), ([1], [100], [151]), ([3], [0], [10]), ([-1], [0], [10]), ([0, 0], [0, 30], [40, 60]),
                    ([1, 0], [0, 0], [40, 40]), ([0], [10], [10])):
            with pytest.raises(ValueError):
                m.predict_windows(xg, list(LENGTHS), W_, P_, M_, segments=bad)
        emb0, utt0, _, _ = m.predict_windows(xg, list(LENGTHS), W_, P_, M_, segments=([], [], []))
        assert emb0.shape == (0, 256) and utt0.size == 0


# ---- end to end: decode.py --vad-segments / --segments, diarize.py -----------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(tmp_path_factory, recordings):
    import wave
    d = tmp_path_factory.mktemp("segment_e2e")
    lines = []
    for k in recordings["names"]:
        p = str(d / (k + ".wav"))
        with wave.open(p, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(S.RATE)
            wf.writeframes(recordings["rec"][k][0].tobytes())
        lines.append("%s %s\n" % (k, p))
    scp = str(d / "wav.scp")
    open(scp, "w").writelines(lines)
    case = H.CASES["r18_s21"]
    m, _ = make_model(case)
    ckpt = str(d / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT

    def decode(tag, *flags):
        out = str(d / tag)
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(H.SPK_NUM), "--arch", case[0],
               "--input-dim", str(case[2]), "--pooling", case[5], "--model-path", ckpt, "--wav-scp", scp, "--out-path", out,
               "--batch-size", "8", "--fbank-config", os.path.join(FB, "fbank.conf"), "--cmn-window", "300", "--window", "60",
               "--period", "30"]
        r = subprocess.run(cmd + list(flags), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return out, r

    vadconf = os.path.join(FB, "vad.conf")
    out, r = decode("vadseg", "--vad-config", vadconf, "--vad-segments")
    return {"decode": decode, "dir": d, "out": out, "r": r, "vadconf": vadconf, "model": m, "env": env}


def read_segments(path):
    """[(key, recording, start frame, end frame)] of a segments file written with --frame-shift 0.01; the key restates the frames"""
    out = []
    for line in open(path):
        key, rec, t0, t1 = line.split()
        name, s, e = key.rsplit("-", 2)
        assert name == rec and t0 == "%.3f" % (int(s) * 0.01) and t1 == "%.3f" % (int(e) * 0.01), line
        out.append((key, rec, int(s), int(e)))
    return out


def test_decode_vad_segments_end_to_end(pk, recordings, e2e):
    features = pk["features"]
    out = e2e["out"]
    windows = read_segments(os.path.join(out, "segments.alone"))
    speech = read_segments(os.path.join(out, "speech_segments.alone"))
    vec = _read_vectors(os.path.join(out, "alone"), "text")
    assert sorted(vec) == sorted(k for k, _, _, _ in windows) and np.isfinite(np.stack(list(vec.values()))).all()
    assert "=> 0 of %d segments shorter than --min-window were skipped" % len(speech) in e2e["r"].stdout
    # the kernel's segments are the loop reference applied to the GPU's own VAD vector
    fb, vo, T, v = gpu_vad(features, recordings)
    d = features.SegmentOptions()
    v = v.cpu().numpy()
    tol = vo.vad_frames_context + d.padding + 2
    for b, name in enumerate(recordings["names"]):
        mine = [(s, e) for _, rec, s, e in speech if rec == name]
        assert mine == S.segments_loop(v[b], T[b], d.padding, d.max_gap, d.min_length), name
        bursts = recordings["rec"][name][1]
        assert len(mine) == len(bursts) == 4
        for (s, e), (bs, be) in zip(mine, bursts):                          # boundaries near the planted bursts
            assert abs(s - bs) <= tol and abs(e - be) <= tol and 0 <= s < e <= T[b], (name, mine, bursts)
        win = [(s, e) for _, rec, s, e in windows if rec == name]
        assert win
        for s, e in win:                                                    # every window lies inside one speech segment
            assert any(ss <= s and e <= se for ss, se in mine), (name, s, e)
            for q0, q1 in S.silences(bursts, int(T[b])):                    # and reaches into a planted silence by the margin at most
                assert max(0, min(e, q1) - max(s, q0)) <= tol, (name, s, e, q0, q1)
        for ss, se in mine:                                                 # the windows of a segment are the window rule inside it
            got = sorted((s, e) for s, e in win if ss <= s and e <= se)
            assert got == [(ss + ws, ss + ws + wl) for ws, wl in WR.brute_windows(se - ss, 60, 30, 1)]


def test_decode_segments_file_gives_the_same_keys(e2e):
    out2, r = e2e["decode"]("fileseg", "--segments", os.path.join(e2e["out"], "speech_segments.alone"))
    first, second = (open(os.path.join(o, "segments.alone")).read() for o in (e2e["out"], out2))
    assert first == second and first
    assert open(os.path.join(out2, "speech_segments.alone")).read() == open(os.path.join(e2e["out"], "speech_segments.alone")).read()
    a, b = (_read_vectors(os.path.join(o, "alone"), "text") for o in (e2e["out"], out2))
    assert list(a) == list(b)
    for k in a:             # the same frames of the same features: the same vectors, by the bar of a row against the row run alone
        assert close(a[k][None], b[k][None]), k
    assert "segments shorter than --min-window were skipped" in r.stdout


def test_decode_vad_segments_average_and_half(e2e, recordings):
    out, r = e2e["decode"]("avg", "--vad-config", e2e["vadconf"], "--vad-segments", "--average-windows", "--min-window", "20", "--half")
    vec = _read_vectors(os.path.join(out, "alone"), "text")
    assert sorted(vec) == recordings["names"] and np.isfinite(np.stack(list(vec.values()))).all()
    assert not os.path.exists(os.path.join(out, "segments.alone")) and os.path.exists(os.path.join(out, "speech_segments.alone"))
    assert "windows left the fp16 range" in r.stdout and "=> 0 of 8 segments shorter than --min-window were skipped" in r.stdout


def test_diarize_on_the_result_spans_no_planted_silence(e2e, recordings):
    out = e2e["out"]
    dd = str(e2e["dir"] / "diar")
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "diarize.py"), "--embeddings", os.path.join(out, "alone"), "--segments",
           os.path.join(out, "segments.alone"), "--backend-score", "cosine", "--threshold", "-2.0", "--backend", "hip", "--out-dir", dd]
    r = subprocess.run(cmd, env=e2e["env"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l.split() for l in open(os.path.join(dd, "rttm"))]
    assert sorted({l[1] for l in lines}) == recordings["names"]
    for l in lines:                 # threshold -2: everything is one speaker, so only the gaps between segments can split a line
        t0, t1 = float(l[3]), float(l[3]) + float(l[4])
        bursts = recordings["rec"][l[1]][1]
        for (_, e0), (s1, _) in zip(bursts, bursts[1:]):
            assert not (t0 <= e0 * 0.01 + 0.2 and t1 >= s1 * 0.01 - 0.2), (l, e0, s1)
    assert all(sum(1 for l in lines if l[1] == k) == S.NBURST for k in recordings["names"])


def test_the_default_path_is_what_it_was(pk, recordings, e2e):
    """decode.py without the new flags writes, byte for byte, what the calls that existed before them give: Frontend without
    `segments` (voiced frames compacted), predict_windows without `segments`, the same formatting - and no speech_segments file"""
    features, ingest = pk["features"], pk["ingest"]
    out, r = e2e["decode"]("plain", "--vad-config", e2e["vadconf"])
    assert sorted(os.listdir(out)) == ["alone", "segments.alone"]
    assert "utterances shorter than --min-window were skipped" in r.stdout
    fb, vo, cmn = features.options_from_configs(os.path.join(FB, "fbank.conf"), e2e["vadconf"], 300)
    keys, table, batches, short = features.wav_scp_batches(str(e2e["dir"] / "wav.scp"), fb, 8)
    assert len(batches) == 1 and not len(short)
    b, nmax = batches[0]
    buf = torch.empty(len(b), nmax)
    table.read_padded(b, nmax, buf, 2)
    names = [keys[i] for i in b]
    feats, lengths = features.Frontend(fb, vo, cmn)(buf.cuda(), table.nsamp[b], [features.utt_id(k) for k in names], 0,
                                                    input_rate=int(table.rate[b[0]]))
    with torch.no_grad():
        emb, utt, start, length = e2e["model"].predict_windows(feats.contiguous(), lengths, window=60, period=30, min_window=1, batch_size=8)
    wkeys = ["%s-%08d-%08d" % (names[u], s, s + l) for u, s, l in zip(utt, start, length)]
    assert open(os.path.join(out, "alone"), "rb").read() == ingest.format_text_vectors(wkeys, emb.cpu().numpy(), 2)
    want = "".join("%s %s %.3f %.3f\n" % (k, names[u], s * 0.01, (s + l) * 0.01) for k, u, s, l in zip(wkeys, utt, start, length))
    assert open(os.path.join(out, "segments.alone")).read() == want
