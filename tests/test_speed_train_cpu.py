"""Training from audio with speed perturbation, the host half: the `sox ... speed F` entry of a wav.scp, the
resample span rule against brute force over every window, the perturbed frame counts and draws of WavTrainLoader,
wav_scp_batches(speed_entries=), the argument errors of compute_fbank.py and the fourth header of the C ABI.  No GPU."""
import ctypes
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import features, hip, ingest, kaldi_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_span_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOX = "sox -t wav %s -t wav - speed %s |"


def write_wav(path, x, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.asarray(x, dtype="<i2").tobytes())


# ---- the parser ----
def test_speed_entries_are_parsed():
    E = features.WavEntry
    assert features.parse_wav_entry(SOX % ("/d/a.wav", "0.9")) == E("/d/a.wav", None, [], False, "0.9")
    assert features.parse_wav_entry(SOX % ("/d/a.wav", "1.1")).speed == "1.1"
    # a factor equal to 1 is the plain file, and a plain entry still equals its four-argument construction
    assert features.parse_wav_entry(SOX % ("/d/a.wav", "1.0")) == E("/d/a.wav", None, [], False) == features.parse_wav_entry("/d/a.wav")
    assert features.parse_wav_entry(SOX % ("/d/a.wav", "1")).speed is None
    assert E("a", None, [], False).speed is None
    # paths with spaces, quoted either way
    assert features.parse_wav_entry(SOX % ('"/d/my files/a b.wav"', "0.9")) == E("/d/my files/a b.wav", None, [], False, "0.9")
    assert features.parse_wav_entry(SOX % ("'/d/my files/a.wav'", "1.1")).path == "/d/my files/a.wav"
    # an augmented entry has no speed
    e = features.parse_wav_entry('cat a.wav | wav-reverberate --shift-output=true --impulse-response="r.wav" - - |')
    assert e.augmented and e.speed is None


REFUSED_SPEED = [
    "cat a.wav | sox -t wav - -t wav - speed 0.9 |",                          # perturb_data_dir_speed.sh:81 - over a pipe
    "wav-copy a.ark:123 - | sox -t wav - -t wav - speed 0.9 |",               # :82 - over wav-copy
    "sox -t wav - -t wav - speed 0.9 |",                                      # reads its standard input
    "sox -t wav a.wav -t wav - speed fast |", "sox -t wav a.wav -t wav - speed -0.9 |", "sox -t wav a.wav -t wav - speed 0 |",
    "sox -t wav a.wav -t wav - speed 0.9 1.1 |", "sox -t wav a.wav -t wav - tempo 0.9 |", "sox -t wav a.wav -t flac - speed 0.9 |",
    "sox -t wav a.wav -t wav - speed 0.9 | cat |", "sox -t wav a.wav -t wav out.wav speed 0.9 |", "sox -t wav a b.wav -t wav - speed 0.9 |",
    # a sample of what tests/test_augment_cpu.py refuses
    "sox a.flac -t wav - |", "cat a.wav |",
    "cat a.wav | wav-reverberate --shift-output=false --impulse-response=\"r.wav\" - - |",
    "cat a.wav | wav-reverberate --shift-output=true --impulse-response=\"r.wav\" - - | sox - -t wav - |",
]


@pytest.mark.parametrize("text", REFUSED_SPEED)
def test_other_pipes_stay_refused(text):
    with pytest.raises(ValueError, match="pipe"):
        features.parse_wav_entry(text)


# ---- the resample span rule ----
RATES = [("0.9", 16000), ("1.1", 16000), ("0.999", 16000), ("1.1", 8000)]


@pytest.mark.parametrize("speed,rate", RATES)
def test_input_span_holds_every_window_and_little_more(speed, rate):
    """Every (o0, o1) of every utterance of 1 .. 3 iu + K samples.  With lo_j / hi_j the first / one past the last index of window j
    inside [0, nsamp), the union of [o0, o1) is [min lo_j, max hi_j) over the range, so
      - the planned span holds every index of every window for EVERY o1 > o0 iff planned_first(o0) <= min over j >= o0 of lo_j
        and planned_end(o1) >= max over j < o1 of hi_j: the planned first depends on o0 and the planned end on o1 alone;
      - the planned span is no longer than the union plus 2 MARGIN for every pair iff it is for the pairs where the union is
        shortest at that end, o1 = o0 + 1: planned_first(o0) >= lo_o0 - MARGIN, planned_end(o1) <= hi_(o1 - 1) + MARGIN.
    Both are checked for all outputs at once; all pairs are also enumerated one by one for the short utterances."""
    fi, fo = features.speed_rates(speed, rate)
    iu, ou, K, first, _ = features.resample_tables(fi, fo)
    M = ingest.RESAMPLE_SPAN_MARGIN
    assert M == 1
    pairs = 0
    for nsamp in range(1, 3 * iu + K + 1):
        n_out = int(features.num_resampled(nsamp, fi, fo))
        j = np.arange(n_out)
        a = R.window_starts(0, n_out, iu, ou, first)
        lo, hi = np.clip(a, 0, nsamp), np.clip(a + K, 0, nsamp)
        assert (hi > lo).all()                              # every window of an existing output has a sample inside the file
        pf, pc = ingest.resample_input_span(j, np.ones_like(j), nsamp, fi, fo)          # o1 = o0 + 1: first of o0, end of o1
        pe = pf + pc
        assert (pf >= 0).all() and (pe <= nsamp).all() and (pc >= 1).all()
        assert (pf <= np.minimum.accumulate(lo[::-1])[::-1]).all(), (nsamp, "a window starts before the planned span")
        assert (pe >= np.maximum.accumulate(hi)).all(), (nsamp, "a window ends past the planned span")
        assert (pf >= lo - M).all() and (pe <= hi + M).all(), (nsamp, "more than the margin")
        # first and end of a longer range are those of its ends
        if n_out > 1:
            f2, c2 = ingest.resample_input_span(j[:-1], n_out - j[:-1], nsamp, fi, fo)
            assert (f2 == pf[:-1]).all() and (f2 + c2 == pe[-1]).all()
        if nsamp <= 40 or nsamp in (iu + K, 2 * iu + 1, 3 * iu + K):
            for o0 in range(n_out if nsamp <= 40 else min(n_out, 25)):
                for o1 in range(o0 + 1, n_out + 1):
                    u = R.window_union(o0, o1, nsamp, iu, ou, K, first)
                    f, c = ingest.resample_input_span(o0, o1 - o0, nsamp, fi, fo)
                    assert f <= u[0] and f + c >= u[1] and c <= u[1] - u[0] + 2 * M, (nsamp, o0, o1)
                    pairs += 1
    assert pairs > 1000


def test_the_table_is_not_assumed_monotone():
    """a(j) may step back by one across outputs (the fp64 table); what the rule relies on is that it never steps back by more"""
    for speed, rate in RATES + [("0.9", 8000), ("1.001", 16000), ("0.95", 16000)]:
        fi, fo = features.speed_rates(speed, rate)
        iu, ou, K, first, _ = features.resample_tables(fi, fo)
        a = R.window_starts(0, 3 * ou, iu, ou, first)
        assert (a[None, :] - a[:, None])[np.triu_indices(a.size, 1)].min() >= -ingest.RESAMPLE_SPAN_MARGIN


def test_check_resample_spans_refuses_a_span_short_by_one_sample():
    fi, fo = features.speed_rates("0.9", 16000)
    N = 20000
    n_out = int(features.num_resampled(N, fi, fo))
    o, m = np.array([3000, 0, n_out - 700]), np.array([5000, 900, 700])
    f, c = ingest.resample_input_span(o, m, N, fi, fo)
    assert f[1] == 0 and f[2] + c[2] == N and f[0] > 0
    tot = np.full(3, N)
    args = lambda f, c, **kw: features.check_resample_spans("t", fi, fo, c, f, tot, o, m, 6000, 5000, **kw)     # noqa: E731
    args(f, c)
    for row, (df, dc) in [(0, (1, -1)), (0, (0, -1)), (2, (1, -1)), (1, (0, -1))]:
        f2, c2 = f.copy(), c.copy()
        f2[row] += df
        c2[row] += dc
        with pytest.raises(ValueError, match=r"row %d .*outside the row" % row):
            args(f2, c2)
        args(f2, c2, rows=[r for r in range(3) if r != row])           # rows that are not in the list are not looked at
    with pytest.raises(ValueError, match="row 2 .*outputs outside"):
        features.check_resample_spans("t", fi, fo, c, f, tot, o, m + np.array([0, 0, 1]), 6000, 5000)
    with pytest.raises(ValueError, match="row 1 .*not a part"):
        features.check_resample_spans("t", fi, fo, c + np.array([0, N, 0]), f, tot, o, m, 30000, 5000)
    with pytest.raises(ValueError, match="2\\^30"):
        features.check_resample_spans("t", fi, fo, c, f, np.full(3, 2 ** 30), o, m, 6000, 5000)
    with pytest.raises(ValueError, match="2\\^30"):          # the perturbed length, with the file's below the limit
        features.check_resample_spans("t", fi, fo, c, f, np.full(3, 2 ** 30 - 8), o, m, 6000, 5000)


# ---- the loader ----
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """8 files, each as a plain line, an sp0.9- line and an sp1.1- line, with the VAD vectors of the perturbed lengths and a fake
    archive whose entries have as many rows as their line has voiced frames"""
    d = tmp_path_factory.mktemp("speed")
    rs = np.random.RandomState(7)
    opts = features.FbankOptions(num_mel_bins=4, snip_edges=False, dither=0.0)
    wav, vad, feats, u2s, frames = [], [], [], [], {}
    with open(str(d / "vad.ark"), "wb") as fv, open(str(d / "feats.ark"), "wb") as fa:
        for u in range(8):
            n = int(rs.randint(9000, 20000))
            p = d / ("u%d.wav" % u)
            write_wav(p, rs.randint(-3000, 3000, size=n))
            for sp in (None, "0.9", "1.1"):
                key = "s%d-u%d" % (u % 3, u) if sp is None else "sp%s-s%d-u%d" % (sp, u % 3, u)
                n2 = n if sp is None else int(features.num_resampled(n, *features.speed_rates(sp, 16000)))
                T = frames[key] = opts.num_frames(n2)
                v = (rs.rand(T) < 0.7).astype(np.float32)
                v[:40] = 1
                fv.write((key + " ").encode())
                off = fv.tell()
                kaldi_io.write_vec_flt(fv, v)
                vad.append("%s %s:%d" % (key, d / "vad.ark", off))
                foff = kaldi_io.write_mat(fa, np.zeros((int(v.sum()), 4), dtype=np.float32), key=key)
                feats.append("%s %s:%d" % (key, d / "feats.ark", foff))
                wav.append("%s %s" % (key, p if sp is None else SOX % (p, sp)))
                u2s.append("%s %d" % (key, (u % 3) + (0 if sp is None else 3 if sp == "0.9" else 6)))      # new sp<F>- speakers
    for name, lines in (("wav.scp", wav), ("vad.scp", vad), ("feats.scp", feats), ("utt2spkid", u2s)):
        open(str(d / name), "w").write("\n".join(lines) + "\n")
    return d, opts, frames


def _loader(d, opts, **kw):
    kw.setdefault("vad_scp", str(d / "vad.scp"))
    return ingest.WavTrainLoader(str(d / "wav.scp"), str(d / "utt2spkid"), 40, 8, opts, features.CmnOptions(cmn_window=30), **kw)


def test_frames_are_counted_on_the_perturbed_clock(corpus):
    d, opts, frames = corpus
    b = _loader(d, opts)
    assert b.has_speed and b.rates == [(14400, 16000), (17600, 16000)]
    for i, k in enumerate(b.keys):
        sp = b.speed[i]
        assert sp == (k[2:5] if k.startswith("sp") else None)
        n2 = int(b.table.nsamp[i]) if sp is None else int(features.num_resampled(int(b.table.nsamp[i]), *features.speed_rates(sp, 16000)))
        assert b.nsamp_out[i] == n2 and b.frames[i] == opts.num_frames(n2) == frames[k]
        assert b.utt_ids[i] == features.utt_id(k)            # the dither stream of the copy is keyed by the copy's own key
    assert (b.frames[1::3] > b.frames[0::3]).all() and (b.frames[2::3] < b.frames[0::3]).all()
    # the span of the file a chunk needs: planned on the perturbed clock, mapped through the resample span rule
    rows = np.arange(6)
    p = b.plan(rows, [0, 1, 2, 3, 4, 5], 40)
    f, c = b.input_spans(rows, p)
    assert (f[0::3] == p.first[0::3]).all() and (c[0::3] == p.count[0::3]).all()
    for r in (1, 2, 4, 5):
        fi, fo = features.speed_rates(b.speed[r], 16000)
        assert (f[r], c[r]) == tuple(int(v) for v in ingest.resample_input_span(p.first[r], p.count[r], b.table.nsamp[r], fi, fo))
        assert 0 <= f[r] and f[r] + c[r] <= b.table.nsamp[r] and abs(c[r] * fo / fi - p.count[r]) < 40


def test_a_vad_vector_of_the_unperturbed_length_is_refused(corpus, tmp_path):
    d, opts, _ = corpus
    vl = open(str(d / "vad.scp")).read().splitlines()
    assert vl[4].startswith("sp0.9-s1-u1 ") and vl[3].startswith("s1-u1 ")
    vl[4] = "sp0.9-s1-u1 " + vl[3].split()[1]         # the recipe's mistake: the clean file's vector under the copy's key
    open(str(tmp_path / "v.scp"), "w").write("\n".join(vl) + "\n")
    with pytest.raises(ValueError, match=r"sp0\.9-s1-u1.*frames but its vector"):
        _loader(d, opts, vad_scp=str(tmp_path / "v.scp"))


@pytest.mark.parametrize("chunk_range", [None, (24, 40, 8)])
def test_draws_equal_native_train_loader(corpus, chunk_range):
    d, opts, _ = corpus
    n = 0
    for world, rank in ((1, 0), (2, 1)):
        kw = dict(rank=rank, world=world, seed=3, chunk_range=chunk_range)
        a = ingest.NativeTrainLoader(str(d / "feats.scp"), str(d / "utt2spkid"), 40, 8, **kw)
        b = _loader(d, opts, **kw)
        assert len(a) == len(b)
        np.testing.assert_array_equal(a.labels, b.labels)
        for epoch in (0, 1):
            a.set_epoch(epoch)
            b.set_epoch(epoch)
            da, db = list(a.draws()), list(b.draws())
            assert len(da) == len(db) == len(a)
            for (ka, sa, ra, Ta, sta), (kb, sb, rb, Tb, stb) in zip(da, db):
                np.testing.assert_array_equal(sa, sb)
                assert (ka, Ta, sta) == (kb, Tb, stb)
                assert [a.table.rows[i] for i in ra] == [b.rows[i] for i in rb]
                n += len(sta)
    assert n > 0


def test_loader_refuses_a_factor_beyond_the_lds_budget(corpus, tmp_path):
    d, opts, _ = corpus
    lines = open(str(d / "wav.scp")).read().splitlines()
    path = lines[0].split()[1]
    fi, fo = features.speed_rates("0.99975", 16000)
    iu, ou, K = features._resample_first(fi, fo)[:3]
    assert hip.lib().spk_resample_tile(iu, ou, K) == 0
    open(str(tmp_path / "w.scp"), "w").write("\n".join(lines[:-1] + ["sp1.1-s1-u7 " + SOX % (path, "0.99975")]) + "\n")
    with pytest.raises(ValueError, match=r"sp1\.1-s1-u7.*15996 -> 16000"):
        ingest.WavTrainLoader(str(tmp_path / "w.scp"), str(d / "utt2spkid"), 40, 8, opts, vad_scp=str(d / "vad.scp"))
    with pytest.raises(ValueError, match=r"sp1\.1-s1-u7.*15996 -> 16000"):
        features.wav_scp_batches(str(tmp_path / "w.scp"), opts, 4, speed_entries=True)


# ---- wav_scp_batches ----
def test_wav_scp_batches_with_speed_entries(corpus, tmp_path):
    d, opts, _ = corpus
    scp = str(d / "wav.scp")
    with pytest.raises(ValueError, match="pipe"):
        features.wav_scp_batches(scp, opts, 4)
    with pytest.raises(ValueError, match="pipe"):
        features.wav_scp_batches(scp, opts, 4, augment=True)
    with pytest.raises(ValueError, match="does not combine"):
        features.wav_scp_batches(scp, opts, 4, speed="0.9", speed_entries=True)
    keys, table, batches, short = features.wav_scp_batches(scp, opts, 4, speed_entries=True)
    assert table.speed == [None, "0.9", "1.1"] * 8 and short.size == 0
    assert sorted(int(i) for idx, _ in batches for i in idx) == list(range(24))
    for idx, nmax in batches:
        assert len({table.speed[i] for i in idx}) == 1 and nmax >= table.nsamp[idx].max()
    # `short` is judged after perturbation: 399 samples played at 0.9 are 444 >= 400, at 1.1 they are 363
    write_wav(tmp_path / "s.wav", np.zeros(399, dtype=np.int16))
    open(str(tmp_path / "s.scp"), "w").write("".join("%s %s\n" % (k, v) for k, v in [
        ("a", tmp_path / "s.wav"), ("sp0.9-a", SOX % (tmp_path / "s.wav", "0.9")), ("sp1.1-a", SOX % (tmp_path / "s.wav", "1.1"))]))
    _, _, b2, short2 = features.wav_scp_batches(str(tmp_path / "s.scp"), opts, 4, speed_entries=True)
    assert list(short2) == [0, 2] and [list(i) for i, _ in b2] == [[1]]
    # a plain wav.scp gives the batches of before, with or without the argument
    plain = str(tmp_path / "plain.scp")
    open(plain, "w").write("\n".join(open(scp).read().splitlines()[0::3]) + "\n")
    ref = features.wav_scp_batches(plain, opts, 3)
    got = features.wav_scp_batches(plain, opts, 3, speed_entries=True)
    assert ref[0] == got[0] and len(ref[2]) == len(got[2]) >= 3
    for (ia, na), (ib, nb) in zip(ref[2], got[2]):
        assert list(ia) == list(ib) and na == nb
    assert got[1].speed == [None] * 8


# ---- compute_fbank.py: argument errors need no GPU ----
def _run(args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py")] + args, env=env, capture_output=True,
                          text=True, timeout=300)


def test_compute_fbank_argument_errors(corpus, tmp_path):
    d, _, _ = corpus
    out = str(tmp_path / "out")
    r = _run([str(d / "wav.scp"), out, "--speed", "0.9"])
    assert r.returncode == 2 and "--speed does not combine with the `sox ... speed` entries" in r.stderr, r.stderr[-2000:]
    piped = str(tmp_path / "p.scp")
    open(piped, "w").write("u0 cat a.wav | sox -t wav - -t wav - speed 0.9 |\n")
    r = _run([piped, out])
    assert r.returncode == 2 and "pipe" in r.stderr
    aug = str(tmp_path / "a.scp")
    open(aug, "w").write('u0 cat a.wav | wav-reverberate --shift-output=true --impulse-response="r.wav" - - |\n')
    r = _run([aug, out, "--speed", "0.9"])
    assert r.returncode == 2 and "--speed does not combine with wav-reverberate entries" in r.stderr
    assert not os.path.exists(out)


# ---- the C ABI ----
NEW = ["spkw_resample_span_fwd", "spkw_copy_rows_fwd"]


def test_the_fourth_header_is_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spkwav.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(spkw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert sorted(decl) == sorted(NEW) == sorted(hip.wav_symbols()) == sorted(hip._WAV_SIGS)
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    others = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("spkhip.h", "spkder.h", "spkcal.h"))
    for name in NEW:
        assert hasattr(hip.lib(), name) and re.search(r" T %s$" % name, nm, re.M), name
        assert len([p for p in decl[name].split(",") if p.strip() != "void"]) == len(hip._WAV_SIGS[name]), name
        assert getattr(hip.lib(), name).restype is ctypes.c_int
        assert not re.fullmatch(r"spk_[a-z0-9_]+", name) and not re.search(r"\b%s\b" % name, others), name
        assert name not in hip.exported_symbols() + hip.der_symbols() + hip.cal_symbols()
    # the three old tables and what the library exports under spk_* are as they were
    assert (len(hip.exported_symbols()), len(hip.der_symbols()), len(hip.cal_symbols())) == (128, 7, 9)
    exported = set(re.findall(r" T (spk_[a-z0-9_]+)$", nm, re.M))
    assert exported == set(hip.exported_symbols()) | set(hip.der_symbols()) | set(hip.cal_symbols())
    assert set(re.findall(r" T (spkw_[a-z0-9_]+)$", nm, re.M)) == set(NEW)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "include/spkwav.h" in readme and "(128 exports)" in readme


def test_span_calls_are_refused_on_the_host_before_any_launch():
    """no device is needed: a refused call launches nothing and touches no pointer"""
    lib = hip.lib()
    one = ctypes.c_void_p(8)            # never followed
    ok = [one] * 7 + [2, 2, 100, one, one, 14400, 16000, 15, one, 100, None]
    assert lib.spkw_resample_span_fwd(*([None] + ok[1:])) < 0 and b"spkw_resample_span_fwd: null" in lib.spk_last_error()
    for pos, val, msg in [(12, 16000, b"rates"), (9, 2 ** 30, b"Nmax_in"), (16, 2 ** 30, b"Nmax_out"), (7, 3, b"R=3"), (7, 0, b"R=0"),
                          (12, 15998, b"LDS"), (14, 0, b"K=0")]:
        a = list(ok)
        a[pos] = val
        assert lib.spkw_resample_span_fwd(*a) < 0 and msg in lib.spk_last_error(), (pos, lib.spk_last_error())
    a = list(ok)
    a[6], a[7] = None, 1                # without a row list R must be B
    assert lib.spkw_resample_span_fwd(*a) < 0 and b"R=1" in lib.spk_last_error()
    assert lib.spkw_copy_rows_fwd(None, one, None, 2, 2, 8, one, 8, None) < 0 and b"spkw_copy_rows_fwd: null" in lib.spk_last_error()
    assert lib.spkw_copy_rows_fwd(one, one, one, 3, 2, 8, one, 8, None) < 0 and b"R=3" in lib.spk_last_error()
    # the wrapper: lengths at or above 2^30 and a table beyond the LDS budget, before the tensor is looked at further
    with pytest.raises(ValueError, match="float32 cuda"):
        features.resample_span(np.zeros((1, 8), dtype=np.float32), [8], [0], [8], [0], [4], 14400, 16000)
