"""Reference for the speech-segment rule (include/spkhip.h: spk_vad_segments): a frame-by-frame state machine
over the VAD decisions, written from the text of the rule and sharing no code with ingest.segments_from_vad or the kernel; a brute
force lister of the windows inside segments; the rows both test files run (every edge the rule and the kernel's 64-frame chunks
have); and the synthetic recording of the end-to-end test with the bursts it plants."""
import numpy as np

import window_ref as W


def segments_loop(v, T, p, g, m):
    """[(start, end)] of one row: frames 0 .. T - 1 of v, voiced iff != 0"""
    T = min(max(int(T), 0), len(v))
    out = []
    cur = None              # the running segment [a, b]
    run = None              # first frame of the run we are in

    def close():
        if cur is not None and cur[1] - cur[0] >= m:
            out.append((cur[0], cur[1]))

    for t in range(T + 1):
        voiced = t < T and v[t] != 0
        if voiced and run is None:
            run = t
        elif not voiced and run is not None:            # the run [run, t) has ended
            a, b = max(0, run - p), min(T, t + p)
            if cur is None:
                cur = [a, b]
            elif a - cur[1] > g:
                close()
                cur = [a, b]
            else:
                cur[1] = b
            run = None
    close()
    return out


def segments_batch(v, T, p, g, m):
    """(row, start, end) lists of a padded batch v [B, Tcap]"""
    row, start, end = [], [], []
    for b in range(len(v)):
        for s, e in segments_loop(v[b], T[b], p, g, m):
            row.append(b)
            start.append(s)
            end.append(e)
    return row, start, end


def check_consequences(segs, T, g):
    """what the rule implies for one row: disjoint and ascending, more than g frames apart, at most ceil(T / (g + 2)) segments"""
    for (s0, e0), (s1, e1) in zip(segs, segs[1:]):
        assert s0 < e0 <= s1 < e1 and s1 - e0 > g, (segs, g)
    for s, e in segs:
        assert 0 <= s < e <= T
    assert len(segs) <= -(-T // (g + 2)), (len(segs), T, g)


def segment_windows(seg_utt, seg_start, seg_end, window, period, min_window):
    """(utt, start, length, seg, skipped): the windows of every segment listed one by one with window_ref.brute_windows"""
    utt, start, length, seg, skipped = [], [], [], [], []
    for j, (u, s, e) in enumerate(zip(seg_utt, seg_start, seg_end)):
        if e - s < min_window:
            skipped.append(j)
            continue
        for ws, wl in W.brute_windows(e - s, window, period, min_window):
            utt.append(u)
            start.append(s + ws)
            length.append(wl)
            seg.append(j)
    return utt, start, length, seg, skipped


# ---- the rows of the tests ---------------------------------------------------------------------------------------------------------
DESIGN = (3, 5, 8)          # (padding, max_gap, min_length) the gap and length edges below are built for
OPTS = [DESIGN, (0, 0, 1), (10, 30, 50), (1, 1, 2), (7, 30, 50), (0, 30, 1), (7, 0, 2), (70, 1, 1)]
LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025]


def _row(T, runs, value=1):
    v = np.zeros(T, dtype=np.int32)
    for s, e in runs:
        v[s:e] = value
    return v


def edge_rows():
    """[(name, v, T)]: v may be longer than T (the frames past T are voiced there and must be ignored)"""
    p, g, m = DESIGN
    rows = []
    for T in LENGTHS:
        rows.append(("voiced%d" % T, np.ones(T, dtype=np.int32), T))
        rows.append(("silent%d" % T, np.zeros(T, dtype=np.int32), T))
        rows.append(("alt%d" % T, (np.arange(T) % 2 == 0).astype(np.int32), T))            # 1 0 1 0 ...: the maximum count
        rows.append(("alt1_%d" % T, (np.arange(T) % 2 == 1).astype(np.int32), T))          # 0 1 0 1 ...
    rows.append(("both_ends", _row(50, [(0, 5), (45, 50)]), 50))                            # padding clipped at 0 and at T
    rows.append(("both_ends_long", _row(200, [(0, 30), (170, 200)]), 200))
    first = (10, 30)
    for d, name in ((g, "gap_g_joins"), (g + 1, "gap_g1_splits")):                          # the gap after padding
        s2 = first[1] + 2 * p + d
        rows.append((name, _row(s2 + 40, [first, (s2, s2 + 20)]), s2 + 40))
    rows.append(("padded_overlap", _row(80, [(10, 20), (22, 30), (31, 40)]), 80))           # padded runs overlap: a - b < 0
    rows.append(("exactly_m", _row(60, [(30, 30 + m - 2 * p)]), 60))                        # kept
    rows.append(("m_minus_1", _row(60, [(30, 30 + m - 2 * p - 1)]), 60))                    # dropped
    rows.append(("dropped_between", _row(160, [(10, 40), (70, 71), (110, 150)]), 160))      # a dropped segment between two kept
    rows.append(("dropped_first_last", _row(160, [(10, 11), (50, 90), (130, 131)]), 160))
    vals = _row(120, [(5, 30), (60, 100)])
    vals[5:30] = [2, -1, 255, 1 << 30, -(1 << 31)] * 5                                       # nonzero values other than 1
    vals[60:100] = 7
    rows.append(("other_values", vals, 120))
    # runs and gaps across the 64-frame chunk boundaries, and across the boundary of the kernel's eight-chunk round at 512
    for edge in (64, 128, 512, 1024):
        T = edge + 70
        rows.append(("run_over_%d" % edge, _row(T, [(edge - 9, edge + 6)]), T))
        rows.append(("run_ends_at_%d" % edge, _row(T, [(edge - 20, edge)]), T))
        rows.append(("run_starts_at_%d" % edge, _row(T, [(edge, edge + 20)]), T))
        rows.append(("run_ends_at_%d_minus_1" % edge, _row(T, [(edge - 20, edge - 1), (edge + 1, edge + 15)]), T))
        rows.append(("gap_over_%d" % edge, _row(T, [(edge - 30, edge - 2), (edge + 3, edge + 30)]), T))
        rows.append(("gap_g1_over_%d" % edge, _row(T, [(edge - 30, edge - 5), (edge - 5 + 2 * p + g + 1, edge + 40)]), T))
        rows.append(("one_frame_runs_%d" % edge, _row(T, [(edge - 1, edge), (edge + 1, edge + 2), (edge + 63, edge + 64)]), T))
        rows.append(("voiced_to_T_%d" % edge, _row(edge, [(edge - 40, edge)]), edge))       # a run that reaches T, a chunk multiple
    rows.append(("three_chunks", _row(400, [(50, 50 + 3 * 64 + 5), (300, 330)]), 400))     # starts in one chunk, ends three later
    rows.append(("three_chunks_b", _row(400, [(5, 20), (63, 63 + 3 * 64 + 2)]), 400))
    long_T = 1500
    rows.append(("voiced_past_T", np.ones(long_T, dtype=np.int32), 700))                    # frames past T must be ignored
    rows.append(("voiced_past_T_64", np.ones(long_T, dtype=np.int32), 640))
    rows.append(("T_beyond_Tcap", _row(100, [(10, 100)]), 5000))                            # T is clamped to the row
    rows.append(("T_negative", np.ones(100, dtype=np.int32), -3))
    return rows


def random_rows(n, seed, tmax=400):
    """n rows of geometric runs and gaps of mixed scales"""
    rng = np.random.RandomState(seed)
    rows = []
    for i in range(n):
        T = int(rng.randint(0, tmax + 1))
        v = np.zeros(T, dtype=np.int32)
        t, on = 0, bool(rng.randint(2))
        scale = (1, 3, 12, 60)[rng.randint(4)]
        while t < T:
            n_ = int(rng.geometric(1.0 / scale))
            if on:
                v[t:t + n_] = 1
            t += n_
            on = not on
        rows.append(("random%d" % i, v, T))
    return rows


def pad_rows(rows):
    """(v [B, Tcap] int32, T [B] int64) of a list of rows; T as given (also out of range), the padding voiced where the row is short
    of Tcap only through T"""
    Tcap = max(len(v) for _, v, _ in rows)
    out = np.zeros((len(rows), Tcap), dtype=np.int32)
    for b, (_, v, _) in enumerate(rows):
        out[b, :len(v)] = v
    return out, np.array([T for _, _, T in rows], dtype=np.int64)


# ---- the synthetic recording of the end-to-end test -------------------------------------------------------------------------------
RATE = 16000
SHIFT = 160                 # samples per frame (10 ms)
BURST, SILENCE, NBURST = 1.2, 0.8, 4


def burst_recording(lead, tail, seed):
    """int16 samples: `lead` seconds of zeros, then NBURST bursts of Gaussian noise (sigma 3000) of BURST seconds separated by
    SILENCE seconds of zeros, then `tail` seconds of zeros.  -> (samples, bursts [(first frame, end frame)])"""
    rng = np.random.RandomState(seed)
    parts, bursts, n = [np.zeros(int(lead * RATE))], [], int(lead * RATE)
    for k in range(NBURST):
        if k:
            parts.append(np.zeros(int(SILENCE * RATE)))
            n += int(SILENCE * RATE)
        nb = int(BURST * RATE)
        parts.append(np.clip(rng.randn(nb) * 3000.0, -32768, 32767))
        bursts.append((n // SHIFT, (n + nb) // SHIFT))
        n += nb
    parts.append(np.zeros(int(tail * RATE)))
    return np.concatenate(parts).astype(np.int16), bursts


RECORDINGS = {"recA": (0.8, 0.8, 5), "recB": (0.4, 1.3, 6)}        # name: (lead, tail, seed): two lengths


def silences(bursts, T):
    """the planted silences of a recording of T frames: before, between and after the bursts"""
    edges = [0] + [f for b in bursts for f in b] + [T]
    return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2) if edges[i + 1] > edges[i]]
