"""Native batch ingest (libspkio): scp/ark -> pinned [B, F, T] staging, cropped at read time.

Same sampling semantics as the reference's SequenceDataset + DataLoader(shuffle / DistributedSampler)
(scripts/datasets.py:10-72, scripts/train_resnet.py:237-247): class-balanced repetition of scp lines, a fresh
permutation per epoch (seeded with the epoch like DistributedSampler.set_epoch), equal shards per rank (padded by
wrap-around), a uniform random crop start per sample.  What changes is the mechanics: one C++ call reads a whole
batch with pread() on a small thread pool, reading only the cropped frames, and transposes them straight into pinned
memory; a background thread keeps the next batch ready while the GPU works on the current one.

WavTrainLoader is the same loader over 16-bit PCM WAV files (train_resnet.py --wav-scp): the same draws from
one seeded index function, the span of each file that a chunk needs read as int16 (spk_wav_read_span), the chunk computed on the GPU.
"""
import collections
import ctypes
import os
import queue
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libspkio.so")
        if not os.path.exists(path):
            raise RuntimeError("libspkio.so is missing at %s: run `python __graft_entry__.py build`" % path)
        l = ctypes.CDLL(path)
        l.spk_io_last_error.restype = ctypes.c_char_p
        cpp, i64p, i32p = ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        l.spk_ark_probe.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i64p]
        l.spk_ark_read_crop.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int]
        l.spk_ark_read_padded.argtypes = [ctypes.c_int, cpp, i64p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        l.spk_ark_probe_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i64p, i32p]
        l.spk_ark_read_crop_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_int]
        l.spk_ark_read_padded_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_int]
        l.spk_ark_read_crop_codes.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
        l.spk_ark_read_padded_codes.argtypes = [ctypes.c_int, cpp, i64p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int]
        l.spk_wav_probe.argtypes = [ctypes.c_int, cpp, ctypes.c_int, i32p, i64p, i64p]
        l.spk_wav_read_padded.argtypes = [ctypes.c_int, cpp, i64p, i64p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]
        l.spk_wav_read_span.argtypes = [ctypes.c_int, cpp, i64p, i64p, i64p, i64p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]
        l.spk_text_vectors_bound.argtypes = [ctypes.c_int, ctypes.c_int, cpp]
        l.spk_text_vectors_bound.restype = ctypes.c_int64
        l.spk_format_text_vectors.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, cpp, ctypes.c_char_p, ctypes.c_int64,
                                              ctypes.c_int]
        l.spk_format_text_vectors.restype = ctypes.c_int64
        _LIB = l
    return _LIB


def format_text_vectors(keys, vecs, nthreads=4):
    """bytes of the text ark 'key [ v0 v1 ... ]\\n' per row of float32 vecs [n][D], every value printed exactly like
    numpy's str(np.float32) (the reference's scripts/decode.py:206 line format), formatted natively on `nthreads` threads."""
    vecs = np.ascontiguousarray(vecs, dtype=np.float32)
    n, D = vecs.shape
    assert len(keys) == n
    arr = (ctypes.c_char_p * n)(*[k.encode() for k in keys])
    cap = lib().spk_text_vectors_bound(n, D, arr)
    buf = ctypes.create_string_buffer(cap)
    w = lib().spk_format_text_vectors(n, D, vecs.ctypes.data, arr, buf, cap, int(nthreads))
    if w < 0:
        raise RuntimeError("spk_format_text_vectors: buffer too small")
    return buf.raw[:w]


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, lib().spk_io_last_error().decode()))


def _split_rx(rx):
    path, off = rx.rsplit(":", 1)
    return path, int(off)


KIND_FM, KIND_CM = 0, 1        # ArkTable.kind: float32 'FM ' / one-byte compressed 'CM ' 


def _i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


class ArkTable:
    """Parsed scp: per line the ark path, the payload offset, the frame count and the kind of the record - float32 'FM ' or
    Kaldi's one-byte compressed 'CM ', mixed freely (headers probed once)."""

    def __init__(self, rxfiles):
        paths, offs = zip(*[_split_rx(r) for r in rxfiles])
        uniq = sorted(set(paths))
        self._cpaths = {p: ctypes.c_char_p(p.encode()) for p in uniq}
        self.paths = list(paths)
        n = len(paths)
        self.rows = np.zeros(n, dtype=np.int32)
        self.cols = np.zeros(n, dtype=np.int32)
        self.data_off = np.zeros(n, dtype=np.int64)
        self.kind = np.zeros(n, dtype=np.int32)
        arr = (ctypes.c_char_p * n)(*[self._cpaths[p].value for p in paths])
        offs = np.asarray(offs, dtype=np.int64)
        _check(lib().spk_ark_probe_kinds(n, arr, _i64p(offs), _i32p(self.rows), _i32p(self.cols), _i64p(self.data_off),
                                         _i32p(self.kind)), "spk_ark_probe_kinds")
        self.all_cm = bool(n > 0 and (self.kind == KIND_CM).all())

    def _batch(self, idx):
        B = len(idx)
        F = int(self.cols[idx[0]])
        assert (self.cols[idx] == F).all()
        arr = (ctypes.c_char_p * B)(*[self._cpaths[self.paths[i]].value for i in idx])
        return (B, F, arr, np.ascontiguousarray(self.data_off[idx]), np.ascontiguousarray(self.rows[idx]),
                np.ascontiguousarray(self.kind[idx]))

    def read_crop(self, idx, starts, T, out, nthreads=4):
        """out: contiguous float32 host tensor [B, F, T] (ideally pinned).  'CM ' entries are decoded on the host, to the bits of
        kaldi_io.read_mat."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, F, T) and out.dtype == torch.float32
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        _check(lib().spk_ark_read_crop_kinds(B, arr, _i64p(doff), _i32p(rows), _i32p(st), _i32p(kind), F, T, out.data_ptr(), nthreads),
               "spk_ark_read_crop")
        return out

    def read_padded(self, idx, T, out, nthreads=4):
        """Whole utterances idx (each of 1..T frames) into a contiguous float32 host tensor out [B, F, T] (ideally pinned), the
        frames past each utterance's length zero-filled; self.rows[idx] are the lengths to pass to predict(x, lengths=...)."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, F, T) and out.dtype == torch.float32
        _check(lib().spk_ark_read_padded_kinds(B, arr, _i64p(doff), _i32p(rows), _i32p(kind), F, T, out.data_ptr(), nthreads),
               "spk_ark_read_padded")
        return out

    def read_crop_codes(self, idx, starts, T, codes, colhdr, nthreads=4):
        """'CM ' entries as stored, for features.decompress (the GPU decode): codes, a contiguous uint8 host tensor [B, F, T]
        (codes[b, f, t]: frame starts[b] + t, bin f), and colhdr, contiguous float32 [B, F, 4], the decoded column headers.  A
        quarter of read_crop's bytes and no transpose; an 'FM ' entry is an error."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert codes.is_contiguous() and tuple(codes.shape) == (B, F, T) and codes.dtype == torch.uint8
        assert colhdr.is_contiguous() and tuple(colhdr.shape) == (B, F, 4) and colhdr.dtype == torch.float32
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        _check(lib().spk_ark_read_crop_codes(B, arr, _i64p(doff), _i32p(rows), _i32p(st), F, T, codes.data_ptr(), colhdr.data_ptr(),
                                             nthreads), "spk_ark_read_crop_codes")
        return codes, colhdr

    def read_padded_codes(self, idx, T, codes, colhdr, nthreads=4):
        """read_crop_codes for whole utterances idx (each of 1..T frames): codes zero past each utterance's length"""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert codes.is_contiguous() and tuple(codes.shape) == (B, F, T) and codes.dtype == torch.uint8
        assert colhdr.is_contiguous() and tuple(colhdr.shape) == (B, F, 4) and colhdr.dtype == torch.float32
        _check(lib().spk_ark_read_padded_codes(B, arr, _i64p(doff), _i32p(rows), F, T, codes.data_ptr(), colhdr.data_ptr(), nthreads),
               "spk_ark_read_padded_codes")
        return codes, colhdr


class WavTable:
    """Parsed wav.scp entries (file paths; Kaldi pipe entries 'cmd |' are refused): per file the sample count and the offset of the
    samples, probed once.  PCM 16-bit mono only, at `sample_rate` (0: any) - everything else is refused naming the file."""

    def __init__(self, paths, sample_rate=0):
        for p in paths:
            if p.rstrip().endswith("|"):
                raise ValueError("wav.scp pipe entries are not supported: %r" % p)
        self.paths = list(paths)
        n = len(self.paths)
        self._cpaths = [ctypes.c_char_p(p.encode()) for p in self.paths]
        self.rate = np.zeros(n, dtype=np.int32)
        self.nsamp = np.zeros(n, dtype=np.int64)
        self.data_off = np.zeros(n, dtype=np.int64)
        arr = (ctypes.c_char_p * max(n, 1))(*[c.value for c in self._cpaths])
        _check(lib().spk_wav_probe(n, arr, int(sample_rate), self.rate.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   self.nsamp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                   self.data_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "spk_wav_probe")

    def read_padded(self, idx, Nmax, out, nthreads=4):
        """Files idx into a contiguous float32 host tensor out [B, Nmax] (ideally pinned) at int16 scale, zero past each file's
        sample count self.nsamp[idx] (each <= Nmax)."""
        B = len(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, Nmax) and out.dtype == torch.float32
        arr = (ctypes.c_char_p * B)(*[self._cpaths[i].value for i in idx])
        doff = np.ascontiguousarray(self.data_off[idx])
        ns = np.ascontiguousarray(self.nsamp[idx])
        _check(lib().spk_wav_read_padded(B, arr, doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(Nmax), out.data_ptr(), nthreads),
               "spk_wav_read_padded")
        return out

    def read_span(self, idx, first, count, Nmax, out, nthreads=4):
        """Per row b, count[b] samples from sample first[b] of file idx[b], as they lie in the file, into a contiguous int16 host
        tensor out [B, Nmax] (ideally pinned), zero past the count: only the span is read.  A span outside its file, or longer than
        Nmax, is refused naming the file."""
        B = len(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, Nmax) and out.dtype == torch.int16
        arr = (ctypes.c_char_p * B)(*[self._cpaths[i].value for i in idx])
        doff = np.ascontiguousarray(self.data_off[idx])
        ns = np.ascontiguousarray(self.nsamp[idx])
        fi = np.ascontiguousarray(np.asarray(first, dtype=np.int64))
        ct = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
        assert fi.shape == (B,) and ct.shape == (B,)
        _check(lib().spk_wav_read_span(B, arr, _i64p(doff), _i64p(ns), _i64p(fi), _i64p(ct), int(Nmax), out.data_ptr(), nthreads),
               "spk_wav_read_span")
        return out


def pad_batches(lengths, batch_size, max_pad_ratio=0.1, quantum=8):
    """Length-sorted padded batches for whole-utterance extraction: a list of (indices, T_pad).  Utterances are taken in order of
    length (stable) and a batch grows until it holds batch_size of them or one more would make its padded frames
    len * T_pad exceed (1 + max_pad_ratio) x its real frames; T_pad = the batch's longest utterance rounded up to `quantum`.
    Every index lands in exactly one batch; a batch of one may exceed the ratio by its rounding."""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if batch_size < 1 or quantum < 1 or max_pad_ratio < 0:
        raise ValueError("pad_batches: batch_size >= 1, quantum >= 1, max_pad_ratio >= 0")
    if L.size and L.min() < 1:
        raise ValueError("pad_batches: every length must be >= 1")
    order = np.argsort(L, kind="stable")
    batches, i, n = [], 0, len(order)
    while i < n:
        j, real = i + 1, int(L[order[i]])
        while j < n and j - i < batch_size:
            t_pad = -(-int(L[order[j]]) // quantum) * quantum
            if (j - i + 1) * t_pad > (1.0 + max_pad_ratio) * (real + int(L[order[j]])):
                break
            real += int(L[order[j]])
            j += 1
        idx = order[i:j]
        batches.append((idx, -(-int(L[idx[-1]]) // quantum) * quantum))
        i = j
    return batches


# ---- windowed extraction ----
WindowPlan = collections.namedtuple("WindowPlan", "utt start length skipped")
WindowPlan.__doc__ = """plan_windows' result: flat int64 arrays, one entry per window in utterance order and then window order - the
utterance, the first frame and the frame count of the window - and `skipped`, the utterances shorter than min_window (ascending)"""


def plan_windows(lengths, window, period, min_window):
    """The window rule (numpy only).  An utterance of n frames with n < min_window yields no window and is listed in `skipped`;
    otherwise window k = 0, 1, ... covers the frames [k period, min(k period + window, n)), the last one being the first k with
    k period + window >= n (later ones would be subsets of it), emitted only when it has at least min_window frames or is k = 0.
    period == window is Kaldi's chunking (nnet3-xvector-compute --chunk-size window --min-chunk-size min_window)."""
    W, P, M = int(window), int(period), int(min_window)
    if W < 1 or P < 1 or not 1 <= M <= W:
        raise ValueError("plan_windows: window >= 1, period >= 1 and 1 <= min_window <= window, got window=%d period=%d min_window=%d"
                         % (W, P, M))
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("plan_windows: a length is negative")
    keep = n >= M
    klast = np.where(keep, np.maximum(0, -(-(n - W) // P)), 0)          # the first k with k P + W >= n
    emit_last = (klast == 0) | (n - klast * P >= M)
    count = np.where(keep, klast + emit_last, 0)
    utt = np.repeat(np.arange(n.size, dtype=np.int64), count)
    first = np.cumsum(count) - count
    k = np.arange(int(count.sum()), dtype=np.int64) - np.repeat(first, count)
    start = k * P
    length = np.minimum(start + W, n[utt]) - start
    return WindowPlan(utt, start, length, np.nonzero(~keep)[0].astype(np.int64))


def window_batches(length, batch_size, max_pad_ratio=0.1, quantum=8):
    """The rows of a window plan grouped into padded batches: pad_batches over the window lengths - a list of (plan rows, Wcap) with
    at most batch_size rows each, Wcap the batch's longest window rounded up to `quantum`, at most max_pad_ratio padded frames.
    Every plan row lands in exactly one batch; concatenating the batches' rows gives the permutation that restores plan order."""
    return pad_batches(length, batch_size, max_pad_ratio, quantum)


# ---- speech segments: VAD decisions -> segments, and the windows inside them ----
def segments_from_vad(v, T, opts):
    """The segment rule of include/spkhip.h: spk_vad_segments on the host (numpy only; the `host` back end of
    scripts/vad_to_segments.py and the reference of features.vad_segments).  v [Tcap] or [B, Tcap]: frame t of row b is voiced iff
    v[b, t] != 0 and t < T[b] (T clamped to [0, Tcap]; a scalar for one row).  opts: padding >= 0, max_gap >= 0, min_length >= 1
    in frames (features.SegmentOptions).  -> (row, start, end), flat int64 arrays, one entry per segment in row and then time order."""
    p, g, m = int(opts.padding), int(opts.max_gap), int(opts.min_length)
    if p < 0 or g < 0 or m < 1:
        raise ValueError("segments_from_vad: padding >= 0, max_gap >= 0 and min_length >= 1, got %d %d %d" % (p, g, m))
    v = np.asarray(v)
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim != 2:
        raise ValueError("segments_from_vad: v must be [Tcap] or [B, Tcap], got shape %s" % (v.shape,))
    B, Tcap = v.shape
    Tv = np.clip(np.asarray(T, dtype=np.int64).reshape(-1), 0, Tcap)
    if Tv.shape != (B,):
        raise ValueError("segments_from_vad: T has %d entries for %d rows" % (Tv.size, B))
    voiced = np.zeros((B, Tcap + 2), dtype=np.int8)           # a silent frame on either side: every run has both edges
    voiced[:, 1:-1] = (v != 0) & (np.arange(Tcap)[None, :] < Tv[:, None])
    d = np.diff(voiced, axis=1)                                # [B, Tcap + 1]: +1 at a run's first frame, -1 at its exclusive end
    row, s = np.nonzero(d == 1)                                # row-major: by row, then ascending
    e = np.nonzero(d == -1)[1]
    a = np.maximum(s - p, 0)
    b = np.minimum(e + p, Tv[row])
    opens = np.ones(row.size, dtype=bool)
    opens[1:] = (row[1:] != row[:-1]) | (a[1:] - b[:-1] > g)
    first = np.nonzero(opens)[0]
    last = np.append(first[1:], row.size)[:first.size] - 1     # the last run of each segment (none without a run)
    seg_row, seg_a, seg_b = row[first], a[first], b[last]
    keep = seg_b - seg_a >= m
    return seg_row[keep].astype(np.int64), seg_a[keep].astype(np.int64), seg_b[keep].astype(np.int64)


SegmentWindowPlan = collections.namedtuple("SegmentWindowPlan", "utt start length seg skipped")
SegmentWindowPlan.__doc__ = """plan_segment_windows' result: flat int64 arrays, one entry per window in segment order and then window
order - the utterance, the first frame IN THE UTTERANCE, the frame count and the segment of the window - and `skipped`, the segments
shorter than min_window (ascending)"""


def plan_segment_windows(seg_utt, seg_start, seg_end, window, period, min_window):
    """The window rule inside speech segments (numpy only): segment j = frames [seg_start[j], seg_end[j]) of utterance seg_utt[j]
    gets exactly the windows of plan_windows([seg_end[j] - seg_start[j]], window, period, min_window), shifted by seg_start[j].
    The segments come sorted by utterance, and ascending and disjoint within one (touching is allowed)."""
    u = np.asarray(seg_utt, dtype=np.int64).reshape(-1)
    s = np.asarray(seg_start, dtype=np.int64).reshape(-1)
    e = np.asarray(seg_end, dtype=np.int64).reshape(-1)
    if not u.size == s.size == e.size:
        raise ValueError("plan_segment_windows: seg_utt, seg_start and seg_end have %d, %d and %d entries" % (u.size, s.size, e.size))

    def refuse(mask, msg):
        if mask.any():
            j = int(np.nonzero(mask)[0][0])
            raise ValueError("plan_segment_windows: segment %d (utterance %d, frames [%d, %d)) %s" % (j, u[j], s[j], e[j], msg))

    refuse(s < 0, "starts before frame 0")
    refuse(e <= s, "is empty")
    if u.size:
        refuse(np.append(False, u[1:] < u[:-1]), "comes after a segment of a later utterance: seg_utt must not decrease")
        refuse(np.append(False, (u[1:] == u[:-1]) & (s[1:] < e[:-1])), "starts before the end of the segment before it")
    plan = plan_windows(e - s, window, period, min_window)
    return SegmentWindowPlan(u[plan.utt], plan.start + s[plan.utt], plan.length, plan.utt, plan.skipped)


def time_to_frame(t, frame_shift):
    """frame of a time: floor(t / frame_shift + 0.5), evaluated on the decimal values as written (t: the text of a segments file,
    or a number taken by its shortest representation), so that a time on a half-frame boundary always rounds up"""
    import fractions
    import math
    return math.floor(fractions.Fraction(str(t)) / fractions.Fraction(str(frame_shift)) + fractions.Fraction(1, 2))


def read_segments_file(path, recordings, frame_shift):
    """A Kaldi segments file, '<segment-id> <recording> <start s> <end s>' per line, for scripts/decode.py --segments ->
    {recording: (start frames, end frames)}, int64 arrays ascending in time (time_to_frame; ends not yet clipped to the recording).
    ValueError naming the lines: a malformed line, a recording that is not in `recordings`, a segment that is empty after rounding,
    segments of one recording that overlap."""
    known = set(recordings)
    per = {}
    for n, line in enumerate(open(path), 1):
        tok = line.split()
        if not tok:
            continue
        where = "%s:%d" % (path, n)
        if len(tok) != 4:
            raise ValueError("%s: expected '<segment-id> <recording> <start> <end>', got %r" % (where, line.rstrip("\n")))
        try:
            s, e = time_to_frame(tok[2], frame_shift), time_to_frame(tok[3], frame_shift)
        except (ValueError, ZeroDivisionError):
            raise ValueError("%s: times %r %r are not numbers" % (where, tok[2], tok[3]))
        if tok[1] not in known:
            raise ValueError("%s: recording %r is not in the wav.scp" % (where, tok[1]))
        if s < 0 or e <= s:
            raise ValueError("%s: segment %s is empty after rounding to frames [%d, %d)" % (where, tok[0], s, e))
        per.setdefault(tok[1], []).append((s, e, n))
    out = {}
    for rec, segs in per.items():
        segs.sort()
        for (s0, e0, n0), (s1, e1, n1) in zip(segs, segs[1:]):
            if s1 < e0:
                raise ValueError("%s:%d and %s:%d: segments of recording %r overlap (frames [%d, %d) and [%d, %d))"
                                 % (path, n0, path, n1, rec, s0, e0, s1, e1))
        out[rec] = (np.array([s for s, _, _ in segs], dtype=np.int64), np.array([e for _, e, _ in segs], dtype=np.int64))
    return out


# ---- the draws of an epoch: one seeded index function for NativeTrainLoader (archives) and WavTrainLoader (audio) ----
def read_utt2spkid(utt2spkid_file):
    utt2spk = {}
    for line in open(utt2spkid_file):
        u, s = line.split()
        utt2spk[u] = int(s)
    return utt2spk


def balanced_repetitions(keys, utt2spk):
    """(repetitions per key, cap): the class balancing of the reference's datasets.py:23-31 - a key of a speaker with c utterances is
    listed max(1, cap // c) times, cap = min(500, (max c + 1) // 2)"""
    count = {}
    for s in utt2spk.values():
        count[s] = count.get(s, 0) + 1
    cap = min(500, int((max(count.values()) + 1) / 2))          # datasets.py:23-24
    return [max(1, cap // count[utt2spk[u]]) for u in keys], cap


def epoch_indices(n, seed, epoch, rank, world):
    """this rank's samples of the epoch: a permutation seeded like DistributedSampler.set_epoch, padded by wrap-around"""
    g = np.random.RandomState(seed + epoch)
    perm = g.permutation(n)
    total = -(-n // world) * world
    perm = np.concatenate([perm, perm[: total - n]])               # DistributedSampler pads by wrap-around
    return perm[rank: total: world]


def crop_rng(seed, epoch, rank):
    return np.random.RandomState((seed + epoch) * 7919 + rank)


def batch_draws(idx, batch_size, drop_last, lens, T_fixed, rng, sample_to_row, rows):
    """the batches of an epoch: (k, samples sel, their table rows, chunk length T, crop starts), the starts drawn one by one from
    rng.randint(0, rows - T + 1) (datasets.py:66) in batch order - `rows` is what a crop is taken from: the frames of an archive
    entry, the voiced frames of an audio entry"""
    k = 0
    for b0 in range(0, len(idx), batch_size):
        sel = idx[b0:b0 + batch_size]
        if len(sel) < batch_size and drop_last:
            break
        r = sample_to_row[sel]
        T = T_fixed if lens is None else int(lens[k])          # one chunk length per batch
        starts = [int(rng.randint(0, int(rows[i]) - T + 1)) for i in r]   # datasets.py:66
        yield k, sel, r, T, starts
        k += 1


class NativeTrainLoader:
    """Iterable over (features [B,F,T] pinned, labels [B] int64) batches of one epoch for this rank."""

    def __init__(self, scp_file, utt2spkid_file, chunk_size, batch_size, rank=0, world=1, seed=0, threads=4,
                 drop_last=False, prefetch=2, device=None, chunk_range=None):
        """chunk_range=(lo, hi, quantum): variable-length training - one chunk length per batch from
        datasets.chunk_length_schedule (seeded by (seed, epoch) only: the same length on every rank); chunk_size is then
        ignored and the pinned ring is sized for hi.
        device=None: batches are fresh pageable host tensors (the caller copies them; a copy from pageable memory is
        staged by the runtime before .cuda() returns, so nothing can overwrite it early).
        device=cuda:N: the loader owns a ring of PINNED staging buffers and the host->device copy: it issues the copy on
        its own copy stream (overlapping the previous step's kernels), records an event per ring slot, and the reader
        thread waits for that event before it refills the slot - the training loop never syncs with the host, so
        without this guard the reader could overwrite a slot whose asynchronous copy has not executed yet.  Yields
        device tensors, already ordered after the copy on the consumer's current stream.
        When every entry of the scp is a one-byte compressed 'CM ' matrix the ring holds the codes as they
        lie in the archive (a quarter of the bytes, no transpose) plus the small column headers; both are copied and decoded to
        float32 by spk_cm_decode on the copy stream, ahead of the same event.  With device=None, or 'FM ' entries among them, the
        reader decodes on the host and the batches are float32 as before - the same bits either way."""
        self.device = torch.device(device) if device is not None else None
        utt2spk = read_utt2spkid(utt2spkid_file)
        lines = [line.rstrip().split(None, 1) for line in open(scp_file)]
        reps, cap = balanced_repetitions([u for u, _ in lines], utt2spk)
        rx, lab = [], []
        for (u, r), rep in zip(lines, reps):
            rx.extend([r] * rep)
            lab.extend([utt2spk[u]] * rep)
        uniq = sorted(set(rx))
        pos = {r: i for i, r in enumerate(uniq)}
        self.table = ArkTable(uniq)
        self.sample_to_row = np.array([pos[r] for r in rx], dtype=np.int64)
        self.labels = np.array(lab, dtype=np.int64)
        self.chunk_range = tuple(int(v) for v in chunk_range) if chunk_range is not None else None
        self.T = int(chunk_size) if self.chunk_range is None else self.chunk_range[1]
        short = self.table.rows < self.T
        if short.any():
            raise AssertionError("%d utterances are shorter than the chunk size %d (reference: assert len(full_mat) >= seq_len)"
                                 % (int(short.sum()), self.T))
        self.bs, self.rank, self.world, self.seed, self.threads = batch_size, rank, world, seed, threads
        self.drop_last, self.prefetch = drop_last, prefetch
        self.epoch = 0
        print("Totally " + str(len(rx)) + " samples with at most " + str(cap) + " samples for one class")

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _indices(self):
        return epoch_indices(len(self.labels), self.seed, self.epoch, self.rank, self.world)

    def _lens(self):
        if self.chunk_range is None:
            return None
        from .datasets import chunk_length_schedule
        return chunk_length_schedule(self.chunk_range[0], self.chunk_range[1], self.chunk_range[2], len(self) + 1, self.seed, self.epoch)

    def draws(self):
        """the draws of the current epoch without reading anything: (k, samples, table rows, chunk length, crop starts) per batch"""
        return batch_draws(self._indices(), self.bs, self.drop_last, self._lens(), self.T, crop_rng(self.seed, self.epoch, self.rank),
                           self.sample_to_row, self.table.rows)

    def __len__(self):
        n = -(-len(self.labels) // self.world)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def __iter__(self):
        draws = self.draws()
        F = int(self.table.cols[0])
        q = queue.Queue(maxsize=self.prefetch)
        dev = self.device
        nslot = self.prefetch + 2
        as_codes = dev is not None and self.table.all_cm
        if as_codes:
            from . import features
            ring = [torch.empty(self.bs * F * self.T, dtype=torch.uint8).pin_memory() for _ in range(nslot)]
            hring = [torch.empty(self.bs * F * 4).pin_memory() for _ in range(nslot)]
        else:
            ring = [torch.empty(self.bs * F * self.T).pin_memory() for _ in range(nslot)] if dev is not None else None
        copied = [None] * nslot          # per slot: event recorded after the H2D copy that last read the slot

        def producer():
            try:
                for k, sel, rows, T, starts in draws:
                    slot = k % nslot
                    if ring is not None:
                        ev = copied[slot]
                        if ev is not None:
                            ev.synchronize()            # the device has finished reading this pinned buffer
                        buf = ring[slot][:len(sel) * F * T].view(len(sel), F, T)
                    else:
                        buf = torch.empty(len(sel), F, T)
                    if as_codes:
                        buf = (buf, hring[slot][:len(sel) * F * 4].view(len(sel), F, 4))
                        self.table.read_crop_codes(rows, starts, T, buf[0], buf[1], self.threads)
                    else:
                        self.table.read_crop(rows, starts, T, buf, self.threads)
                    q.put((slot, buf, torch.from_numpy(self.labels[sel])))
                q.put(None)
            except BaseException as e:      # surface reader errors in the training loop
                q.put(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        copy_stream = torch.cuda.Stream(device=dev) if dev is not None else None
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            slot, buf, lab = item
            if dev is None:
                yield buf, lab
                continue
            cur = torch.cuda.current_stream(dev)
            with torch.cuda.stream(copy_stream):
                if as_codes:         # bytes and headers across, then the decode, all before the event below
                    xg = features.decompress(buf[0].to(dev, non_blocking=True), buf[1].to(dev, non_blocking=True))
                else:
                    xg = buf.to(dev, non_blocking=True)
                yg = lab.pin_memory().to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            copied[slot] = ev
            cur.wait_event(ev)
            xg.record_stream(cur)
            yg.record_stream(cur)
            yield xg, yg
        th.join()


# ---- training from audio ----
SpanPlan = collections.namedtuple("SpanPlan", "frame_lo frame_hi first count rel")
SpanPlan.__doc__ = """plan_spans' result, one entry per row: the frames [frame_lo, frame_hi) of the utterance that are computed, the
samples [first, first + count) that are read, and rel [B, T]: the selected frames counted from frame_lo"""


def plan_spans(voiced_idx, v0, T, W, total_frames, opts, nsamp):
    """The span of each row's utterance that a chunk needs (numpy only).  Row b takes the voiced frames
    voiced_idx[b][v0[b] : v0[b] + T] (voiced_idx[b]: the ascending frame numbers of the voiced frames, or None: every frame) of an
    utterance of total_frames[b] frames and nsamp[b] samples; W: the window of the sliding CMN (0: none), opts: the framing options.
    The span [lo, hi) holds every frame that the whole-utterance CMN window of a selected frame covers, and is placed so that the
    window rule of spk_cmn_select applied to the span (shift the window into [0, hi - lo)) picks those very frames:
        lo = max(0, t_first - W/2), hi = min(Ttot, t_last - W/2 + W)
        lo == 0   -> hi = max(hi, min(W, Ttot))       a window clipped at the head is [0, min(W, Ttot))
        hi == Ttot -> lo = min(lo, max(0, Ttot - W))   a window clipped at the tail is [max(0, Ttot - W), Ttot)
    (DESIGN.md section 6k has the case analysis.)  hi - lo <= min(Ttot, t_last - t_first + 1 + 2 W)."""
    B = len(v0)
    v0 = np.asarray(v0, dtype=np.int64)
    Ttot = np.asarray(total_frames, dtype=np.int64)
    T, W = int(T), int(W)
    sel = np.empty((B, T), dtype=np.int64)
    ar = np.arange(T, dtype=np.int64)
    for b in range(B):
        sel[b] = v0[b] + ar if voiced_idx[b] is None else voiced_idx[b][v0[b]:v0[b] + T]
    t_first, t_last = sel[:, 0], sel[:, -1]
    assert (t_first >= 0).all() and (t_last < Ttot).all(), "plan_spans: a selected frame lies outside its utterance"
    if W > 0:
        lo = np.maximum(0, t_first - W // 2)
        hi = np.minimum(Ttot, t_last - W // 2 + W)
        hi = np.where(lo == 0, np.maximum(hi, np.minimum(W, Ttot)), hi)
        lo = np.where(hi == Ttot, np.minimum(lo, np.maximum(0, Ttot - W)), lo)
    else:
        lo, hi = t_first.copy(), t_last + 1
    from . import features
    first, last = features.span_samples(opts, lo, hi, nsamp)
    return SpanPlan(lo, hi, first, last - first, (sel - lo[:, None]).astype(np.int32))


RESAMPLE_SPAN_MARGIN = 1        # samples resample_input_span adds at either end of the windows' union (before the cut to the file)


def resample_input_span(ofirst, ocount, nsamp, fi, fo):
    """The samples of an utterance of nsamp samples that outputs [ofirst, ofirst + ocount) of its resampling from fi to fo Hz read
    (numpy only; integers or integer arrays, ocount >= 1): (first, count).  With features.resample_tables' (iu, ou, K, first),
    output j reads the window [a(j), a(j) + K), a(j) = first[j % ou] + (j // ou) * iu.  The span is
        [a(ofirst) - MARGIN, a(ofirst + ocount - 1) + K + MARGIN)   cut to [0, nsamp),   MARGIN = RESAMPLE_SPAN_MARGIN = 1
    which holds the union of the windows of the range: a(j) is ceil(x_j) of a value x_j that grows with j, computed in fp64 with an
    error far below 1/2, so a later window can start before an earlier one by at most one sample - hence
    the margin, instead of an assumption that a(j) is monotone across a unit boundary.  The span is never longer than the union
    plus 2 MARGIN, and it is never empty (at least one sample, inside the file)."""
    from . import features
    t = features._resample_cached(features._int_rate(fi, "resample_input_span"), features._int_rate(fo, "resample_input_span"), None)
    o, m, n = (np.asarray(v, dtype=np.int64) for v in (ofirst, ocount, nsamp))
    last = o + m - 1
    a0 = t.first[o % t.ou] + (o // t.ou) * t.iu
    a1 = t.first[last % t.ou] + (last // t.ou) * t.iu
    lo = np.minimum(np.maximum(a0 - RESAMPLE_SPAN_MARGIN, 0), np.maximum(n - 1, 0))
    hi = np.maximum(np.minimum(a1 + t.K + RESAMPLE_SPAN_MARGIN, n), lo + 1)
    return lo, hi - lo


class WavTrainLoader:
    """NativeTrainLoader for audio: iterable over (chunks [B, F, T] cuda float32, labels [B] cuda int64) of one epoch for this
    rank, the chunks computed from 16-bit PCM WAV files as they are drawn.  Same class balancing, permutation, sharding, chunk
    lengths and crop starts as NativeTrainLoader over the archive that compute_fbank.py / compute_mfcc.py --egs --vad-scp
    --cmn-window W writes for the same wav.scp (one seeded index function, batch_draws): a draw is (entry, first voiced frame v0,
    length T), and the chunk is columns v0 .. v0 + T - 1 of that entry's matrix, to one fp32 ulp.

    wav_scp: the recipe's wav.scp - plain paths and the wav-reverberate entries features.parse_wav_entry accepts, which are
    applied to the span that is read (features.AugmentPool), and the `sox -t wav PATH -t wav - speed F |` entries of a
    speed-perturbed copy (local/perturb_data_dir_speed.sh), which are resampled on the GPU: frames, voiced frames and the VAD
    vector of such an entry are those of the PERTURBED utterance, of num_resampled(nsamp, *speed_rates(F, rate)) samples - the
    archive compute_fbank.py writes for the same wav.scp - and the reader reads the span of the file that the span of the perturbed
    signal needs (resample_input_span); vad_scp: the 0/1 vector per key (None: every frame is voiced);
    opts: FbankOptions or MfccOptions, cmn: CmnOptions or None, feat_seed: the dither seed (compute_fbank.py --seed).
    The reader thread plans the spans (plan_spans) and reads them (WavTable.read_span) into a ring of pinned int16 slots; the
    consumer copies a slot and its numbers on the loader's copy stream and runs features.ChunkFrontend there, behind the previous
    training step; one event per slot lets the reader refill it.  Refused, before anything is launched: a file at another rate
    than opts.sample_frequency, a pipe entry of another shape, a key without a label or without a VAD vector, a VAD vector whose
    length is not the file's frame count, a file shorter than one frame; an entry with fewer than T voiced frames raises the
    AssertionError of NativeTrainLoader."""

    SLACK = 8        # frames of slack per row of the pinned ring beyond T + W

    def __init__(self, wav_scp, utt2spkid_file, chunk_size, batch_size, opts, cmn=None, vad_scp=None, feat_seed=0, rank=0, world=1,
                 seed=0, threads=4, drop_last=False, prefetch=2, device="cuda", chunk_range=None, shuffle=True, times=None):
        from . import features, kaldi_io
        self.device = torch.device(device)
        self.opts, self.cmn, self.feat_seed, self.times = opts, cmn, feat_seed, times
        self.W = int(cmn.cmn_window) if cmn is not None else 0
        keys, entries = features.read_wav_scp(wav_scp) if isinstance(wav_scp, str) else wav_scp      # refuses other pipe entries
        utt2spk = read_utt2spkid(utt2spkid_file)
        for k in keys:
            if k not in utt2spk:
                raise ValueError("%s: %s has no label in %s" % (wav_scp, k, utt2spkid_file))
        fs = int(opts.sample_frequency)
        try:
            self.table = WavTable([e.path for e in entries], fs)
        except RuntimeError as e:
            raise ValueError("%s (--sample-frequency is %d: resample the file offline, compute_fbank.py --allow-downsample / "
                             "--allow-upsample)" % (e, fs))
        n = len(keys)
        short = np.nonzero((self.table.nsamp < opts.frame_len) & np.asarray([e.speed is None for e in entries]))[0]
        if short.size:
            raise ValueError("%s: %d samples, shorter than one frame (%d)" % (self.table.paths[short[0]],
                                                                              int(self.table.nsamp[short[0]]), opts.frame_len))
        # speed-perturbed entries: the rates of their resampling and their length on the perturbed clock; a plain entry has its own
        self.speed = [e.speed for e in entries]
        self.has_speed = any(v is not None for v in self.speed)
        self.nsamp_out = self.table.nsamp.astype(np.int64).copy()
        self.group = np.zeros(n, dtype=np.int64)        # 0: plain, g > 0: rates[g - 1]
        self.rates = []
        for i, e in enumerate(entries):
            if e.speed is None:
                continue
            if e.augmented:
                raise ValueError("%s: speed %s does not combine with wav-reverberate entries" % (keys[i], e.speed))
            fi, fo = features.speed_rates(e.speed, fs)
            if (fi, fo) not in self.rates:
                features.check_speed_table("%s (speed %s)" % (keys[i], e.speed), fi, fo)
                self.rates.append((fi, fo))
            self.group[i] = 1 + self.rates.index((fi, fo))
            self.nsamp_out[i] = features.num_resampled(int(self.table.nsamp[i]), fi, fo)
            if self.table.nsamp[i] >= 2 ** 30 or self.nsamp_out[i] >= 2 ** 30:
                raise ValueError("%s: %s has %d samples (%d at speed %s): the span resampler takes fewer than 2^30"
                                 % (keys[i], self.table.paths[i], int(self.table.nsamp[i]), int(self.nsamp_out[i]), e.speed))
        short = np.nonzero(self.nsamp_out < opts.frame_len)[0]
        if short.size:
            raise ValueError("%s: %s has %d samples at speed %s, shorter than one frame (%d)"
                             % (keys[short[0]], self.table.paths[short[0]], int(self.nsamp_out[short[0]]), self.speed[short[0]],
                                opts.frame_len))
        self.frames = np.asarray([opts.num_frames(int(v)) for v in self.nsamp_out], dtype=np.int64)
        self.voiced = [None] * n
        self.rows = self.frames.copy()
        if vad_scp is not None:
            vad = dict(l.split(None, 1) for l in open(vad_scp) if l.strip())
            for i, k in enumerate(keys):
                if k not in vad:
                    raise ValueError("%s has no entry in --vad-scp %s" % (k, vad_scp))
                v = kaldi_io.read_vec_flt(vad[k].strip())
                if v.shape[0] != self.frames[i]:
                    raise ValueError("%s: %s has %d frames but its vector in --vad-scp %s has %d"
                                     % (k, self.table.paths[i], int(self.frames[i]), vad_scp, v.shape[0]))
                self.voiced[i] = np.nonzero(v != 0)[0].astype(np.int32)
                self.rows[i] = self.voiced[i].size
        self.utt_ids = np.asarray([features.utt_id(k) for k in keys], dtype=np.int64)
        self.augmented = any(e.augmented for e in entries)
        self.pool = None
        if self.augmented:
            self.pool = features.AugmentPool(features.WavAugmentation(self.table, entries), self.device, fs)
        self.frontend = features.ChunkFrontend(opts, cmn, feat_seed, self.pool)
        reps, cap = balanced_repetitions(keys, utt2spk)
        self.sample_to_row = np.repeat(np.arange(n, dtype=np.int64), reps)
        self.labels = np.repeat(np.asarray([utt2spk[k] for k in keys], dtype=np.int64), reps)
        self.keys = keys
        self.chunk_range = tuple(int(v) for v in chunk_range) if chunk_range is not None else None
        self.T = int(chunk_size) if self.chunk_range is None else self.chunk_range[1]
        short = self.rows < self.T
        if short.any():
            raise AssertionError("%d utterances are shorter than the chunk size %d (reference: assert len(full_mat) >= seq_len)"
                                 % (int(short.sum()), self.T))
        self.bs, self.rank, self.world, self.seed, self.threads = batch_size, rank, world, seed, threads
        self.drop_last, self.prefetch, self.shuffle = drop_last, prefetch, shuffle
        self.epoch = 0
        self.reader_seconds = []        # host time of the reader thread per batch (plan + read)
        print("Totally " + str(len(self.labels)) + " samples with at most " + str(cap) + " samples for one class")

    dim = property(lambda self: self.frontend.dim)

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _indices(self):
        if not self.shuffle:            # validation: every sample once, in order (world 1)
            return np.arange(len(self.labels))
        return epoch_indices(len(self.labels), self.seed, self.epoch, self.rank, self.world)

    _lens = NativeTrainLoader._lens
    __len__ = NativeTrainLoader.__len__

    def draws(self):
        """the draws of the current epoch without reading anything, as NativeTrainLoader.draws"""
        return batch_draws(self._indices(), self.bs, self.drop_last, self._lens(), self.T, crop_rng(self.seed, self.epoch, self.rank),
                           self.sample_to_row, self.rows)

    def plan(self, rows, starts, T):
        """the span plan of a batch, on the clock the frames are counted on (the perturbed one for a speed entry)"""
        r = np.asarray(rows, dtype=np.int64)
        return plan_spans([self.voiced[i] for i in r], starts, T, self.W, self.frames[r], self.opts, self.nsamp_out[r])

    def input_spans(self, rows, p):
        """(first, count) of the samples of each row's FILE that the plan p of the batch needs: p's own for a plain row,
        resample_input_span of p's output samples for a speed row"""
        r = np.asarray(rows, dtype=np.int64)
        first, count = p.first.astype(np.int64).copy(), p.count.astype(np.int64).copy()
        for g in np.unique(self.group[r]):
            if g:
                m = self.group[r] == g
                first[m], count[m] = resample_input_span(p.first[m], p.count[m], self.table.nsamp[r[m]], *self.rates[g - 1])
        return first, count

    def __iter__(self):
        import time
        from . import features
        draws = self.draws()
        dev, bs, S = self.device, self.bs, self.opts.frame_sh
        nslot = self.prefetch + 2
        # a row of the ring: the samples of T + W + SLACK frames; a batch that needs more (sparse voiced frames) gets its own buffer
        ring_n = (self.T + self.W + self.SLACK) * S + self.opts.frame_len
        # a speed row reads fi / fo input samples per sample of the span, the filter's taps and the margin: sized for the largest
        ring_n = max([ring_n] + [-(-ring_n * fi // fo) + features.resample_tables(fi, fo)[2] + 2 * RESAMPLE_SPAN_MARGIN + 1
                                 for fi, fo in self.rates])
        ring_n = -(-ring_n // 8) * 8
        ring_t = self.T + 2 * self.W + self.SLACK
        ring = [torch.empty(bs * ring_n, dtype=torch.int16).pin_memory() for _ in range(nslot)]
        # the numbers of a batch: int64 [3][B] (first, total, utt id), int32 [3][B] (count, frame0, nframes) + rel [B][Tcap]; with
        # speed entries two more rows each: (ofirst, ototal) and (ocount, the rows grouped by factor)
        n64, n32 = (5, 5) if self.has_speed else (3, 3)
        iring = [(torch.empty(n64 * bs, dtype=torch.int64).pin_memory(),
                  torch.empty(bs * (n32 + ring_t), dtype=torch.int32).pin_memory()) for _ in range(nslot)]
        copied = [None] * nslot
        q = queue.Queue(maxsize=self.prefetch)

        def producer():
            try:
                for k, sel, rows, T, starts in draws:
                    t0 = time.perf_counter()
                    B = len(sel)
                    p = self.plan(rows, starts, T)
                    ifirst, icount = self.input_spans(rows, p) if self.has_speed else (p.first, p.count)
                    Nmax = -(-int(icount.max()) // 8) * 8
                    Tcap = int((p.frame_hi - p.frame_lo).max())
                    slot = k % nslot
                    ev = copied[slot]
                    if ev is not None:
                        ev.synchronize()            # the device has finished reading this slot's pinned buffers
                    fits = Nmax <= ring_n and Tcap <= ring_t
                    pcm = (ring[slot][:B * Nmax] if fits else torch.empty(B * Nmax, dtype=torch.int16).pin_memory()).view(B, Nmax)
                    m64 = iring[slot][0][:n64 * B].view(n64, B)
                    m32 = (iring[slot][1][:B * (n32 + Tcap)] if fits else torch.empty(B * (n32 + Tcap), dtype=torch.int32).pin_memory())
                    self.table.read_span(rows, ifirst, icount, Nmax, pcm, self.threads)
                    m64n, m32n = m64.numpy(), m32.numpy()
                    m64n[0], m64n[1], m64n[2] = ifirst, self.table.nsamp[rows], self.utt_ids[rows]
                    m32n[:B], m32n[B:2 * B], m32n[2 * B:3 * B] = icount, p.frame_lo, p.frame_hi - p.frame_lo
                    sp = None
                    if self.has_speed:
                        g = self.group[rows]
                        order = np.argsort(g, kind="stable")
                        lo = np.searchsorted(g[order], np.arange(len(self.rates) + 2))
                        m64n[3], m64n[4] = p.first, self.nsamp_out[rows]
                        m32n[3 * B:4 * B], m32n[4 * B:5 * B] = p.count, order
                        if lo[1] < B:       # a batch without a speed row takes the plain chain
                            sp = ([self.rates[j - 1] + (int(lo[j]), int(lo[j + 1])) for j in range(1, len(self.rates) + 1)
                                   if lo[j + 1] > lo[j]], (0, int(lo[1])), -(-int(p.count.max()) // 4) * 4)
                    rel = m32n[n32 * B:].reshape(B, Tcap)
                    rel[:, :T] = p.rel
                    rel[:, T:] = 0
                    aplan = self.pool.plan(rows) if self.pool is not None else None
                    self.reader_seconds.append(time.perf_counter() - t0)
                    q.put((slot, pcm, m64, m32, T, Tcap, aplan, sp, torch.from_numpy(self.labels[sel])))
                q.put(None)
            except BaseException as e:      # surface reader errors in the training loop
                q.put(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        copy_stream = torch.cuda.Stream(device=dev)
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            slot, pcm, m64, m32, T, Tcap, aplan, sp, lab = item
            B = pcm.shape[0]
            cur = torch.cuda.current_stream(dev)
            with torch.cuda.stream(copy_stream):
                times = {} if self.times is not None else None
                if times is not None:
                    h0, h1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    h0.record()
                pg = pcm.to(dev, non_blocking=True)
                g64 = m64.to(dev, non_blocking=True)
                g32 = m32.to(dev, non_blocking=True)
                yg = lab.pin_memory().to(dev, non_blocking=True)
                if times is not None:
                    h1.record()
                    times["h2d"] = (h0, h1)
                if sp is not None:
                    sp = features.SpeedBatch(g64[3], g64[4], g32[3 * B:4 * B], g32[4 * B:5 * B], *sp)
                xg = self.frontend(pg, g32[:B], g64[0], g64[1], g32[B:2 * B], g32[2 * B:3 * B], g32[n32 * B:].view(B, Tcap), T,
                                   g64[2], aplan, times, sp)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            if times is not None:
                self.times.append(times)
            copied[slot] = ev
            cur.wait_event(ev)
            xg.record_stream(cur)
            yg.record_stream(cur)
            yield xg, yg
        th.join()
