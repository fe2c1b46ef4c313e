"""Numpy restatement of the span form of the resampler (include/spkwav.h; DESIGN.md sections 6e "Resampling" and 6k): which samples
of an utterance a range of outputs reads, by brute force over every window, and what the span launch writes, in terms of the
whole-utterance resampler of tests/resample_ref.py."""
import numpy as np

import resample_ref


def window_starts(o0, o1, iu, ou, first):
    """a(j) = first[j % ou] + (j // ou) * iu for j in [o0, o1)"""
    j = np.arange(o0, o1, dtype=np.int64)
    return np.asarray(first, dtype=np.int64)[j % ou] + (j // ou) * iu


def window_union(o0, o1, nsamp, iu, ou, K, first):
    """(lo, hi): the hull of every index of every window [a(j), a(j) + K), j in [o0, o1), that lies inside [0, nsamp); the windows of
    consecutive outputs overlap (K is far above iu / ou + 1), so the hull is the union.  None when no index is inside."""
    a = window_starts(o0, o1, iu, ou, first)
    idx = (a[:, None] + np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
    idx = idx[(idx >= 0) & (idx < nsamp)]
    return (int(idx.min()), int(idx.max()) + 1) if idx.size else None


def zero_outside_row(x, ifirst, icount):
    """the utterance as the span kernel sees it from a row that holds samples [ifirst, ifirst + icount): 0 everywhere else"""
    z = np.zeros_like(np.asarray(x))
    z[ifirst:ifirst + icount] = x[ifirst:ifirst + icount]
    return z


def resample_span(x, ifirst, icount, ofirst, ocount, fi, fo, Nmax_out, dtype=np.float64):
    """what the span launch writes for one row, [Nmax_out]: outputs [ofirst, ofirst + ocount) of the resampling of the utterance x
    as the row sees it (zero_outside_row), zeros where the resampled utterance has no such output and from ocount on"""
    y = resample_ref.resample(zero_outside_row(x, ifirst, icount), fi, fo, dtype)
    out = np.zeros(Nmax_out, dtype=dtype)
    part = y[ofirst:ofirst + ocount]
    out[:len(part)] = part
    return out
