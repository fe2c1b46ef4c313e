"""An independent restatement of DESIGN.md section 6r for the tests: every speaker is rasterised onto an array of ticks and the rule is
applied tick by tick.  Nothing here is shared with pytorch_kaldi_resnet_amd.diarize: no interval arithmetic, no potentials.  The
assignment is solved by trying every injective mapping while min(Sr, Sh) <= 6, beyond that by scipy.optimize.linear_sum_assignment
(HAVE_SCIPY says whether it is importable; the tests skip the larger cases where it is not).  Merge lists are cut by replaying them one
merge at a time."""
import itertools
import math

import numpy as np

try:
    from scipy.optimize import linear_sum_assignment
    HAVE_SCIPY = True
except ImportError:                                                # pragma: no cover
    HAVE_SCIPY = False


def tick(t, tick_s):
    return int(math.floor(t / tick_s + 0.5))


def raster(turns, tick_s, T):
    """turns [(speaker, start s, dur s)] -> (names in order of first appearance, bool [S][T]: speaker active at tick t)"""
    names = []
    for spk, _, _ in turns:
        if spk not in names:
            names.append(spk)
    grid = np.zeros((len(names), T), dtype=bool)
    for spk, start, dur in turns:
        a = tick(start, tick_s)
        b = a + tick(dur, tick_s)
        assert 0 <= a and b <= T, (a, b, T)
        if b > a:
            grid[names.index(spk), a:b] = True
    return names, grid


def horizon(ref, hyp, uem, tick_s):
    end = [tick(s, tick_s) + tick(d, tick_s) for _, s, d in list(ref) + list(hyp)] + [tick(e, tick_s) for _, e in (uem or [])]
    return max(end + [0]) + 2


def best_assignment(C):
    """the largest sum of C[i][map(i)] over one-to-one partial mappings"""
    Sr, Sh = C.shape
    if Sr == 0 or Sh == 0:
        return 0
    if min(Sr, Sh) <= 6:
        A = C if Sr <= Sh else C.T                                 # rows: the smaller side; every row mapped (C >= 0: no loss)
        best = 0
        for cols in itertools.permutations(range(A.shape[1]), A.shape[0]):
            best = max(best, sum(int(A[i, j]) for i, j in enumerate(cols)))
        return best
    assert HAVE_SCIPY
    i, j = linear_sum_assignment(C.astype(np.float64), maximize=True)       # (tick counts here are far below 2^53)
    return int(C[i, j].sum())


def der(ref, hyp, uem=None, collar=0.25, ignore_overlap=False, tick_s=0.01):
    """ref, hyp: [(speaker, start s, dur s)] of one recording; uem: [(start s, end s)] or None -> dict(scored, miss, fa, conf, opt, der,
    C, ref_names, hyp_names)"""
    T = horizon(ref, hyp, uem, tick_s)
    rn, R = raster(ref, tick_s, T)
    hn, H = raster(hyp, tick_s, T)
    S = np.zeros(T, dtype=bool)
    turns = [(tick(s, tick_s), tick(s, tick_s) + tick(d, tick_s)) for _, s, d in ref]
    turns = [(a, b) for a, b in turns if b > a]
    if uem is not None:
        for s, e in uem:
            S[tick(s, tick_s):tick(e, tick_s)] = True
    elif turns:
        S[min(a for a, _ in turns):max(b for _, b in turns)] = True
    c = tick(collar, tick_s)
    for a, b in turns:
        for edge in (a, b):
            S[max(edge - c, 0):max(edge + c, 0)] = False
    Nr, Nh = R.sum(axis=0), H.sum(axis=0)
    if ignore_overlap:
        S &= Nr < 2
    scored = int(Nr[S].sum())
    miss = int(np.maximum(Nr - Nh, 0)[S].sum())
    fa = int(np.maximum(Nh - Nr, 0)[S].sum())
    C = np.array([[int((R[i] & H[j] & S).sum()) for j in range(len(hn))] for i in range(len(rn))], dtype=np.int64).reshape(len(rn), len(hn))
    opt = best_assignment(C)
    conf = int(np.minimum(Nr, Nh)[S].sum()) - opt
    return {"scored": scored, "miss": miss, "fa": fa, "conf": conf, "opt": opt, "C": C, "ref_names": rn, "hyp_names": hn,
            "der": float("nan") if scored == 0 else (miss + fa + conf) / scored}


def five(d):
    return (d["scored"], d["miss"], d["fa"], d["conf"], d["opt"])


def cut(merges, costs, n, threshold):
    """replays the merge list of one recording of n windows: merges [(i, j)] and their costs -> labels from 1 by lowest member window
    after the longest prefix whose costs all satisfy c <= -threshold"""
    member = list(range(n))
    for (i, j), c in zip(merges, costs):
        if not c <= -threshold:
            break
        member = [i if x == j else x for x in member]
    names = sorted(set(member))
    return [names.index(x) + 1 for x in member]


def pieces(windows, labels):
    """windows [(start tick, end tick)] sorted by (start, end) -> [(label, start, end)] with the adjacent pairs of different labels that
    overlap cut at (a + b) // 2"""
    w = [[a, b, l] for (a, b), l in zip(windows, labels)]
    for cur, nxt in zip(w[:-1], w[1:]):
        if cur[2] != nxt[2] and nxt[0] < cur[1]:
            cur[1] = nxt[0] = (nxt[0] + cur[1]) // 2
    return [(l, a, b) for a, b, l in w]
