"""The scoring cases tests/test_der_cpu.py and tests/test_der_gpu.py share.  Times lie on the 10 ms grid and the
tests score with tick = 0.01, so a case spans at most a few thousand ticks and tests/der_ref.py can rasterise it."""
import numpy as np

import der_ref

TICK = 0.01


def case(ref, hyp, uem=None, collar=0.0, ignore_overlap=False):
    return {"ref": ref, "hyp": hyp, "uem": uem, "collar": collar, "ignore_overlap": ignore_overlap}


def random_turns(rng, speakers, turns, T, longest=3.0):
    """`turns` turns of `speakers` speakers (each speaks at least once while turns >= speakers) on the 10 ms grid inside [0, T) s"""
    out = []
    for t in range(turns):
        s = round(rng.uniform(0.0, T - 0.05), 2)
        d = round(min(rng.uniform(0.01, longest), T - s), 2)
        out.append(("s%d" % (t if t < speakers else rng.randint(speakers)), s, d))
    return out


def random_case(seed, Sr, Sh, nref, nhyp, T=20.0, collar=0.05, ignore_overlap=False, uem=None):
    rng = np.random.RandomState(seed)
    ref = random_turns(rng, Sr, nref, T)
    hyp = [("h%s" % s[1:], a, d) for s, a, d in random_turns(rng, Sh, nhyp, T, 1.0)]
    return case(ref, hyp, uem, collar, ignore_overlap)


# a hand-computed case (collar 0): S = [0, 8) s.  x [0, 5) and y [5, 7) leave [7, 8) unheard: miss 100 ticks.  w [1, 2) doubles x while A
# alone speaks: false alarm 100.  z [9, 10) lies outside S.  C[A][x] = 400, C[A][w] = 100, C[B][x] = 100, C[B][y] = 200: opt = A-x +
# B-y = 600, the sum of min(Nr, Nh) is 700 (all of [0, 7)), so confusion = 100: x goes on while B speaks in [4, 5).
HAND = case([("A", 0.0, 4.0), ("B", 4.0, 4.0)], [("x", 0.0, 5.0), ("y", 5.0, 2.0), ("z", 9.0, 1.0), ("w", 1.0, 1.0)])
HAND_FIVE = (800, 100, 100, 100, 600)

CASES = {
    "hand": HAND,
    "empty_hyp": case([("A", 0.5, 2.0), ("B", 2.0, 2.0)], [], collar=0.1),
    "hyp_outside_S": case([("A", 1.0, 2.0)], [("x", 0.0, 0.9), ("y", 3.5, 2.0)], collar=0.25),
    "nothing_scored": case([("A", 1.0, 0.3)], [("x", 0.0, 2.0)], collar=0.25),
    "collar_removes_a_turn": case([("A", 1.0, 0.3), ("B", 3.0, 4.0)], [("x", 0.0, 5.0), ("y", 5.0, 3.0)], collar=0.25),
    "collar_clipped_at_0": case([("A", 0.1, 3.0), ("B", 3.1, 2.0)], [("x", 0.0, 2.0), ("y", 2.0, 4.0)], collar=0.25),
    "ref_overlap": case([("A", 0.0, 5.0), ("B", 3.0, 5.0), ("C", 4.0, 2.0)], [("x", 0.0, 4.0), ("y", 3.5, 5.0)], collar=0.1),
    "ref_overlap_ignored": case([("A", 0.0, 5.0), ("B", 3.0, 5.0), ("C", 4.0, 2.0)], [("x", 0.0, 4.0), ("y", 3.5, 5.0)], collar=0.1,
                                ignore_overlap=True),
    "uem_two_regions": case([("A", 0.0, 5.0), ("B", 5.0, 5.0)], [("x", 0.0, 6.0), ("y", 6.0, 6.0)], uem=[(1.0, 4.0), (5.5, 11.0)],
                            collar=0.1),
    "one_speaker_twice": case([("A", 0.0, 3.0), ("A", 2.0, 3.0), ("B", 6.0, 2.0), ("B", 6.5, 0.5)],
                              [("x", 0.0, 2.5), ("x", 1.0, 3.0), ("x", 0.5, 1.0), ("y", 5.0, 4.0), ("y", 6.0, 1.0)], collar=0.1),
    "more_ref_than_hyp": random_case(11, 5, 2, 14, 9),
    "more_hyp_than_ref": random_case(12, 2, 6, 7, 20),
    "tie_one_hyp": case([("A", 0.0, 2.0), ("B", 2.0, 2.0)], [("x", 0.0, 4.0)]),
    "tie_two_by_two": case([("A", 0.0, 2.0), ("B", 2.0, 2.0)], [("x", 0.0, 1.0), ("y", 1.0, 1.0), ("x", 2.0, 1.0), ("y", 3.0, 1.0)]),
    "labels_not_consecutive": case([("A", 0.0, 3.0), ("B", 3.0, 3.0)], [("17", 0.0, 2.0), ("5", 2.0, 2.5), ("1000", 4.5, 1.5)], collar=0.1),
    "random_overlap_ignored": random_case(13, 4, 4, 16, 24, ignore_overlap=True, uem=[(0.5, 9.0), (9.5, 19.0)]),
}

_REF = {}


def reference(name):
    """der_ref.der of a case, computed once"""
    if name not in _REF:
        c = CASES[name]
        _REF[name] = der_ref.der(c["ref"], c["hyp"], c["uem"], c["collar"], c["ignore_overlap"], TICK)
    return _REF[name]


def check_case(D, name, backend):
    """diarize.der on one case against the reference: the five integers, the DER, and a mapping that is one-to-one and attains opt"""
    c, want = CASES[name], reference(name)
    hyp = {"rec": c["hyp"]} if c["hyp"] else {}
    got = D.der({"rec": c["ref"]}, hyp, uem=None if c["uem"] is None else {"rec": c["uem"]}, collar=c["collar"],
                ignore_overlap=c["ignore_overlap"], tick=TICK, backend=backend)
    p = got["per_recording"]["rec"]
    five = (p["scored"], p["miss"], p["fa"], p["conf"], p["opt"])
    assert five == der_ref.five(want), (name, backend, five, der_ref.five(want))
    assert (p["der"] != p["der"] and want["der"] != want["der"]) or p["der"] == want["der"], (name, p["der"], want["der"])
    m = p["mapping"]
    assert len(set(m.values())) == len(m), (name, m)
    assert sum(int(want["C"][want["ref_names"].index(a), want["hyp_names"].index(b)]) for a, b in m.items()) == want["opt"], (name, m)
    assert got["total"]["scored"] == p["scored"] and got["host_jobs"] == 0
    return got


# ---- merge lists ------------------------------------------------------------------------------------------------------------------------
def merge_case(D, sizes, seed, backend="host"):
    """random symmetric scores of recordings of the given sizes, clustered to one cluster -> (scores, rec_off, merges, cost, n_merges)"""
    rng = np.random.RandomState(seed)
    mats = []
    for n in sizes:
        a = rng.randn(n, n).astype(np.float32)
        mats.append(np.triu(a) + np.triu(a, 1).T)
    scores = np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0, np.float32)
    rec_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    _, merges, cost, nm = D.cluster(scores, rec_off, None, None, backend)
    return scores, rec_off, merges, cost, nm


def cut_thresholds(cost, rec_off, nm, K=None):
    """below every cost's threshold, above every one, exactly -cost of a merge of every recording, both infinities, one value twice;
    with K: padded with a grid to K values"""
    used = np.concatenate([cost[rec_off[r]:rec_off[r] + nm[r]] for r in range(len(nm))] + [np.zeros(1)])
    th = [-used.max() - 1.0, -used.min() + 1.0, np.inf, -np.inf]
    for r in range(len(nm)):
        if nm[r]:
            th.append(-cost[rec_off[r] + nm[r] // 2])
    th.append(th[-1])
    if K is not None:
        th = (th + list(np.linspace(-used.max(), -used.min(), max(K - len(th), 0))))[:K]
    return np.array(th, dtype=np.float64)


# ---- planted speakers --------------------------------------------------------------------------------------------------------------------
def planted_recording(reco, turns, seed, dim=16, window=1.5, period=0.75, noise=0.05):
    """turns [(speaker index, start s, end s)] that tile a recording -> (segments, embeddings [n][dim], reference turns): sliding windows
    on the 10 ms grid, each window embedded near the centre of the speaker who holds its midpoint"""
    rng = np.random.RandomState(seed)
    centres = np.linalg.qr(rng.randn(dim, dim))[0][:max(t[0] for t in turns) + 1] * 4.0
    end = max(t[2] for t in turns)
    segs, emb = [], []
    w = 0
    while w * period + window <= end + 1e-9:
        a, b = round(w * period, 2), round(w * period + window, 2)
        mid = 0.5 * (a + b)
        spk = [t[0] for t in turns if t[1] <= mid < t[2]][0]
        segs.append(("%s-%08d-%08d" % (reco, round(a * 100), round(b * 100)), reco, a, b))
        emb.append(centres[spk] + noise * rng.randn(dim))
        w += 1
    return segs, np.array(emb), [("spk%d" % t[0], t[1], round(t[2] - t[1], 2)) for t in turns]
