"""VBx resegmentation on the GPU (spk_vbx_batch in csrc/diar.hip, ops.vbx_batch, diarize.vbx) against
tests/vbx_ref.py.

The tolerance rule of section 6o: for each input and each of gamma, pi (absolute) and the ELBO (relative) the bound is
M * e64 + floor, e64 the error of vbx_ref in float64 against vbx_ref in numpy.longdouble on the same input (computed here, shared
through vbx_ref's caches), floor = 2^-49, M = vbx_ref.M_FACTOR.  Run with -s to see the largest error, the bound and the ratio
err / (e64 + floor) of every launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vbx_ref as V  # noqa: E402

GUARD = 64
SENT = -7.0


@pytest.fixture(scope="module")
def ops():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops
    return ops


@pytest.fixture(scope="module")
def diarize():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize
    return diarize


def up(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def banded(shape, fill, dtype=torch.float64):
    """a tensor of `shape` inside a larger one filled with `fill`: (the whole buffer, the view)"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return big, big[GUARD:GUARD + n].view(*shape)


def bands_intact(big, fill):
    return bool((big[:GUARD] == fill).all()) and bool((big[-GUARD:] == fill).all())


# ---- batches ------------------------------------------------------------------------------------------------------------------------
# per D: (T, S) of the recordings of one launch.  T: 1, 2, 63, 64, 65 and 257; S: 1, 2, 16 and 64; Smax = 64 with n_states 1, 3 and 64
LAUNCHES = {1: [(1, 1), (2, 2), (63, 3), (64, 16), (65, 2), (257, 4)],
            3: [(1, 1), (2, 2), (63, 3), (64, 16), (65, 2), (257, 4)],
            4: [(1, 1), (2, 2), (63, 3), (64, 16), (65, 2), (257, 4)],
            5: [(1, 1), (2, 3), (63, 64), (64, 3), (65, 64), (257, 16)],
            150: [(1, 1), (2, 2), (63, 3), (64, 16), (65, 2), (257, 4)],
            512: [(1, 1), (64, 2), (65, 16), (257, 4)]}
_BATCH = {}


def batch(D, Fa=0.3, Fb=17.0, loopP=0.99, iters=4):
    """the recordings of LAUNCHES[D] laid out as one batch, with the yardstick of each (made once)"""
    key = (D, Fa, Fb, loopP, iters)
    if key not in _BATCH:
        Phi = V.planted(1, D, 2, 1, seed=D)[1]
        recs = []
        for r, (T, S) in enumerate(LAUNCHES[D]):
            X, _, truth, first = V.planted(T, D, S, min(S, 3), seed=100 * D + r, Phi=Phi)
            g0 = V.init_gamma(first, S)
            if (D, T) == (5, 65):                                          # a one-hot start: most of the 64 states are empty
                g0 = (first[:, None] == np.arange(S)[None, :]).astype(np.float64)
            p0 = np.full(S, 1.0 / S)
            recs.append({"X": X, "gamma0": g0, "pi0": p0, "S": S, "T": T, "y": V.Yardstick(X, Phi, g0, p0, Fa, Fb, loopP, iters, -np.inf)})
        _BATCH[key] = pack(recs, Phi)
    return _BATCH[key]


def pack(recs, Phi, Smax=None):
    Smax = Smax or max(c["gamma0"].shape[1] for c in recs)
    rec_off = np.concatenate([[0], np.cumsum([len(c["X"]) for c in recs])]).astype(np.int64)
    gamma = np.full((int(rec_off[-1]), Smax), np.nan)                      # columns at or beyond n_states must not be read
    pi = np.full((len(recs), Smax), np.nan)
    for r, c in enumerate(recs):
        S = c["gamma0"].shape[1]
        gamma[rec_off[r]:rec_off[r + 1], :S] = c["gamma0"]
        pi[r, :S] = c["pi0"]
    return {"recs": recs, "Phi": Phi, "X": np.concatenate([c["X"] for c in recs]), "rec_off": rec_off, "gamma0": gamma, "pi0": pi,
            "n_states": np.array([c["gamma0"].shape[1] for c in recs], dtype=np.int32), "Smax": Smax}


def launch(ops, b, Fa=0.3, Fb=17.0, loopP=0.99, iters=4, epsilon=-np.inf, **kw):
    """one guarded run of ops.vbx_batch -> (gamma, pi, elbo, n_iters) as numpy; nothing may be written outside the outputs"""
    R, Ntot, Smax = len(b["recs"]), int(b["rec_off"][-1]), b["Smax"]
    bg, g = banded((Ntot, Smax), SENT)
    bp, p = banded((R, Smax), SENT)
    be, e = banded((R, iters), SENT)
    bn, n = banded((R,), -7, torch.int32)
    g.copy_(up(b["gamma0"]))
    p.copy_(up(b["pi0"]))
    Xb, X = banded((Ntot, b["X"].shape[1]), SENT)
    X.copy_(up(b["X"]))
    ops.vbx_batch(X, up(b["Phi"]), b["rec_off"], b["n_states"], g, p, Fa, Fb, loopP, iters, epsilon, elbo=e, n_iters=n, **kw)
    torch.cuda.synchronize()
    for big, fill in ((bg, SENT), (bp, SENT), (be, SENT), (bn, -7), (Xb, SENT)):
        assert bands_intact(big, fill)
    assert bool((X == up(b["X"])).all())
    return g.cpu().numpy(), p.cpu().numpy(), e.cpu().numpy(), n.cpu().numpy()


def check_batch(b, out, what, iters):
    gamma, pi, elbo, nit = out
    worst = {"gamma": (0.0, 0.0, 0.0), "pi": (0.0, 0.0, 0.0), "elbo": (0.0, 0.0, 0.0)}
    assert nit.tolist() == [iters] * len(b["recs"])
    for r, c in enumerate(b["recs"]):
        lo, hi, S, y = int(b["rec_off"][r]), int(b["rec_off"][r + 1]), c["gamma0"].shape[1], c["y"]
        assert (gamma[lo:hi, S:] == 0).all() and (pi[r, S:] == 0).all(), (what, r)
        assert np.isfinite(gamma[lo:hi]).all() and np.isfinite(pi[r]).all() and np.isfinite(elbo[r]).all(), (what, r)
        if S == 1:
            assert (gamma[lo:hi, 0] == 1).all() and pi[r, 0] == 1
        err, rat = y.errors(gamma[lo:hi, :S], pi[r, :S], elbo[r]), y.ratios(gamma[lo:hi, :S], pi[r, :S], elbo[r])
        for k in worst:
            if rat[k] >= worst[k][2]:
                worst[k] = (err[k], y.bound[k], rat[k])
        if V.top_two_gap(y.gamma) >= 1e-3:
            assert V.labels_of(gamma[lo:hi, :S]).tolist() == V.labels_of(y.gamma).tolist(), (what, r)
    for k, (e, bd, ratio) in worst.items():
        print("vbx %s %s: error %.3e, bound %.3e, largest err / (e64 + floor) %.3f" % (what, k, e, bd, ratio))
    for r, c in enumerate(b["recs"]):
        lo, hi, S, y = int(b["rec_off"][r]), int(b["rec_off"][r + 1]), c["gamma0"].shape[1], c["y"]
        err = y.errors(gamma[lo:hi, :S], pi[r, :S], elbo[r])
        for k in err:
            assert err[k] <= y.bound[k], (what, r, k, err[k], y.bound[k])


@pytest.mark.parametrize("D", sorted(LAUNCHES))
def test_fixed_iterations_against_the_reference(ops, D):
    b = batch(D)
    check_batch(b, launch(ops, b), "D=%d" % D, 4)


def test_one_iteration(ops):
    b = batch(5, iters=1)
    out = launch(ops, b, iters=1)
    check_batch(b, out, "D=5 max_iters=1", 1)


@pytest.mark.parametrize("T,D,S,K", [c for c in V.CASES if c[0] >= 130])
@pytest.mark.parametrize("Fa,Fb,loopP", V.PARAMS)
def test_planted_speakers(diarize, T, D, S, K, Fa, Fb, loopP):
    c = V.planted_case(T, D, S, K, Fa, Fb, loopP)
    r = diarize.vbx(c["X"], c["Phi"], [0, T], gamma=c["gamma0"], pi=c["pi0"][None, :], Fa=Fa, Fb=Fb, loop_prob=loopP, max_iters=10,
                    epsilon=-np.inf, backend="hip")
    c["y"].check(r["gamma"], r["pi"][0], r["elbo"][0], "planted (%d,%d,%d,%d) Fa=%g" % (T, D, S, K, Fa))
    assert V.top_two_gap(c["y"].gamma) >= 1e-3
    assert r["labels"].tolist() == V.labels_of(c["y"].gamma).tolist()
    assert V.same_partition(r["labels"], c["truth"]) and len(set(r["labels"].tolist())) == K


# ---- degenerate inputs --------------------------------------------------------------------------------------------------------------
def test_zero_prior_and_one_hot_start(ops):
    T, D, S = 65, 5, 4
    X, Phi, _, first = V.planted(T, D, S, 3, seed=3)
    hot = (first[:, None] == np.arange(S)[None, :]).astype(np.float64)
    hot[:, 3] = 0
    hot[hot.sum(axis=1) == 0, 0] = 1                                       # state 3 is empty: N_s = 0, invL = 1, alpha = 0
    pi0 = np.array([0.5, 0.0, 0.25, 0.25])                                 # log 0: state 1 keeps gamma = 0
    rec = {"X": X, "gamma0": hot, "pi0": pi0, "y": V.Yardstick(X, Phi, hot, pi0, 0.3, 17.0, 0.99, 5, -np.inf)}
    b = pack([rec], Phi, Smax=6)
    out = launch(ops, b, iters=5)
    check_batch(b, out, "zero prior", 5)
    assert (out[0][:, 1] == 0).all() and out[1][0, 1] == 0


def test_underflow_gives_zeros_and_no_nan(ops):
    b = batch(512)
    gamma, pi, elbo, nit = launch(ops, b, Fa=1.0, Fb=1.0, loopP=0.9, iters=4)
    assert np.isfinite(gamma).all() and np.isfinite(pi).all() and np.isfinite(elbo).all() and nit.tolist() == [4] * len(b["recs"])
    assert (gamma == 0).any() and (gamma >= 0).all()
    for r, c in enumerate(b["recs"]):
        rows = gamma[b["rec_off"][r]:b["rec_off"][r + 1]]
        assert np.abs(rows.sum(axis=1) - 1).max() <= c["S"] * 2.0 ** -49 and abs(pi[r].sum() - 1) <= c["S"] * 2.0 ** -49


# ---- early stopping -----------------------------------------------------------------------------------------------------------------
def test_early_stopping(ops):
    E = V.EARLY
    b = pack(V.early_cases(), V.early_cases()[0]["Phi"])
    gamma, pi, elbo, nit = launch(ops, b, E["Fa"], E["Fb"], E["loopP"], E["max_iters"], E["epsilon"])
    want = [len(c["elbo"]) for c in b["recs"]]
    assert nit.tolist() == want and len(set(want)) > 1 and max(want) < E["max_iters"]
    for r, c in enumerate(b["recs"]):
        assert (elbo[r, want[r]:] == SENT).all()                          # the slots past n_iters keep what was there
        lo, hi, S = int(b["rec_off"][r]), int(b["rec_off"][r + 1]), c["gamma0"].shape[1]
        c["y"].check(gamma[lo:hi, :S], pi[r, :S], elbo[r, :want[r]], "early stop %d" % r)
    assert np.isfinite(gamma).all() and np.isfinite(pi).all()


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------
def test_runs_and_splits_give_the_same_bits(ops):
    b = batch(5)
    a = launch(ops, b)
    again = launch(ops, b)
    per_row, per_rec = 8 * (3 + 2 * b["Smax"]), 8 * b["Smax"] * 5
    split = launch(ops, b, ws_budget_bytes=70 * per_row + 2 * per_rec)      # two or three launches
    for x, y, z in zip(a, again, split):
        assert x.tobytes() == y.tobytes() == z.tobytes()
    # wherever a recording sits in the batch: the same recordings in reverse order
    rev = pack(b["recs"][::-1], b["Phi"], b["Smax"])
    g, p, e, n = launch(ops, rev)
    R = len(b["recs"])
    for r in range(R):
        lo, hi = int(b["rec_off"][r]), int(b["rec_off"][r + 1])
        l2, h2 = int(rev["rec_off"][R - 1 - r]), int(rev["rec_off"][R - r])
        assert a[0][lo:hi].tobytes() == g[l2:h2].tobytes() and a[1][r].tobytes() == p[R - 1 - r].tobytes()
        assert a[2][r].tobytes() == e[R - 1 - r].tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ops):
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    assert ops.vbx_max_states() == 64
    Ntot, D, R = 8, 4, 2
    ro = np.array([0, 3, 8], dtype=np.int64)
    X, Phi = up(np.ones((Ntot, D))), up(np.ones(D))
    rod = up(ro)
    outs = [torch.full((Ntot * 65,), SENT, device="cuda", dtype=torch.float64), torch.full((R * 65,), SENT, device="cuda", dtype=torch.float64),
            torch.full((R * 3,), SENT, device="cuda", dtype=torch.float64), torch.full((1 << 14,), SENT, device="cuda", dtype=torch.float64)]
    nit = torch.full((R,), -7, device="cuda", dtype=torch.int32)

    def call(Smax, n_states, ws_elems, loopP=0.99):
        ns = np.asarray(n_states, dtype=np.int32)
        rc = lib.spk_vbx_batch(X.data_ptr(), Phi.data_ptr(), ro.ctypes.data, rod.data_ptr(), ns.ctypes.data, up(ns).data_ptr(),
                               outs[0].data_ptr(), outs[1].data_ptr(), 0.3, 17.0, loopP, 3, 1e-6, outs[3].data_ptr(), ws_elems, outs[2].data_ptr(),
                               nit.data_ptr(), Ntot, D, R, Smax, hip.stream())
        torch.cuda.synchronize()
        return rc, lib.spk_last_error().decode()

    for args, word in [((65, (65, 1), 1 << 14), "Smax"), ((5, (6, 1), 1 << 14), "n_states"), ((5, (5, 0), 1 << 14), "n_states"),
                       ((5, (5, 1), 8 * 13 + 2 * 5 * 4 - 1), "workspace"), ((5, (5, 1), 1 << 14, 1.0), "loopP")]:
        rc, msg = call(*args)
        assert rc < 0 and msg.startswith("spk_vbx_batch") and word in msg, (args, msg)
    assert all(bool((t == SENT).all()) for t in outs) and bool((nit == -7).all())
    with pytest.raises(RuntimeError):
        ops.vbx_batch(X, Phi, ro, [1, 1], torch.zeros(Ntot, 65, device="cuda", dtype=torch.float64),
                      torch.zeros(R, 65, device="cuda", dtype=torch.float64))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_diarize_with_vbx_hip_against_host(diarize):
    from pytorch_kaldi_resnet_amd import plda
    rng = np.random.RandomState(8)
    D, L = 64, 10
    basis = rng.randn(L, D)
    base = rng.randn(D) * 0.5
    train, utt2spk = {}, {}
    for spk in range(40):
        centre = rng.randn(L) @ basis
        for u in range(8):
            k = "s%02d-u%d" % (spk, u)
            train[k] = (base + centre + 0.25 * rng.randn(D)).astype(np.float32)
            utt2spk[k] = "s%02d" % spk
    mean = np.mean(np.stack(list(train.values())).astype(np.float64), axis=0).astype(np.float32)
    transform, _ = plda.compute_lda(train, utt2spk, dim=L, mean=mean, backend="host")
    model = plda.compute_plda(train, utt2spk, transform, mean=mean, backend="host")
    emb, segments, planted = {}, [], []
    for r, n in enumerate([30, 45, 61]):
        centres = rng.randn(3, L) @ basis
        who = np.repeat(np.concatenate([np.arange(3), rng.randint(0, 3, size=n)]), 4)[:n]
        first = {}
        for w, c in enumerate(who):
            k = "rec%d-%08d-%08d" % (r, 20 * w, 20 * w + 40)
            emb[k] = (base + centres[c] + 0.25 * rng.randn(D)).astype(np.float32)
            segments.append((k, "rec%d" % r, 0.2 * w, 0.2 * w + 0.4))
            planted.append(first.setdefault(c, len(first) + 1))
    res = {}
    for backend in ("hip", "host"):                                        # the first pass is told six speakers: VBx prunes them
        res[backend] = diarize.diarize(emb, segments, "plda", reco2num_spk={"rec0": 6, "rec1": 6, "rec2": 6}, backend=backend, mean=mean,
                                       transform=transform, plda=model, vbx=dict(max_iters=20, epsilon=-np.inf))
    h, c = res["hip"], res["host"]
    assert h["ahc_labels"].tolist() == c["ahc_labels"].tolist() and len(set(h["ahc_labels"][:30].tolist())) == 6
    assert h["labels"].tolist() == c["labels"].tolist() and h["rttm"] == c["rttm"]
    assert h["labels"].tolist() == planted
    assert h["vbx_n_iters"].tolist() == c["vbx_n_iters"].tolist() == [20] * 3 and h["vbx_pi"].shape == c["vbx_pi"].shape == (3, 6)
    assert np.isfinite(h["vbx_elbo"]).all() and h["vbx_elbo"].shape == (3, 20)
    plain = diarize.diarize(emb, segments, "plda", reco2num_spk={"rec0": 6, "rec1": 6, "rec2": 6}, backend="hip", mean=mean,
                            transform=transform, plda=model)
    assert "ahc_labels" not in plain and plain["labels"].tolist() == h["ahc_labels"].tolist()
