"""Per-recording PCA of the dense PLDA scores on the device: the batched Jacobi eigensolver alone, steps 1-5
(spk_pca_plda_batch) with the per-recording row and score kernels under the tolerance rule of tests/pca_ref.py, the skips, the
clamps, the error path, bit-identity across runs, orders and splits, the host-side refusals, and diarize(..., target_energy=) on the
hip back end against the host one.  Run with -s to see err / (e64 + floor) per quantity and launch: section 6p's M comes from them."""
import numpy as np
import pytest

import diar_ref as DR
import pca_ref as P

pytestmark = pytest.mark.gpu
LD = np.longdouble
GUARD = 64


@pytest.fixture(scope="module")
def env():
    import torch
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import diarize, hip, ops, plda
    return {"torch": torch, "diarize": diarize, "hip": hip, "ops": ops, "plda": plda}


# ---- the eigensolver ------------------------------------------------------------------------------------------------------------------
def _cov_like(m, seed, rank=None):
    rng = np.random.RandomState(seed)
    x = rng.randn(3 * m if rank is None else rank, m) * 0.97 ** np.arange(m)
    return x.T @ x / len(x)


def _eig_batch():
    """(name, matrix) of one launch at ld = 256"""
    mats = [("psd%d" % m, _cov_like(m, m)) for m in (1, 2, 3, 15, 16, 17, 63, 64, 65, 150, 256)]
    rng = np.random.RandomState(3)
    q = np.linalg.qr(rng.randn(15, 15))[0]
    mats += [("zero", np.zeros((16, 16))), ("diag_ascending", np.diag(np.arange(1.0, 18.0))),
             ("rank1", np.outer(*[rng.randn(64)] * 2)),
             ("fourfold", q @ np.diag([5.0] + [2.0] * 4 + list(np.linspace(1.5, 0.1, 10))) @ q.T),
             ("big", _cov_like(65, 7) * 2.0 ** 200), ("small", _cov_like(63, 8) * 2.0 ** -200)]
    return [(n, (a + a.T) / 2) for n, a in mats]


def _run_syevj(env, mats, ld=256):
    """one launch through the C ABI with guard bands round every output -> (w, vec, sweeps, info) as numpy"""
    torch, hip = env["torch"], env["hip"]
    R = len(mats)
    A = np.zeros((R, ld, ld))
    for r, a in enumerate(mats):
        A[r, :len(a), :len(a)] = a
        A[r, len(a):, :] = np.nan                                  # nothing outside the order is read
        A[r, :, len(a):] = np.nan
    orders = np.array([len(a) for a in mats], dtype=np.int32)
    Ad, od = torch.from_numpy(A).cuda(), torch.from_numpy(orders).cuda()
    need = hip.lib().spk_syevj_ws_elems(R, ld)
    ws = torch.empty(need, device="cuda", dtype=torch.float64)
    w = torch.full((R * ld + 2 * GUARD,), -7.0, device="cuda", dtype=torch.float64)
    vec = torch.full((R * ld * ld + 2 * GUARD,), -7.0, device="cuda", dtype=torch.float64)
    sw = torch.full((R + 2 * GUARD,), -7, device="cuda", dtype=torch.int32)
    info = torch.full((R + 2 * GUARD,), -7, device="cuda", dtype=torch.int32)
    hip.call("spk_syevj_batch", Ad.data_ptr(), orders.ctypes.data, od.data_ptr(), ws.data_ptr(), need, w[GUARD:].data_ptr(),
             vec[GUARD:].data_ptr(), sw[GUARD:].data_ptr(), info[GUARD:].data_ptr(), R, ld, hip.stream())
    torch.cuda.synchronize()
    for t in (w, vec, sw, info):
        h = t.cpu().numpy()
        assert (h[:GUARD] == -7).all() and (h[-GUARD:] == -7).all()
    return (w[GUARD:-GUARD].cpu().numpy().reshape(R, ld), vec[GUARD:-GUARD].cpu().numpy().reshape(R, ld, ld),
            sw[GUARD:-GUARD].cpu().numpy(), info[GUARD:-GUARD].cpu().numpy())


@pytest.fixture(scope="module")
def eig_case(env):
    named = _eig_batch()
    mats = [a for _, a in named]
    return named, mats, _run_syevj(env, mats)


def test_syevj_eigenvalues_and_residuals(env, eig_case):
    named, mats, (w, vec, sweeps, info) = eig_case
    bound = env["ops"].syevj_max_sweeps()
    per_order = None
    worst = {"w": 0.0, "res": 0.0, "orth": 0.0}
    for r, (name, a) in enumerate(named):
        m = len(a)
        assert info[r] == 0 and 1 <= sweeps[r] < bound, (name, info[r], sweeps[r])
        got, V = w[r, :m], vec[r, :m, :m]
        assert (w[r, m:] == 0).all() and (vec[r, m:, :] == 0).all() and (vec[r, :, m:] == 0).all(), name
        assert (np.diff(got) <= 0).all(), name
        lw, lv = np.linalg.eigh(a)
        if m <= 150:
            hi = P.jacobi(a, LD)[0]
            e64 = float(np.abs(P.jacobi(a, np.float64)[0].astype(LD) - hi).max())
            if name == "psd150":
                per_order = e64 / float(np.abs(hi).max()) / 150
        else:
            # order 256: numpy.linalg.eigh is the reference, and e64 is the order-150 case's e64 per order and per unit of the
            # largest eigenvalue, times this order and this matrix's largest eigenvalue
            hi = lw[::-1].astype(LD)
            e64 = per_order * 256 * float(np.abs(hi).max())
        floor = 16 * P.ULP * float(np.abs(hi).max())
        err = float(np.abs(got.astype(LD) - hi).max())
        ratio = err / (e64 + floor) if e64 + floor > 0 else 0.0
        worst["w"] = max(worst["w"], ratio)
        assert err <= P.M * e64 + floor, (name, err, e64, floor)
        # residuals: numpy.linalg.eigh on the same matrix is the yardstick
        scale = float(np.abs(a).max())
        res = float(np.abs(a @ V.T - V.T * got[None, :]).max())
        orth = float(np.abs(V @ V.T - np.eye(m)).max())
        res0 = float(np.abs(a @ lv - lv * lw[None, :]).max())
        orth0 = float(np.abs(lv.T @ lv - np.eye(m)).max())
        rf, of = 16 * P.ULP * scale, 16 * P.ULP                    # 16 ulp of the largest magnitude: |A|max, and 1 for V^T V
        worst["res"] = max(worst["res"], res / (res0 + rf) if res0 + rf > 0 else 0.0)
        if orth / (orth0 + of) > worst["orth"]:
            worst["orth"], worst["orth_at"] = orth / (orth0 + of), name
        assert res <= max(P.M * res0, rf), (name, res, res0, rf)
        assert orth <= max(P.M * orth0, of), (name, orth, orth0, of)
    print("syevj: sweeps %s, largest err / (e64 + floor) of the eigenvalues %.3f, residual / (eigh + floor) %.3f, orthogonality %.3f (%s)"
          % (sweeps.tolist(), worst["w"], worst["res"], worst["orth"], worst.get("orth_at")))


def test_syevj_same_bits_again_and_reversed(env, eig_case):
    _, mats, first = eig_case
    again = _run_syevj(env, mats)
    rev = _run_syevj(env, mats[::-1])
    for a, b, c in zip(first, again, rev):
        assert a.tobytes() == b.tobytes() and a.tobytes() == c[::-1].tobytes()


def test_syevj_nan_reaches_the_sweep_bound_and_touches_nothing_else(env, eig_case):
    _, mats, first = eig_case
    bad = mats[4].copy()
    bad[2, 5] = bad[5, 2] = np.nan
    w, vec, sweeps, info = _run_syevj(env, mats[:6] + [bad] + mats[6:9])
    assert info[6] == 1 and sweeps[6] == env["ops"].syevj_max_sweeps() and np.isnan(w[6, :16]).any()
    keep = [0, 1, 2, 3, 4, 5, 7, 8, 9]
    for got, want in zip((w, vec, sweeps, info), first):
        assert got[keep].tobytes() == want[:9].tobytes()


def test_syevj_refusals(env):
    lib = env["hip"].lib()

    def go(orders=(3, 4), ld=4, R=2, ws=None):
        od = np.asarray(orders, dtype=np.int32)
        rc = lib.spk_syevj_batch(None, od.ctypes.data, None, None, 2 * R * (ld + (ld & 1)) ** 2 if ws is None else ws, None, None, None,
                                 None, R, ld, None)
        return rc, lib.spk_last_error().decode()

    rc, msg = go()
    assert rc < 0 and "spk_syevj_batch: null device pointer" in msg
    for kw, word in [(dict(ld=0), "ld="), (dict(ld=257), "ld="), (dict(orders=(0, 4)), "orders"), (dict(orders=(3, 5)), "orders"),
                     (dict(R=0), "R="), (dict(ws=63), "workspace")]:
        rc, msg = go(**kw)
        assert rc < 0 and msg.startswith("spk_syevj_batch") and word in msg, (kw, msg)
    assert lib.spk_syevj_max_dim() == 256 and lib.spk_syevj_ws_elems(2, 257) < 0 and lib.spk_syevj_ws_elems(3, 5) == 3 * 2 * 36


# ---- steps 1-5 and the per-recording kernels --------------------------------------------------------------------------------------------
NS = [1, 2, 3, 16, 17, 63, 64, 65, 257]
LS = [1, 3, 4, 5, 17, 64, 65, 150]
CLAMP_LS = (5, 17)                                                 # the launches that also run E = 0.999


def _launch(L):
    """the recordings of the launch at L: rows, rec_off and the model they share"""
    model = P.planted(8, L, 1, seed=50)[2]
    base = 2 if L == 17 else 1                                     # (seeds at which every recording meets the conditions of section 6p)
    zs = [P.planted(n, L, min(3, n), seed=base + i)[0] for i, n in enumerate(NS)]
    return zs, np.concatenate([[0], np.cumsum(NS)]).astype(np.int64), model


_YARD = {}


def _yard(L, r, E):
    if (L, r, E) not in _YARD:
        zs, _, model = _launch(L)
        y = P.Yardstick(zs[r], model, E)
        assert y.same_dim
        P.assert_conditions(y.hi, E, (L, NS[r], E))
        _YARD[(L, r, E)] = y
    return _YARD[(L, r, E)]


@pytest.mark.parametrize("L", LS)
def test_pca_launch_under_the_rule(env, L):
    diarize, torch = env["diarize"], env["torch"]
    zs, ro, model = _launch(L)
    Z = np.concatenate(zs)
    worst = {}
    for E in [0.1, 0.5, 0.9] + ([0.999] if L in CLAMP_LS else []):
        p = diarize.pca_rows(Z, ro, model, E, backend="hip")
        U = p["U"].cpu().numpy()
        scores, mat_off = env["ops"].score_dense(p["U"], ro, p["q"], p["g"], p["K"])
        scores, gK, gg, qq = scores.cpu().numpy(), p["K"].cpu().numpy(), p["g"].cpu().numpy(), p["q"].cpu().numpy()
        assert (p["info"] == 0).all()
        for r, n in enumerate(NS):
            y = _yard(L, r, E)
            d = int(p["dim"][r])
            assert d == y.dim, (L, n, E, d, y.dim)
            u = U[ro[r]:ro[r + 1]]
            assert (u[:, d:] == 0).all() and (p["psi_r"][r, d:] == 0).all() and (gg[r, d:] == 0).all()
            if y.skip:
                assert d == L and n == 1 or not y.hi["s"].sum() > 0
                assert (p["psi_r"][r] == model[2]).all()
            S64 = P.scores_fp64(u, p["psi_r"][r], d)
            for k, v in y.check(p["s"][r], p["psi_r"][r], S64, ("hip", L, n, E)).items():
                worst[k] = max(worst.get(k, 0.0), v)
            # the float matrix against the fp64 expression of its own operands: section 6n's derived bound, and symmetry
            S = scores[mat_off[r]:mat_off[r + 1]].reshape(n, n)
            assert (S == S.T).all()
            ref, bound, _ = DR.dense_ref(u, qq[ro[r]:ro[r + 1]], gg[r], gK[r])
            assert (np.abs(S.astype(LD) - ref) <= bound).all(), (L, n, E)
    print("pca L=%d: largest err / (e64 + floor): %s" % (L, {k: "%.3f" % v for k, v in sorted(worst.items())}))


def test_score_terms_kernel(env):
    """g, k and the weights take the operations of diarize.plda_dense_terms in its order: the same bits; K sums L terms of at most
    log(psi + 1) in another order with the device's log: L + 8 roundings of the sum of their magnitudes"""
    ops, torch, diarize = env["ops"], env["torch"], env["diarize"]
    rng = np.random.RandomState(11)
    for L in (1, 63, 64, 65, 150):
        psi = np.sort(rng.uniform(0.0, 8.0, (3, L)), axis=1)[:, ::-1].copy()
        psi[1, L // 2:] = 0.0                                       # the zero padding beyond dim
        psi[2] = 0.0
        g, k, qn, K = (t.cpu().numpy() for t in ops.pca_score_terms(torch.from_numpy(psi).cuda()))
        for r in range(3):
            wg, wk, wK = diarize.plda_dense_terms(psi[r])
            assert g[r].tobytes() == wg.tobytes() and k[r].tobytes() == wk.tobytes() and qn[r].tobytes() == (1.0 / (psi[r] + 1.0)).tobytes()
            mag = 0.5 * float((np.log(psi[r] + 1.0) + np.log(1.0 + psi[r] / (psi[r] + 1.0))).sum())
            assert abs(K[r] - wK) <= (L + 8) * 2.0 ** -53 * mag, (L, r, K[r], wK)
        assert K[2] == 0 and (g[2] == 0).all() and (qn[2] == 1).all()


def test_pca_clamps(env):
    """E = 0.999: short recordings stop at n - 1, long ones keep all L dimensions"""
    diarize = env["diarize"]
    for L in CLAMP_LS:
        zs, ro, model = _launch(L)
        p = diarize.pca_rows(np.concatenate(zs), ro, model, 0.999, backend="hip")
        assert p["dim"].tolist() == [_yard(L, r, 0.999).dim for r in range(len(NS))]
        assert p["dim"][NS.index(2)] == 1 and p["dim"][NS.index(3)] == 2 and p["dim"][NS.index(257)] == L


def test_pca_skips_equal_the_global_model(env):
    diarize, plda = env["diarize"], env["plda"]
    L = 17
    zs, _, model = _launch(L)
    same = np.repeat(zs[5][:1], 9, axis=0)                        # identical rows: tot = 0
    Z = np.concatenate([zs[0], same, zs[4]])
    ro = np.array([0, 1, 10, 10 + len(zs[4])])
    p = diarize.pca_rows(Z, ro, model, 0.5, backend="hip")
    assert p["dim"][0] == L and p["dim"][1] == L and p["dim"][2] < L
    glob = plda._side_host(Z[:10], model, np.ones(10, dtype=np.int64), True, False)
    U = p["U"].cpu().numpy()[:10]
    assert np.abs(U - glob).max() <= 64 * L * P.ULP * np.abs(glob).max()
    assert (p["psi_r"][:2] == model[2][None, :]).all()


def test_pca_non_positive_definite_w_is_reported(env):
    ops, torch, diarize = env["ops"], env["torch"], env["diarize"]
    L = 5
    zs, ro, model = _launch(L)
    Z = torch.from_numpy(np.concatenate(zs)).cuda()
    m, T, psi = model
    up = env["plda"]._up
    W = -np.eye(L)
    dim, s, psi_r, A_r, b_r, info = ops.pca_plda_batch(Z, ro, up(W), up(np.eye(L)), up(T), up(psi), up(m), 0.5)
    info, dim = info.cpu().numpy(), dim.cpu().numpy()
    skipped = np.array([n == 1 for n in NS])
    assert (info[~skipped] == 2).all() and (info[skipped] == 0).all()
    for t in (s, psi_r, A_r, b_r):
        assert torch.isfinite(t).all()
    assert (A_r[torch.from_numpy(~skipped).cuda()] == 0).all() and (psi_r[torch.from_numpy(~skipped).cuda()] == 0).all()
    # a NaN row: the first eigendecomposition of that recording reaches its sweep bound, and pca_rows names the recording
    Zn = np.concatenate(zs)
    Zn[ro[3] + 2, 1] = np.nan
    with pytest.raises(ValueError, match="recording 3 "):
        diarize.pca_rows(Zn, ro, model, 0.5, backend="hip")


def test_pca_invariants_at_the_largest_dimension(env):
    """L = 256 with n = 64 on the invariants alone: A_r W A_r^T = I and A_r B A_r^T = diag(psi_r)"""
    ops, torch = env["ops"], env["torch"]
    L, n = 256, 64
    z, _, model = P.planted(n, L, 4, seed=9)
    m, T, psi = model
    Ti = np.linalg.inv(T)
    W, B = Ti @ Ti.T, (Ti * psi[None, :]) @ Ti.T
    up = env["plda"]._up
    dim, s, psi_r, A_r, b_r, info = ops.pca_plda_batch(torch.from_numpy(z).cuda(), np.array([0, n]), up(W), up(B), up(T), up(psi), up(m),
                                                       0.9)
    d = int(dim[0])
    assert int(info[0]) == 0 and 2 <= d <= n - 1
    A, p = A_r[0].cpu().numpy()[:d], psi_r[0].cpu().numpy()[:d]
    assert (A_r[0].cpu().numpy()[d:] == 0).all() and (np.diff(p) <= 0).all() and (p >= 0).all()
    cond = np.linalg.cond(W)
    tol = 64 * L * P.ULP * cond
    e1 = float(np.abs(A @ W @ A.T - np.eye(d)).max())
    e2 = float(np.abs(A @ B @ A.T - np.diag(p)).max()) / float(p.max())
    print("pca L=256: dim %d, |A W A^T - I| %.2e, |A B A^T - diag| / psi_1 %.2e, tolerance %.2e (cond W %.1e)" % (d, e1, e2, tol, cond))
    assert e1 <= tol and e2 <= tol
    assert np.abs(b_r[0].cpu().numpy()[:d] + A @ m).max() <= 64 * L * P.ULP * np.abs(A).max() * np.abs(m).max()


def test_pca_split_and_reversed_batches_give_the_same_bits(env):
    ops, torch = env["ops"], env["torch"]
    L = 65
    zs, ro, model = _launch(L)
    m, T, psi = model
    Ti = np.linalg.inv(T)
    up = env["plda"]._up
    args = (up(Ti @ Ti.T), up((Ti * psi[None, :]) @ Ti.T), up(T), up(psi), up(m), 0.5)
    Z = torch.from_numpy(np.concatenate(zs)).cuda()
    whole = [t.cpu().numpy() for t in ops.pca_plda_batch(Z, ro, *args)]
    per = 8 * (ops.pca_plda_ws_elems(np.array([0, 1]), L) - 1)
    split = [t.cpu().numpy() for t in ops.pca_plda_batch(Z, ro, *args, ws_budget_bytes=2 * per)]
    Zr = torch.from_numpy(np.concatenate(zs[::-1])).cuda()
    ror = np.concatenate([[0], np.cumsum(NS[::-1])])
    rev = [t.cpu().numpy() for t in ops.pca_plda_batch(Zr, ror, *args)]
    for a, b, c in zip(whole, split, rev):
        assert a.tobytes() == b.tobytes() and a.tobytes() == c[::-1].tobytes()


def test_pca_refusals_and_the_dimension_cap(env):
    diarize, ops, torch = env["diarize"], env["ops"], env["torch"]
    z, _, model = P.planted(8, 4, 2)
    with pytest.raises(RuntimeError, match="rec_off"):
        ops.pca_plda_ws_elems(np.array([0, 3, 3]), 4)
    with pytest.raises(RuntimeError, match="L="):
        ops.pca_plda_ws_elems(np.array([0, 3]), 257)
    big = (np.zeros(257), np.eye(257), np.ones(257))
    with pytest.raises(ValueError, match="256"):
        diarize.pca_rows(np.zeros((4, 257), dtype=np.float32), [0, 4], big, 0.5, backend="hip")
    for E in (0.0, 1.0, np.nan):
        with pytest.raises(ValueError):
            diarize.pca_rows(z, [0, 8], model, E, backend="hip")


# ---- diarize() ------------------------------------------------------------------------------------------------------------------------
def _diar_case(n, L, K, seed):
    z, lab, model = P.planted(n, L, K, seed=seed)
    keys = ["rec-%04d" % i for i in range(n)]
    segments = [(k, "rec", 0.25 * i, 0.25 * i + 0.5) for i, k in enumerate(keys)]
    args = dict(mean=np.zeros(L), transform=np.eye(L), plda=model)
    return {k: z[i].astype(np.float64) for i, k in enumerate(keys)}, segments, args


@pytest.mark.parametrize("n,L,K", [(130, 128, 4), (65, 40, 4), (33, 17, 3)])
def test_diarize_hip_equals_host(env, n, L, K):
    diarize = env["diarize"]
    emb, segments, args = _diar_case(n, L, K, 21)
    full = diarize.diarize(emb, segments, "plda", reco2num_spk={"rec": 1}, backend="host", target_energy=0.5, **args)
    cost = full["merge_cost"][:n - 1]
    order = np.sort(cost)
    k = int(np.argmax(np.diff(order)))
    thr = -0.5 * (order[k] + order[k + 1])
    assert np.abs(cost + thr).min() >= 1e-3, np.abs(cost + thr).min()
    host = diarize.diarize(emb, segments, "plda", threshold=thr, backend="host", target_energy=0.5, **args)
    dev = diarize.diarize(emb, segments, "plda", threshold=thr, backend="hip", target_energy=0.5, **args)
    assert host["pca_dim"] == dev["pca_dim"] and len(dev["pca_dim"]) == 1
    assert host["labels"].tolist() == dev["labels"].tolist() and host["rttm"] == dev["rttm"]
    assert 1 < len(set(dev["labels"].tolist())) < n
    vb = dict(max_iters=5, epsilon=-np.inf)
    both = diarize.diarize(emb, segments, "plda", threshold=thr, backend="hip", target_energy=0.5, vbx=vb, **args)
    assert both["ahc_labels"].tolist() == dev["labels"].tolist() and both["pca_dim"] == dev["pca_dim"]
    keys = [s[0] for s in segments]
    X, Phi = diarize.vbx_inputs(np.stack([emb[k] for k in keys]), backend="hip", **args)
    want = diarize.vbx(X, Phi, [0, n], init_labels=dev["labels"], backend="hip", **vb)
    assert both["labels"].tolist() == want["labels"].tolist()
    assert both["vbx_elbo"].tobytes() == want["elbo"].tobytes() and both["vbx_pi"].tobytes() == want["pi"].tobytes()
