"""csrc/se.hip, csrc/plda.hip, csrc/eval.hip and csrc/cm.hip on a real MI355X at the edges their feature tests never reach: the
cases of tests/late_edges_ref.py (whose premises tests/test_late_edges_cpu.py proves) through `ops` / `features` against the fp64
references and derived per-element bounds of se_ref.py, plda_ref.py, backend_ref.py and cm_ref.py.  Every floating-point
comparison is error / bound <= 1 under the bound the reference module derives from the operation count; everything else is bit or
byte equality.  Run with -s to see the largest error / bound of every group and the time of the module.

The one large case is SE_BIG = (256, 19, 27, 64), 8.4 M floats per tensor: the smallest map of 64 channels at batch 256 at which
the grid cap of the two apply kernels binds (B x nq must exceed 8192 x 256 groups), so that a thread takes a second trip of the
`i += stride` loop; the same batch takes 32 passes of the finalize kernel's utterance loop.  Its inputs and forward tensors are
built once per module."""
import time

import numpy as np
import pytest
import torch

import backend_ref as BR
import cm_ref
import late_edges_ref as E
import plda_ref as PR
import se_ref as R
import test_backend_gpu as BK
import test_cm_gpu as CM
import test_plda_gpu as PL
from helpers import decode_pairs, sigma_of, slot, slot_value

pytestmark = pytest.mark.gpu

MASK_ACT, MASK_BITS = 1, 3
dev = PL.dev


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def report():
    t0 = time.time()
    yield
    print("\nlargest error / bound per group:", {k: round(v, 3) for k, v in sorted(E.RATIOS.items())})
    print("tests/test_late_edges_gpu.py: %.1f s" % (time.time() - t0))


def twice(fn):
    """run a launch twice: the results must be bit-identical -> the first result"""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if x is not None:                                    # bit patterns: a NaN left in a prefilled output equals itself
            ints = {4: torch.int32, 8: torch.int64}[x.element_size()]
            assert torch.equal(x.view(ints), y.view(ints)), "two runs differ"
    return a


def ilen(wl):
    return torch.tensor(wl, dtype=torch.int32, device="cuda") if wl is not None else None


# ==== A. se.hip =================================================================================================================
_STATE = {}


def se_state(ops, B, H, Wd, C, Cr=None):
    """one SE block tail on the device, built once per shape: the host tensors of E.se_block, and what the forward kernels wrote
    from them (sums, q, u, g, the block output and its sign bits)"""
    key = (B, H, Wd, C, Cr)
    if key not in _STATE:
        d = E.se_block(B, H, Wd, C, Cr)
        g = {k: v.cuda() for k, v in d.items()}
        g["sums"] = ops.se_squeeze(g["raw"])
        g["q"], g["u"], g["g"] = ops.se_excite(g["sums"], (g["scale"], g["shift"]), g["w1"], g["w2"], H, Wd)
        g["out"], g["bits"] = ops.se_apply(g["raw"], (g["scale"], g["shift"]), g["g"], res=g["res"], relu=True, mask=True)
        g["bn4"] = torch.stack([g["mean"], g["inv"], g["scale"], g["shift"]])
        d["mask"] = (g["out"] > 0).cpu()
        _STATE[key] = (d, g)
    return _STATE[key]


def check_squeeze(ops, group, x, wl):
    got = twice(lambda: ops.se_squeeze(x.cuda(), ilen(wl)))
    E.note(group, R.check("sums", got, *R.squeeze_ref(x, wl)))
    xi = E.small_ints(2, *x.shape)                                           # small integers: every float32 partial sum is exact
    assert torch.equal(ops.se_squeeze(xi.cuda(), ilen(wl)).cpu(), R.squeeze_ref(xi, wl)[0])


def check_excite(ops, group, sums, d, H, Wd, affine, wl):
    """sums: the fp64 table handed to the kernel (a device tensor) -> the kernel's (q, u, g)"""
    aff = (d["scale"].cuda(), d["shift"].cuda()) if affine else None
    q, u, g = twice(lambda: ops.se_excite(sums, aff, d["w1"].cuda(), d["w2"].cuda(), H, Wd, ilen(wl)))
    ref = R.excite_ref(sums.cpu(), d["scale"] if affine else None, d["shift"] if affine else None, d["w1"], d["w2"], H, Wd, wl)
    for name, got in (("q", q), ("u", u), ("g", g)):
        E.note(group + " " + name, R.check(name, got, *ref[name]))
    assert float(g.min()) >= 0 and float(g.max()) <= 1
    return q, u, g


def check_apply(ops, group, d, g, form, wl):
    """the checks of tests/test_se_gpu.py::test_apply on host tensors d and a gate table g"""
    raw, B, Wd = d["raw"], d["raw"].shape[0], d["raw"].shape[2]
    C = raw.shape[-1]
    res = d["res"] if form != "plain" else None
    rs, rh = (E.rnd(19, C, scale=0.5, shift=1.0), E.rnd(20, C, scale=0.3)) if form == "affine_res_masked" else (None, None)
    am = slot()
    rawd, resd = raw.cuda(), res.cuda() if res is not None else None
    aff, raff = (d["scale"].cuda(), d["shift"].cuda()), (rs.cuda(), rh.cuda()) if rs is not None else None
    nan = lambda: torch.full_like(rawd, float("nan"))      # noqa: E731  (a group the kernel skips stays NaN: R.check refuses it)
    out, bits = twice(lambda: ops.se_apply(rawd, aff, g.cuda(), res=resd, res_affine=raff, relu=True, mask=True, amax_out=am,
                                           wlen=ilen(wl), out=nan()))
    ref, bound = R.apply_ref(raw, d["scale"], d["shift"], g, res, rs, rh, True, wl)
    E.note(group, R.check("out", out, ref, bound))
    oc = out.cpu()
    if wl is not None:
        for b in range(B):
            assert bool((oc[b, :, wl[b]:] == 0).all()), b                     # zero past wlen[b]
    assert slot_value(am) == float(oc.abs().max())                           # the amax slot: the largest stored value
    assert np.array_equal(E.unpack_bits(bits, tuple(raw.shape)), (oc > 0).numpy())      # the mask words: out > 0 everywhere
    lin = ops.se_apply(rawd, aff, g.cuda(), res=resd, res_affine=raff, relu=False, wlen=ilen(wl), out=nan())
    E.note(group, R.check("out (no relu)", lin, *R.apply_ref(raw, d["scale"], d["shift"], g, res, rs, rh, False, wl)))
    return out, bits


def check_bwd_reduce(ops, group, dout, raw, act, bits, mask):
    """dout, raw, act (its sign is the mask), bits: device tensors; mask: the host bool tensor both stand for"""
    C = raw.shape[-1]
    ca = torch.zeros(C, dtype=torch.int32, device="cuda")
    S = twice(lambda: ops.se_bwd_reduce(dout, raw, bits, MASK_BITS, chan_amax=ca))
    assert torch.equal(S, ops.se_bwd_reduce(dout, raw, act, MASK_ACT))        # the two mask sources select the same values
    ref = R.bwd_reduce_ref(dout.cpu(), mask, raw.cpu())
    E.note(group + " S1", R.check("S1", S[:, 0], *ref["S1"]))
    E.note(group + " S2", R.check("S2", S[:, 1], *ref["S2"]))
    e = dout.cpu() * mask
    assert torch.equal(ca.cpu().view(torch.float32), e.abs().amax((0, 1, 2)))
    assert bool((ops.se_bwd_reduce(torch.zeros_like(dout), raw, bits, MASK_BITS) == 0).all())
    return S


def check_gate(ops, group, d, g, S, HW, accumulate, pair=None):
    """spk_se_bwd_gate on the tables S (fp64, device), g["sums" / "q" / "u" / "g"] against se_ref.gate_ref of the same tables
    -> (coef, dq)"""
    C, Cr = d["w1"].shape[1], d["w1"].shape[0]
    prior = [E.rnd(40 + i, *s, scale=5.0) for i, s in enumerate([(Cr, C), (C, Cr), (C,), (C,)])]

    def run():
        bufs = [p.clone().cuda() for p in prior]
        r = ops.se_bwd_gate(S, g["sums"], g["q"], g["u"], g["g"], g["w1"], g["w2"], g["bn4"], g["gamma"], bufs[0], bufs[1], bufs[2],
                            bufs[3], HW, accumulate=accumulate, pair=pair)
        return r + tuple(bufs)

    coef, dq, da, du, dw1, dw2, dga, dbe = twice(run)
    ref = R.gate_ref(S[:, 0].cpu(), S[:, 1].cpu(), g["sums"].cpu(), g["q"].cpu(), g["u"].cpu(), g["g"].cpu(), d["w1"], d["w2"],
                     d["mean"], d["inv"], d["scale"], d["shift"], d["gamma"], HW, prior=prior if accumulate else None)
    got = {"da": da, "du": du, "dq": dq[0], "dqs": dq[1], "dW1": dw1, "dW2": dw2, "dgamma": dga, "dbeta": dbe, "k1": coef[0],
           "m1": coef[1], "m2": coef[2]}
    for k, v in got.items():
        E.note(group + " " + k, R.check(k, v, *ref[k]))
    return coef, dq


def check_gate_is_a_batchnorm_backward(d, g, coef, dq):
    """the tables reproduce a plain BatchNorm-backward reduction over dz = g e + dq / HW (tests/test_se_gpu.py::test_bwd_gate)"""
    B, H, Wd, _ = d["raw"].shape
    n = B * H * Wd
    if n == 1:
        return
    dz = g["g"].double()[:, None, None, :].cpu() * (d["dout"].double() * d["mask"]) + dq[1].double().cpu()[:, None, None, :]
    xh = (d["raw"].double() - d["mean"].double()) * d["inv"].double()
    assert torch.allclose(coef[1].double().cpu(), dz.sum((0, 1, 2)) / n, rtol=0, atol=1e-5 * float(dz.abs().sum((0, 1, 2)).max()) / n)
    assert torch.allclose(coef[2].double().cpu(), (dz * xh).sum((0, 1, 2)) / n, rtol=0,
                          atol=1e-5 * float((dz * xh).abs().sum((0, 1, 2)).max()) / n)


def loud_tables(ops, d, g, HW, loud):
    """the backward tables with utterance `loud`'s S - and so its dg, da, du and dq - 10^6 times the others', and the operand-scale
    slots (tests/test_se_gpu.py::test_bwd_apply) -> (S, u with every hidden unit live, A, Rr)"""
    S = ops.se_bwd_reduce(g["dout"], g["raw"], g["bits"], MASK_BITS)
    if loud is not None:
        S[loud] *= 1e6
    A, Rr = slot(), slot()
    ops.absmax_into(g["dout"], A)
    ops.absmax_into(g["raw"], Rr)
    return S, g["u"].abs() + 0.1, A, Rr


def check_bound_slot(d, coef, dq, A, Rr, est, loud):
    """the bound slot: se_ref.draw_bound_ref evaluated from the kernel's own tables, within the kernel's rounding slack"""
    B = dq.shape[1]
    if loud is not None:
        rest = torch.cat([dq[1, :loud], dq[1, loud + 1:]])
        assert float(dq[1, loud].abs().max()) > 1e4 * float(rest.abs().max())
    formula = R.draw_bound_ref(coef.cpu(), dq[1].cpu(), d["mean"], d["inv"], slot_value(A), slot_value(Rr))
    assert formula <= slot_value(est) <= formula * (1 + 2.0 ** -14), (formula, slot_value(est), B)


def check_bwd_apply(ops, group, d, g, HW, pairs, loud):
    """the checks of tests/test_se_gpu.py::test_bwd_apply: e_out in place on dout, fp32 or f16-pair draw under the bound slot"""
    C, Cr = d["w1"].shape[1], d["w1"].shape[0]
    S, u, A, Rr = loud_tables(ops, d, g, HW, loud)
    est = slot()
    bufs = [torch.zeros(s, device="cuda") for s in [(Cr, C), (C, Cr), (C,), (C,)]]
    coef, dq, _, _ = ops.se_bwd_gate(S, g["sums"], g["q"], u, g["g"], g["w1"], g["w2"], g["bn4"], g["gamma"], *bufs, HW,
                                     pair=(A, Rr, est))
    check_bound_slot(d, coef, dq, A, Rr, est, loud)
    am = slot()

    def run():
        e = g["dout"].clone()
        draw = ops.se_bwd_apply(e, g["raw"], g["bits"], MASK_BITS, g["g"], dq[1], g["bn4"], coef, e_out=e, amax_out=am,
                                pair_scale=est if pairs else None, draw_out=torch.full_like(e, float("nan")))
        return draw, e

    draw, e = twice(run)
    ref, bound, e_ref = R.bwd_apply_ref(d["dout"], d["mask"], d["raw"], g["g"].cpu(), dq[1].cpu(), d["mean"], d["inv"], coef.cpu())
    assert torch.equal(e.cpu().double(), e_ref)                              # the shortcut gradient, in place
    true_amax = float(ref.abs().max())
    assert slot_value(est) >= true_amax
    if pairs:
        sig = sigma_of(est)
        got = decode_pairs(draw.cpu(), sig)
        bound = bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25 / sig
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        ops.f16_window_count(draw, est, counts, pairs=True)
        assert int(counts[0]) == draw.numel() and int(counts[1]) == 0, counts
    else:
        got = draw
    E.note(group, R.check("draw", got, ref, bound))
    assert abs(slot_value(am) - true_amax) <= float(bound.max())
    draw_act = ops.se_bwd_apply(g["dout"], g["raw"], g["out"], MASK_ACT, g["g"], dq[1], g["bn4"], coef,
                                pair_scale=est if pairs else None)
    assert torch.equal(draw_act, draw)                                       # the activated tensor as the mask source


# ---- A.1 wide channels: C = 512 and 1024, the `c += 256` loops run 2 and 4 times, rstep is 2 and 1 ----
@pytest.mark.parametrize("B,H,Wd,C", E.SE_WIDE)
def test_wide_forward(ops, B, H, Wd, C):
    d, g = se_state(ops, B, H, Wd, C)
    for wl in (None, E.widths(B, Wd)):
        check_squeeze(ops, "A1 squeeze", d["raw"], wl)
    check_excite(ops, "A1 excite", g["sums"], d, H, Wd, True, None)
    check_excite(ops, "A1 excite", g["sums"], d, H, Wd, False, E.widths(B, Wd))
    gate = g["g"].cpu().clone()                                            # the table the excite kernel wrote, with both ends
    gate[0, 0], gate[0, 1] = 0.0, 1.0
    for form, wl in (("plain", None), ("identity_res", None), ("affine_res_masked", E.widths(B, Wd))):
        check_apply(ops, "A1 apply", d, gate, form, wl)


@pytest.mark.parametrize("B,H,Wd,C", E.SE_WIDE)
def test_wide_backward(ops, B, H, Wd, C):
    d, g = se_state(ops, B, H, Wd, C)
    assert 0 < float(d["mask"].double().mean()) < 1
    S = check_bwd_reduce(ops, "A1 bwd_reduce", g["dout"], g["raw"], g["out"], g["bits"], d["mask"])
    for accumulate in (False, True):
        coef, dq = check_gate(ops, "A1 gate", d, g, S, H * Wd, accumulate)
        check_gate_is_a_batchnorm_backward(d, g, coef, dq)
    for pairs in (False, True):
        check_bwd_apply(ops, "A1 bwd_apply", d, g, H * Wd, pairs, 1 if B > 1 else None)


# ---- A.2 hidden widths off the model: Cr = 1, 3 (a wave idles in the `j += 4` loops), Cr = 64 > C, Cr = 64 at C = 1024 ----
@pytest.mark.parametrize("C,Cr", E.SE_HIDDEN)
def test_hidden_widths(ops, C, Cr):
    B, H, Wd = E.SE_HIDDEN_MAP
    d = E.se_block(B, H, Wd, C, Cr)
    g = {k: d[k].cuda() for k in ("w1", "w2", "gamma")}
    g["sums"] = d["raw"].double().sum((1, 2)).cuda()
    g["bn4"] = torch.stack([d["mean"], d["inv"], d["scale"], d["shift"]]).cuda()
    check_excite(ops, "A2 excite", g["sums"], d, H, Wd, False, E.widths(B, Wd))
    g["q"], g["u"], g["g"] = check_excite(ops, "A2 excite", g["sums"], d, H, Wd, True, None)
    assert tuple(g["u"].shape) == (B, Cr)
    S = E.rnd(11, B, 2, C, scale=3.0).double().cuda()
    for accumulate in (False, True):
        check_gate(ops, "A2 gate", d, g, S, H * Wd, accumulate)


# ---- A.3 SE_ROWS edges: HW = 511, 512, 513, 1025 -> 1, 1, 2, 3 reduction blocks per utterance ----
@pytest.mark.parametrize("H,Wd", E.SE_ROW_MAPS)
def test_row_edges(ops, H, Wd):
    B, C = E.SE_ROW_B, E.SE_ROW_C
    raw = E.rnd(1, B, H, Wd, C, scale=1.5, shift=0.3)
    for wl in (None, E.widths(B, Wd)):
        check_squeeze(ops, "A3 squeeze", raw, wl)
    act, dout = E.rnd(2, B, H, Wd, C), E.rnd(3, B, H, Wd, C, scale=2.0)
    mask = act > 0
    assert 0.4 < float(mask.double().mean()) < 0.6
    check_bwd_reduce(ops, "A3 bwd_reduce", dout.cuda(), raw.cuda(), act.cuda(), E.pack_bits(mask).cuda(), mask)


# ---- A.4 the capped grid and many utterances ----
@pytest.fixture(scope="module")
def big(ops):
    return se_state(ops, *E.SE_BIG)


def test_big_apply_takes_a_second_trip(ops, big):
    """threads 0 .. 15 of block 0 of every utterance take a second trip of `i += stride`: the last pixel's values, zeros past
    wlen[b] and mask words come from it"""
    d, g = big
    B, H, Wd, C = E.SE_BIG
    gate = g["g"].cpu().clone()
    gate[0, 0], gate[0, 1] = 0.0, 1.0
    check_apply(ops, "A4 apply", d, gate, "affine_res_masked", E.widths(B, Wd))


def test_big_bwd_reduce(ops, big):
    d, g = big
    check_bwd_reduce(ops, "A4 bwd_reduce", g["dout"], g["raw"], g["out"], g["bits"], d["mask"])


@pytest.mark.parametrize("accumulate", [False, True])
def test_big_bwd_gate(ops, big, accumulate):
    """32 passes of `b += 8`; utterance 200's dq is 10^6 times the others', so the `mq` maximum behind the bound slot comes from
    pass 25"""
    d, g = big
    B, H, Wd, C = E.SE_BIG
    S, u, A, Rr = loud_tables(ops, d, g, H * Wd, E.SE_BIG_LOUD)
    est = slot()
    coef, dq = check_gate(ops, "A4 gate", d, dict(g, u=u), S, H * Wd, accumulate, pair=(A, Rr, est))
    check_bound_slot(d, coef, dq, A, Rr, est, E.SE_BIG_LOUD)
    if not accumulate:
        S = ops.se_bwd_reduce(g["dout"], g["raw"], g["bits"], MASK_BITS)
        coef, dq = check_gate(ops, "A4 gate", d, g, S, H * Wd, False)
        check_gate_is_a_batchnorm_backward(d, g, coef, dq)


@pytest.mark.parametrize("pairs", [False, True])
def test_big_bwd_apply(ops, big, pairs):
    d, g = big
    B, H, Wd, C = E.SE_BIG
    check_bwd_apply(ops, "A4 bwd_apply", d, g, H * Wd, pairs, E.SE_BIG_LOUD)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("H,Wd,C", E.SE_PASS_MAPS)
@pytest.mark.parametrize("B", E.SE_PASS_B)
def test_finalize_pass_count(ops, B, H, Wd, C, accumulate):
    d, g = se_state(ops, B, H, Wd, C)
    S = ops.se_bwd_reduce(g["dout"], g["raw"], g["bits"], MASK_BITS)
    coef, dq = check_gate(ops, "A4 passes", d, g, S, H * Wd, accumulate)
    check_gate_is_a_batchnorm_backward(d, g, coef, dq)


# ==== B. plda.hip ===============================================================================================================
@pytest.mark.parametrize("Do,Di", E.AFFINE_DIMS)
def test_affine_every_instance(ops, Do, Di):
    """the variants of tests/test_plda_gpu.py::test_affine_lennorm at output widths that take NT = 1, 2, 4 and 8"""
    rng = np.random.RandomState(Do * 1000 + Di)
    A = rng.randn(Do, Di) / np.sqrt(Di)
    A[Do // 2, Di // 3] += 2.0                                               # nothing symmetric about it
    b = rng.randn(Do)
    worst64, worst32 = 0.0, 0.0
    for N in E.AFFINE_N:
        for variant in range(4):
            f64_in, use_q = variant & 1, variant >> 1
            x = (rng.randn(N, Di) * 3).astype(np.float64 if f64_in else np.float32)
            q = np.abs(rng.randn(Do)) + 0.1 if use_q else None
            xd = PL.pitched(x, variant)
            for scale in (False, True):
                ref, bound = PR.affine(x, A, b, q, scale)
                y64 = ops.affine_lennorm(xd, dev(A), dev(b), None if q is None else dev(q), scale, torch.float64).cpu().numpy()
                worst64 = max(worst64, PL.ratio(y64, ref, bound))
                y32 = ops.affine_lennorm(xd, dev(A), dev(b), None if q is None else dev(q), scale, torch.float32).cpu().numpy()
                assert y32.dtype == np.float32
                r32 = ref.astype(np.float32)
                ulp = np.spacing(np.abs(r32)).astype(np.float64)
                worst32 = max(worst32, float((np.abs(y32.astype(np.float64) - r32.astype(np.float64)) / ulp).max()))
                if scale:                                                    # the weighted length really is sqrt(Do)
                    ss = (y64 * y64 * (1.0 if q is None else q)).sum(axis=1)
                    assert np.abs(ss / Do - 1).max() < 1e-12
    print("affine (%d, %d) NT=%d: fp64 largest error / bound = %.3f; fp32 largest error = %.2f ulp" % (
        Do, Di, E.affine_nt(Do), worst64, worst32))
    E.note("B1 affine fp64", worst64)
    E.note("B1 affine fp32 ulp", worst32)
    assert worst64 <= 1.0 and worst32 <= 1.0


@pytest.mark.parametrize("D", E.AFFINE_IDENTITY_D)
def test_affine_identity(ops, D):
    """A = NULL: ivector-normalize-length of float32 rows (D = 512: the embeddings themselves), and a plain copy without the scale"""
    rng = np.random.RandomState(D)
    v = (rng.randn(65, D) * 2).astype(np.float32)
    v[7] = 0
    z = ops.affine_lennorm(dev(v), None, None, None, True, torch.float32).cpu().numpy()
    ref, _ = PR.affine(v, None, None, None, True)
    r32 = ref.astype(np.float32)
    assert (np.abs(z.astype(np.float64) - r32) <= np.spacing(np.abs(r32))).all() and not z[7].any()
    z64 = ops.affine_lennorm(dev(v), None, None, None, True, torch.float64).cpu().numpy()
    E.note("B1 identity fp64", PL.ratio(z64, *PR.affine(v, None, None, None, True)))
    assert PL.ratio(z64, *PR.affine(v, None, None, None, True)) <= 1.0
    rows = np.arange(65) != 7
    assert np.abs(np.sqrt((z64[rows] ** 2).sum(axis=1)) / np.sqrt(D) - 1).max() < 1e-12      # the scaled length is sqrt(D)
    assert np.array_equal(ops.affine_lennorm(dev(v), None, None, None, False, torch.float64).cpu().numpy(), v.astype(np.float64))
    assert np.array_equal(ops.affine_lennorm(dev(v), None, None, None, False, torch.float32).cpu().numpy(), v)


@pytest.mark.parametrize("Do,Di", E.AFFINE_EXACT)
def test_affine_places_every_element(ops, Do, Di):
    """exact integer data with an asymmetric A and a bias: every output element lands in its place"""
    Ai = (np.arange(Do * Di).reshape(Do, Di) % 17 - 8).astype(np.float64)
    xi = (np.arange(70 * Di).reshape(70, Di) % 13 - 6).astype(np.float64)
    assert not np.array_equal(Ai[:Di, :Di], Ai[:Di, :Di].T)
    got = ops.affine_lennorm(dev(xi), dev(Ai), dev(np.arange(float(Do))), None, False, torch.float64).cpu().numpy()
    assert np.array_equal(got, xi @ Ai.T + np.arange(float(Do)))
    got = ops.affine_lennorm(dev(xi.astype(np.float32)), dev(Ai), dev(np.arange(float(Do))), None, False, torch.float32).cpu().numpy()
    assert np.array_equal(got, (xi @ Ai.T + np.arange(float(Do))).astype(np.float32))


def test_affine_writes_a_row_range_only(ops):
    Do, Di = E.AFFINE_RANGE_DO, 17
    Ai = (np.arange(Do * Di).reshape(Do, Di) % 17 - 8).astype(np.float64)
    xi = (np.arange(70 * Di).reshape(70, Di) % 13 - 6).astype(np.float64)
    table = torch.full((100, Do), 7.0, device="cuda", dtype=torch.float64)
    ops.affine_lennorm(dev(xi), dev(Ai), None, None, False, torch.float64, out=table[10:80])
    t = table.cpu().numpy()
    assert np.array_equal(t[10:80], xi @ Ai.T) and (t[:10] == 7.0).all() and (t[80:] == 7.0).all()


@pytest.mark.parametrize("D", E.SCATTER_D)
def test_scatter_wave_and_tile_edges(ops, D):
    rng = np.random.RandomState(D)
    worst = 0.0
    for i, N in enumerate(E.SCATTER_N):
        k = i + D
        worst = max(worst, PL._scatter_case(ops, rng, N, D, k & 1, (k >> 1) & 1, (k >> 2) & 1, 3 if i % 2 else 0))
    print("scatter D=%d: largest |C - ref| / bound = %.3f" % (D, worst))
    E.note("B2 scatter", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("D", E.SCATTER_EXACT_D)
def test_scatter_places_every_element(ops, D):
    """exact integer data, one row: C = x x^T has a different value at every (a, b) with a <= b, so a misplaced fragment shows"""
    x = (np.arange(D, dtype=np.float64) * 3 + 1)[None, :]
    assert np.abs(x).max() ** 2 < 2.0 ** 53
    assert np.array_equal(ops.scatter_f64(dev(x)).cpu().numpy(), x.T @ x)


@pytest.mark.parametrize("N", E.SCATTER_SLAB_N)
def test_scatter_slab_growth(ops, N):
    """past 128 x 1024 rows the slab grows to a multiple of four rows: whole numbers, so every order of summation gives these bits"""
    assert ops.scatter_slab_rows(N) == E.SCATTER_SLAB_ROWS[E.SCATTER_SLAB_N.index(N)]
    X, mu, w, C = E.scatter_slab_case(N)
    for f64 in (False, True):
        got = ops.scatter_f64(dev(X.astype(np.float64) if f64 else X), dev(mu), dev(w)).cpu().numpy()
        assert np.array_equal(got, C), (N, f64)
    plain = ops.scatter_f64(dev(X)).cpu().numpy()
    assert np.array_equal(plain, (X.astype(np.float64).T @ X.astype(np.float64)))


@pytest.mark.parametrize("D", E.SEG_D)
def test_segment_sum_empty_classes(ops, D):
    rng = np.random.RandomState(300 + D)
    seg = np.array(E.SEG_OFF, dtype=np.int32)
    worst = 0.0
    for case in range(4):
        x = rng.randn(11, D).astype(np.float32 if case % 2 else np.float64)
        rows = rng.permutation(11)[:7].astype(np.int32) if case >= 2 else None
        for pad in (0, 3):
            args = (PL.pitched(x, pad), dev(seg), None if rows is None else dev(rows))
            out, cnt = ops.segment_sum_f64(*args)
            ref, rc, bound = PR.segment_sum(x, rows, seg)
            out = out.cpu().numpy()
            assert np.array_equal(cnt.cpu().numpy(), rc) and rc.tolist() == [0, 3, 0, 4, 0]
            assert not out[[0, 2, 4]].any() and np.isfinite(out).all()       # an empty class: an all-zero row, never NaN
            worst = max(worst, PL.ratio(out, ref, bound))
            mean, cnt = ops.segment_sum_f64(*args, mean=True)
            mean = mean.cpu().numpy()
            assert np.array_equal(cnt.cpu().numpy(), rc) and not mean[[0, 2, 4]].any() and np.isfinite(mean).all()
            worst = max(worst, PL.ratio(mean, *E.segment_mean_ref(ref, rc, bound)))
    E.note("B3 segment sum", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("D", E.LLR_D)
def test_plda_llr_lane_edges(ops, D):
    en, te, psi, counts = E.llr_case(D)
    tc, tl = PL._llr_tables(psi, counts)
    assert tc.cpu().tolist() == E.LLR_COUNTS
    worst = 0.0
    for T in E.LLR_T:
        ia, ib = E.llr_trials(T)
        got = ops.plda_llr(dev(en), dev(te), dev(ia), dev(ib), dev(psi), dev(counts), tc, tl)
        ref, bound = PR.llr_table(en, te, ia, ib, psi, counts)
        assert got.dtype == torch.float32 and np.isfinite(got.cpu().numpy()).all()
        worst = max(worst, PL.ratio(got.cpu().numpy().astype(np.float64), ref, bound))
    print("llr D=%d: largest error / bound = %.3f" % (D, worst))
    E.note("B4 llr", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("K,D", E.POSTERIOR_DIMS)
def test_posterior_rows_with_an_empty_class(ops, K, D):
    rng = np.random.RandomState(K * 1000 + D)
    mt, n, psi = rng.randn(K, D), rng.randint(1, 9, K).astype(np.int32), np.abs(rng.randn(D)) * 5
    n[K // 2] = 0
    if D > 1:
        psi[D // 2] = 0
    w, r = ops.plda_posterior_rows(dev(mt), dev(n), dev(psi))
    w, r = w.cpu().numpy(), r.cpu().numpy()
    g = n[:, None] * psi[None, :] / (n[:, None] * psi[None, :] + 1.0)
    assert np.allclose(w, g * mt, rtol=4 * PR.U53 * 2, atol=0)
    assert np.array_equal(r, mt - w)
    assert not w[K // 2].any() and np.array_equal(r[K // 2], mt[K // 2])     # count 0: w is exactly 0 and r is mt
    assert D == 1 or not w[:, D // 2].any()


# ==== C. eval.hip ===============================================================================================================
@pytest.mark.parametrize("layout", E.SWEEP_LAYOUTS)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_error_sweep_many_scan_blocks(ops, k, layout):
    """256, 257 and 513 scan blocks: from 257 on sweep_offsets_kernel carries a running total into its second trip"""
    T = E.sweep_sizes()[k]
    s, lab = E.sweep_case(T, layout)
    got = BK._device_sweep(ops, s, lab, E.COSTS3)
    assert got[:3] == BR.sweep(s, lab, E.COSTS3), (T, layout)
    assert (got[3], got[4]) == (int(lab.sum()), T - int(lab.sum()))


def test_error_sweep_eight_cost_triples(ops):
    from pytorch_kaldi_resnet_amd import hip
    T = ops.sweep_block() + 1
    s, lab = E.sweep_case(T, "random_ties")
    got = BK._device_sweep(ops, s, lab, E.COSTS8)
    ref = BR.sweep(s, lab, E.COSTS8)
    assert got[:3] == ref and len(got[2]) == 8 and len({r[0] for r in ref[2]}) > 1
    # the ninth is refused before any launch, by ops and by the C ABI
    sd, ld = dev(s), dev(lab)
    order = ops.sort_trials(sd)
    with pytest.raises(AssertionError):
        ops.error_sweep(sd, ld, order, E.COSTS8 + [E.COST9])
    lib = hip.lib()
    assert lib.spk_error_sweep_workspace(T, 9) == 0
    cd = dev(np.array(E.COSTS8 + [E.COST9], dtype=np.float64))
    out_d = torch.full((19,), -7.0, device="cuda", dtype=torch.float64)
    out_i = torch.full((12,), -7, device="cuda", dtype=torch.int64)
    ws = torch.zeros(lib.spk_error_sweep_workspace(T, 8) * 2, device="cuda", dtype=torch.uint8)
    rc = lib.spk_error_sweep(hip.ptr(sd), hip.ptr(ld), hip.ptr(order), hip.ptr(cd), 9, hip.ptr(out_d), hip.ptr(out_i), hip.ptr(ws), T,
                             hip.stream())
    torch.cuda.synchronize()
    assert rc < 0 and b"spk_error_sweep" in lib.spk_last_error() and b"P=9" in lib.spk_last_error()
    assert bool((out_d == -7.0).all()) and bool((out_i == -7).all()) and not bool(ws.any())      # nothing was launched


@pytest.mark.parametrize("kind", ["ties", "extremes"])
def test_sort_trials_without_padding(ops, kind):
    rng = np.random.RandomState(5)
    for T in E.sort_sizes():
        s = BK._sort_input(kind, T, rng)
        got = ops.sort_trials(dev(s)).cpu().numpy()
        assert np.array_equal(got, np.lexsort((np.arange(T), s + 0.0))), (kind, T)


# ==== D. cm.hip =================================================================================================================
def _decode_case(B, F, T, lengths, rng, variant):
    """(P [B, F, 4], codes [B, F, T], expected [B, F, T]) with the six special codes at both ends of the flat run"""
    mr, hdr = CM._headers(B, F, rng, variant % 2)
    P = np.stack([cm_ref.uint16_to_float(mr[b, 0], mr[b, 1], hdr[b]) for b in range(B)])
    N = B * F * T
    codes = rng.integers(0, 256, N).astype(np.uint8)
    sp = np.roll(CM.SPECIAL, variant)
    codes[:6], codes[N - 6:] = sp, sp[::-1]
    codes = codes.reshape(B, F, T)
    ref = np.stack([cm_ref.decode_p(P[b], codes[b]).T for b in range(B)])
    for b in range(B):
        ref[b, :, min(max(lengths[b], 0), T):] = 0                           # the clamp of spk_cm_decode
    return P, codes, ref


def _decode_everywhere(P, codes, ref, lengths):
    """decode at the four (code offset, output offset) alignments of tests/test_cm_gpu.py, with a guard around the output"""
    from pytorch_kaldi_resnet_amd import features
    B, F, T = codes.shape
    N = B * F * T
    Pd = torch.from_numpy(P).cuda()
    for coff, ooff in ((0, 0), (0, 1), (5, 0), (3, 3)):
        cbase = torch.zeros(N + 16, dtype=torch.uint8, device="cuda")
        cd = cbase[coff:coff + N].view(B, F, T)
        cd.copy_(torch.from_numpy(codes))
        obase = torch.full((N + 8,), 7.0, device="cuda")
        out = obase[ooff:ooff + N].view(B, F, T)
        assert cd.data_ptr() % 16 == coff and out.data_ptr() % 16 == 4 * ooff
        got = features.decompress(cd, Pd, lengths, out=out)
        assert got.data_ptr() == out.data_ptr()
        np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))
        guard = obase.cpu().numpy()
        assert (guard[:ooff] == 7.0).all() and (guard[ooff + N:] == 7.0).all()                  # nothing outside the tensor


@pytest.mark.parametrize("on_device", [True, False])
def test_decode_clamps_the_lengths(on_device):
    c = E.CM_CLAMP
    rng = np.random.default_rng(37)
    for variant in range(2):
        P, codes, ref = _decode_case(c["B"], c["F"], c["T"], c["lengths"], rng, variant)
        assert not ref[0].any() and not ref[1].any() and ref[2, :, -1].any() and ref[3, :, -1].any()
        lengths = torch.tensor(c["lengths"], dtype=torch.int32).cuda() if on_device else list(c["lengths"])
        _decode_everywhere(P, codes, ref, lengths)


@pytest.mark.parametrize("T", E.CM_RUN_T)
def test_decode_runs_that_cross_rows(T):
    B, F = E.CM_RUN_B, E.CM_RUN_F
    rng = np.random.default_rng(1000 + T)
    for variant in range(2):
        for lengths in ([T, T // 2], None):
            P, codes, ref = _decode_case(B, F, T, lengths if lengths is not None else [T] * B, rng, variant)
            _decode_everywhere(P, codes, ref, lengths)


@pytest.mark.parametrize("kind", E.CM_WIDE_KINDS)
@pytest.mark.parametrize("F", E.CM_WIDE_F)
def test_compress_wide_matrices(F, kind):
    """F > 256: the folds of cm_row_minmax's results take a second trip, and the matrix minimum lies in a row only it sees"""
    from pytorch_kaldi_resnet_amd import features
    x = E.wide_matrix(kind, F)
    mr, hdr, codes = features.compress(torch.from_numpy(x).cuda(), E.CM_WIDE_T)
    assert mr.shape == (3, 2) and hdr.shape == (3, F, 4) and codes.shape == (3, F, E.CM_WIDE_TCAP)
    CM._check_compressed(x, E.CM_WIDE_T, mr, hdr, codes)
