"""DESIGN.md section 6s restated on its own, for the calibration tests: nothing here imports the package.
  - pool-adjacent-violators as the minimax formula over the pools of equal scores, in fractions.Fraction: O(P^2) values of O(P) work
    each, for small cases only;
  - Cllr, minCllr and the training objective with its gradient and Hessian in numpy.longdouble;
  - the bounds the device results are held to, and the cases they are held to them on."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
LN2 = np.log(LD(2.0))
U = 2.0 ** -53                                   # unit roundoff of fp64


# ---- pools ----------------------------------------------------------------------------------------------------------------------------
def tie_pools(scores, labels):
    """[(targets, trials)] of every run of equal scores, ascending; Python compares -0.0 == 0.0; order: the stable sort"""
    order = sorted(range(len(scores)), key=lambda i: scores[i])
    pools = []
    for k, i in enumerate(order):
        if k == 0 or scores[i] != scores[order[k - 1]]:
            pools.append([0, 0])
        pools[-1][0] += int(labels[i] != 0)
        pools[-1][1] += 1
    return [tuple(p) for p in pools], order


def pav_minimax(pools):
    """value_i = max over a <= i of min over b >= i of (sum t / sum n over pools a .. b); pools with equal value are one final pool"""
    P = len(pools)
    ct, cn = [0], [0]
    for t, n in pools:
        ct.append(ct[-1] + t)
        cn.append(cn[-1] + n)
    value = []
    for i in range(P):
        value.append(max(min(Fraction(ct[b + 1] - ct[a], cn[b + 1] - cn[a]) for b in range(i, P)) for a in range(i + 1)))
    assert all(value[i] <= value[i + 1] for i in range(P - 1))
    out = []
    for i, (t, n) in enumerate(pools):
        if i and value[i] == value[i - 1]:
            out[-1] = (out[-1][0] + t, out[-1][1] + n)
        else:
            out.append((t, n))
    return out


def pool_index(pools, order):
    """each trial's pool from the final pools and the sort order"""
    out, pos = [0] * len(order), 0
    for q, (_, n) in enumerate(pools):
        for i in order[pos:pos + n]:
            out[i] = q
        pos += n
    assert pos == len(order)
    return out


# ---- longdouble -------------------------------------------------------------------------------------------------------------------------
def softplus_ld(x):
    x = np.asarray(x, dtype=LD)
    return np.maximum(x, LD(0)) + np.log1p(np.exp(-np.abs(x)))


def cllr_ld(llr, labels):
    llr, tar = np.asarray(llr, dtype=LD), np.asarray(labels) != 0
    return (softplus_ld(-llr[tar]).sum() / LD(tar.sum()) + softplus_ld(llr[~tar]).sum() / LD((~tar).sum())) / (2 * LN2)


def min_cllr_ld(pools, n_tar, n_non):
    a, b = LD(0), LD(0)
    for t, n in pools:
        if 0 < t < n:
            a += LD(t) * np.log1p(LD(n - t) / LD(t) * (LD(n_tar) / LD(n_non)))
            b += LD(n - t) * np.log1p(LD(t) / LD(n - t) * (LD(n_non) / LD(n_tar)))
    return (a / LD(n_tar) + b / LD(n_non)) / (2 * LN2)


def act_dcf(llr, labels, p, c_miss, c_fa):
    """(actDCF, miss, fa, eta) by the stated expressions in Python floats"""
    eta = math.log(c_fa * (1 - p)) - math.log(c_miss * p)
    miss = sum(1 for x, l in zip(llr, labels) if l and x < eta)
    fa = sum(1 for x, l in zip(llr, labels) if not l and x >= eta)
    n_tar = sum(1 for l in labels if l)
    n_non = len(labels) - n_tar
    return (c_miss * (miss / float(n_tar)) * p + c_fa * (fa / float(n_non)) * (1 - p)) / min(c_miss * p, c_fa * (1 - p)), miss, fa, eta


def objective_ld(cols, labels, theta, p_target, l2):
    """f, g [K + 1], H [K + 1][K + 1] of the objective at theta in longdouble, and for each of them the sum of |term| and A =
    max_i (sum_k |w_k s_ik| + |b| + |tau|) that the evaluation bound needs"""
    c = np.asarray(cols, dtype=LD)
    K, T = c.shape
    th = np.asarray(theta, dtype=LD)
    tar = np.asarray(labels) != 0
    n_tar, n_non = int(tar.sum()), int((~tar).sum())
    p = LD(p_target)
    tau = np.log(p / (1 - p))
    S = np.concatenate([c, np.ones((1, T), dtype=LD)])
    z = (th[:, None] * S).sum(0)
    y = np.where(tar, -(z + tau), z + tau)
    cw = np.where(tar, p / LD(n_tar), (1 - p) / LD(n_non))
    sig = 1 / (1 + np.exp(-y))
    dz = np.where(tar, -sig, sig)
    h = sig * (1 / (1 + np.exp(y)))
    ft = cw * softplus_ld(y)
    reg = LD(l2) / 2 * (th[:K] ** 2).sum()
    f, f_abs = ft.sum() + reg, np.abs(ft).sum() + abs(reg)
    g, g_abs = np.zeros(K + 1, dtype=LD), np.zeros(K + 1, dtype=LD)
    H, H_abs = np.zeros((K + 1, K + 1), dtype=LD), np.zeros((K + 1, K + 1), dtype=LD)
    for j in range(K + 1):
        t = cw * dz * S[j]
        r = LD(l2) * th[j] if j < K else LD(0)
        g[j], g_abs[j] = t.sum() + r, np.abs(t).sum() + abs(r)
        for k in range(K + 1):
            t = cw * h * S[j] * S[k]
            r = LD(l2) if j == k and j < K else LD(0)
            H[j, k], H_abs[j, k] = t.sum() + r, np.abs(t).sum() + r
    A = float((np.abs(th[:K, None] * c).sum(0) + abs(th[K]) + abs(tau)).max())
    return {"f": f, "g": g, "H": H, "f_abs": f_abs, "g_abs": g_abs, "H_abs": H_abs, "A": A, "T": T, "K": K}


# ---- bounds (derivations: DESIGN.md section 6s) -----------------------------------------------------------------------------------
def sum_bound(count, value):
    """a sum of `count` non-negative fp64 terms against its exact value: (count + 64) 2^-52 value"""
    return (count + 64) * 2.0 ** -52 * float(value)


def eval_bound(T, K, A, sum_abs):
    """one entry of f, g or H from one evaluation pass: 2^-53 (T + 64 + (K + 2) A) sum |term|"""
    return U * (T + 64 + (K + 2) * A) * float(sum_abs)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def gaussian_llr(seed, T, mu=3.0, p=0.3):
    """(labels, llr): llr ~ N(+-mu, 2 mu), what a calibrated system gives; both classes present"""
    rng = np.random.RandomState(seed)
    lab = (rng.rand(T) < p).astype(np.uint8)
    lab[0], lab[1] = 1, 0
    llr = np.where(lab > 0, mu, -mu) + math.sqrt(2 * mu) * rng.randn(T)
    return lab, llr


def train_columns(seed, T, K):
    """K noisy affine views of one Gaussian LLR list, not separable: (labels, columns [K][T])"""
    lab, llr = gaussian_llr(seed, T)
    rng = np.random.RandomState(seed + 1000)
    cols = [(llr - 1.5) / 4]
    for k in range(1, K):
        cols.append((llr + (1.0 + k) * rng.randn(T)) / (2.0 + k) + 0.25 * k)
    return lab, np.array(cols)


SIZES = ("2", "3", "63", "64", "65", "block-1", "block", "block+1", "2block+1", "3tile+1")
PAV_CASE_NAMES = ["tied_" + n for n in SIZES] + ["distinct_" + n for n in SIZES] + [
    "block_without_targets_block_of_targets", "all_equal", "tie_across_block_edge", "ties_at_tile_edge", "tie_longer_than_a_tile",
    "alternating", "alternating_from_target", "separated", "reversed", "signed_zeros", "separated_shuffled",
    "more_final_pools_than_a_tile"]


def pav_cases(block, tile):
    """name -> (scores, labels): the smallest lists at which the pooling kernels can go wrong (block: trials per block of the scan,
    tile: pools per tile).  Every list has both classes."""
    rng = np.random.RandomState(11)
    out = {}

    def fix(lab):
        lab = np.asarray(lab, dtype=np.uint8).copy()
        if lab.sum() == 0:
            lab[0] = 1
        if lab.sum() == lab.size:
            lab[-1] = 0
        return lab
    for name, T in zip(SIZES, (2, 3, 63, 64, 65, block - 1, block, block + 1, 2 * block + 1, 3 * tile + 1)):
        out["tied_" + name] = (rng.randint(0, max(T // 3, 2), size=T) / 8.0, fix(rng.rand(T) < 0.4))
        s = rng.permutation(T) / 16.0
        out["distinct_" + name] = (s, fix((s * 16 + rng.randn(T) * T / 4) > T / 2))
    T = 3 * block
    lab = np.concatenate([np.zeros(block), np.ones(block), rng.rand(block) < 0.5])
    out["block_without_targets_block_of_targets"] = (np.arange(T) / 4.0, fix(lab))
    out["all_equal"] = (np.full(block + 7, 0.25), fix(rng.rand(block + 7) < 0.5))
    s = np.arange(2 * block + 5, dtype=np.float64)
    s[block - 4:block + 6] = s[block - 4]
    out["tie_across_block_edge"] = (s, fix(rng.rand(s.size) < 0.5))
    s = np.arange(2 * tile + 9, dtype=np.float64)                      # pools tile - 1 and tile are runs of five
    s[tile - 1:tile + 4] = s[tile - 1]
    s[tile + 4:tile + 9] = s[tile + 4]
    out["ties_at_tile_edge"] = (s, fix(rng.rand(s.size) < 0.5))
    s = np.arange(3 * tile, dtype=np.float64)
    s[tile // 2:2 * tile] = s[tile // 2]
    out["tie_longer_than_a_tile"] = (s, fix(rng.rand(s.size) < 0.5))
    T = 2 * block + 1
    out["alternating"] = (np.arange(T) / 2.0, np.arange(T) % 2)
    out["alternating_from_target"] = (np.arange(T) / 2.0, (np.arange(T) + 1) % 2)
    out["separated"] = (np.arange(T) - 100.0, np.arange(T) >= 700)
    out["reversed"] = (np.arange(T) - 100.0, np.arange(T) < 700)
    out["signed_zeros"] = (np.array([-0.0, 0.0, 1.0, 0.0, -0.0, -1.0, -0.0]), np.array([1, 0, 1, 0, 1, 0, 0]))
    perm = rng.permutation(T)                                          # the same through a shuffle: order is not position
    out["separated_shuffled"] = ((np.arange(T) - 100.0)[perm], (np.arange(T) >= 700)[perm])
    # pool k: k targets among k + 1 equal scores - no two merge, and more final pools than one tile holds
    n = np.arange(1, tile + 80)
    s = np.repeat(np.arange(n.size, dtype=np.float64), n)
    lab = np.concatenate([np.r_[0, np.ones(k - 1)] for k in n])
    out["more_final_pools_than_a_tile"] = (s, lab)
    assert sorted(out) == sorted(PAV_CASE_NAMES)
    return {k: (np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(l, dtype=np.uint8)) for k, (s, l) in out.items()}
