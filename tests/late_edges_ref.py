"""Case lists and input builders of the edge tests of the four kernel files that arrived inside feature work: csrc/se.hip
(squeeze-and-excitation), csrc/plda.hip (PLDA back end), csrc/eval.hip (trial sort and error-rate sweep) and csrc/cm.hip (Kaldi
compressed matrices).  This module builds inputs and expectations only: it imports nothing that touches the GPU and never sees
a kernel's output.  tests/test_late_edges_cpu.py proves, without a GPU, the premises the lists rest on (which size takes which
loop trip, template instance or chunk); tests/test_late_edges_gpu.py runs the kernels on them.

The fp64 references and per-element bounds are the ones the feature tests use: se_ref.py, plda_ref.py, backend_ref.py, cm_ref.py.
Tile sizes that the library exports (spk_se_chunks, spk_eval_tile, spk_scatter_slab_rows) are asked of the library - host code,
no GPU needed.  The rules it does not export are restated below, each with the .hip line it mirrors."""
import numpy as np
import torch

import backend_ref as BR
import cm_ref
import plda_ref as PR
from oracle import weights as W

RATIOS = {}             # group -> largest error / bound seen by the GPU tests (printed when the module finishes)


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), float(ratio))
    return ratio


def lib():
    from pytorch_kaldi_resnet_amd import hip
    return hip.lib()


# ==== A. se.hip =================================================================================================================
SE_THREADS = 256        # se.hip:35 / :225 / :340  __launch_bounds__(256) of every SE kernel
SE_GRID_BLOCKS = 8192   # se.hip:217  `long long cap = 8192 / B;` in se_apply_grid
SE_FINAL_ROWS = 8       # se.hip:361  `for (int b = row; b < B; b += 8)` in se_gate_finalize_kernel (row = tid >> 5)
SE_MAX_CR = 64          # se.hip:21
SE_WAVES = 4            # se.hip:185 / :309  `for (int j = wave; j < Cr; j += 4)`


def se_chunks(HW):
    """reduction blocks per utterance, as the library reports them (spk_se_chunks)"""
    return int(lib().spk_se_chunks(int(HW)))


def se_apply_grid(nq, B):
    """(blocks wanted, cap, blocks launched) per utterance of the two apply kernels: se.hip:215-221 se_apply_grid"""
    want = (nq + SE_THREADS - 1) // SE_THREADS
    cap = max(SE_GRID_BLOCKS // B, 1)
    return want, cap, max(min(want, cap), 1)


def se_apply_second_trip(nq, B):
    """group indices i of one utterance that a thread reaches on a trip after its first (`i += stride`, se.hip:243 / :450)"""
    stride = se_apply_grid(nq, B)[2] * SE_THREADS
    return range(stride, nq)


def se_finalize_passes(B):
    """trips of the utterance loop of se_gate_finalize_kernel for the row that takes most (se.hip:361 / :371)"""
    return -(-B // SE_FINAL_ROWS)


def se_channel_trips(C):
    """trips of the `c += 256` loops of the excite and gate-chain kernels (se.hip:177 / :196 / :299 / :320)"""
    return -(-C // SE_THREADS)


def se_rstep(C):
    """pixel rows a reduction block walks at once: se.hip:43 `rstep = 256 / qpr`, qpr = C / 4"""
    return SE_THREADS // (C // 4)


SE_WIDE = [(2, 3, 5, 512), (1, 2, 3, 1024), (9, 1, 1, 1024)]            # A.1 (B, H, W, C), Cr = C / 16
SE_HIDDEN = [(32, 1), (64, 3), (32, 64), (1024, 64)]                    # A.2 (C, Cr) at B = 3, 5 x 7
SE_HIDDEN_MAP = (3, 5, 7)
SE_ROW_MAPS = [(7, 73), (16, 32), (19, 27), (25, 41)]                   # A.3 (H, W): HW = 511, 512, 513, 1025 at C = 32, B = 2
SE_ROW_C, SE_ROW_B = 32, 2
SE_BIG = (256, 19, 27, 64)                                              # A.4: the smallest B x nq at which the grid cap binds
SE_BIG_LOUD = 200                                                       # the utterance whose dq is 10^6 times the others'
SE_PASS_B = [8, 9, 17]                                                  # A.4 companion: 1, 2 and 3 finalize passes
SE_PASS_MAPS = [(1, 1, 32), (5, 7, 64)]


def rnd(seed, *shape, scale=1.0, shift=0.0):
    """float32 tensor of hashed uniforms in shift +- scale (the builder of tests/test_se_gpu.py)"""
    n = int(np.prod(shape))
    return torch.from_numpy(((W.hash_uniform(seed, 1, n) * 2 - 1) * scale + shift).astype(np.float32).reshape(shape))


def small_ints(seed, *shape):
    """whole numbers in [-3, 3] as float32: every float32 partial sum of them is exact"""
    n = int(np.prod(shape))
    return torch.from_numpy((np.floor(W.hash_uniform(seed, 4, n) * 7) - 3).astype(np.float32).reshape(shape))


def widths(B, Wd):
    """valid widths of a batch: 1, W, W / 2, W - 1, 1, ... (at least 1): the last column is valid in some rows and not in others"""
    return [max(1, v) for v in ([1, Wd, Wd // 2, Wd - 1] * B)[:B]]


def bn_rows(raw, seed):
    """mean, invstd, scale, shift, gamma (float32) of a training-mode BatchNorm over raw [B,H,W,C]"""
    C = raw.shape[-1]
    x = raw.double().reshape(-1, C)
    mean = x.mean(0)
    inv = 1 / torch.sqrt(((x - mean) ** 2).mean(0) + 1e-5)
    gamma, beta = rnd(seed, C, scale=0.5, shift=1.0), rnd(seed + 1, C, scale=0.3)
    mean, inv = mean.float(), inv.float()
    scale = gamma * inv
    return mean, inv, scale, beta - mean * scale, gamma


def gate_weights(seed, C, Cr):
    """(W1 [Cr][C], W2 [C][Cr]): the +-0.5 / +-2 fills of tests/test_se_gpu.py at C = 32, Cr = 2, scaled by sqrt(32 / C) and
    sqrt(2 / Cr) so that the pre-activations keep that spread at every width and the gates stay inside (0, 1)"""
    return rnd(seed, Cr, C, scale=0.5 * (32.0 / C) ** 0.5), rnd(seed + 1, C, Cr, scale=2.0 * (2.0 / Cr) ** 0.5)


def se_block(B, H, Wd, C, Cr=None, seed=30):
    """host tensors of one SE block tail: raw, its BatchNorm rows, gate matrices, shortcut and a gradient"""
    Cr = C // 16 if Cr is None else Cr
    raw = rnd(seed, B, H, Wd, C, scale=1.5, shift=0.3)
    mean, inv, scale, shift, gamma = bn_rows(raw, seed + 1)
    w1, w2 = gate_weights(seed + 3, C, Cr)
    return dict(raw=raw, mean=mean, inv=inv, scale=scale, shift=shift, gamma=gamma, w1=w1, w2=w2,
                res=rnd(seed + 5, B, H, Wd, C), dout=rnd(seed + 6, B, H, Wd, C, scale=2.0))


def pack_bits(mask):
    """bool [B,H,W,C] -> int32 [B*H*W*(C/32)]: word [pixel][C/32], bit c % 32 (the layout se_apply writes)"""
    C = mask.shape[-1]
    m = np.ascontiguousarray(mask.numpy().reshape(-1, C // 32, 32)).astype(np.uint8)
    return torch.from_numpy(np.packbits(m, axis=-1, bitorder="little").view("<u4").view(np.int32).reshape(-1).copy())


def unpack_bits(words, shape):
    """the inverse of pack_bits: int32 words -> bool array of `shape` = (B, H, W, C)"""
    C = shape[-1]
    w = words.cpu().view(-1, C // 32).numpy().astype(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(shape).astype(bool)


# ==== B. plda.hip ===============================================================================================================
def affine_nt(Do):
    """the NT instance affine_launch picks: plda.hip:264-269, need = ceil(ceil(Do / 16) / 4) -> 1, 2, 4 or 8"""
    need = -(-(-(-Do // 16)) // 4)
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8


AFFINE_DIMS = [(64, 16), (65, 33), (128, 64), (129, 16), (256, 40), (257, 24), (512, 512)]        # (Do, Di)
AFFINE_NT = [1, 2, 2, 4, 4, 8, 8]
AFFINE_N = [1, 33, 65]
AFFINE_IDENTITY_D = [65, 300, 512]
AFFINE_EXACT = [(100, 33), (300, 17)]
AFFINE_RANGE_DO = 300

SC_TILE, SC_WAVE_TILE = 64, 32          # plda.hip:20 SC_TILE; :52 `a0 = ti * SC_TILE + wm * 32`, the early return at :53
SC_MAX_SLABS = 128                      # plda.hip:22
SCATTER_D = [31, 32, 33, 63, 64, 65, 127, 128, 129, 511]
SCATTER_N = [1, 5, 65]
SCATTER_EXACT_D = [65, 129, 511]
SCATTER_SLAB_N = [131072, 131073, 131077]
SCATTER_SLAB_ROWS = [1024, 1028, 1028]
SCATTER_SLAB_D = 5


def scatter_slab_rows(N):
    return int(lib().spk_scatter_slab_rows(int(N)))


def scatter_idle_waves(D):
    """(wm, wn) sub-tiles of the last diagonal tile that return at `a0 >= D || b0 >= D` (plda.hip:53)"""
    t = (-(-D // SC_TILE)) - 1
    return [(wm, wn) for wm in range(2) for wn in range(2) if wm <= wn
            and (t * SC_TILE + wm * SC_WAVE_TILE >= D or t * SC_TILE + wn * SC_WAVE_TILE >= D)]


def scatter_slab_case(N, seed=0):
    """(X [N][5] float32 whole numbers in [-3, 3], mu whole numbers, w in {1, 2}, C exact): every product and every partial sum is
    a whole number below 2^53, so any summation order gives these bits"""
    rng = np.random.RandomState(N % 1000 + seed)
    X = rng.randint(-3, 4, (N, SCATTER_SLAB_D)).astype(np.float32)
    mu = rng.randint(-2, 3, SCATTER_SLAB_D).astype(np.float64)
    w = rng.randint(1, 3, N).astype(np.float64)
    c = X.astype(np.int64) - mu.astype(np.int64)
    C = (c * w.astype(np.int64)[:, None]).T @ c
    return X, mu, w, C.astype(np.float64)


SEG_OFF = [0, 0, 3, 3, 7, 7]            # classes 0, 2 and 4 are empty: first, in the middle, last
SEG_D = [1, 17, 256]


def segment_mean_ref(ref, cnt, bound):
    """means and their bound from plda_ref.segment_sum's (sums, counts, bound); an empty class has mean 0 exactly (plda.hip:142)"""
    n = np.maximum(cnt, 1)[:, None].astype(np.float64)
    return ref / n, (bound + np.abs(ref) * PR.U53) / n


LLR_D = [63, 64, 65, 512]
LLR_T = [3, 4, 5, 1000]                 # plda.hip:323: four trials per block
LLR_COUNTS = [1, 2, 3, 5, 7]


def llr_case(D, seed=0):
    """(en, te, psi, counts): 23 enrolment rows whose counts cycle through LLR_COUNTS, 31 test rows, every fifth psi 0"""
    rng = np.random.RandomState(70 + D + seed)
    en, te = rng.randn(23, D) * 2, rng.randn(31, D) * 2
    psi = np.abs(rng.randn(D)) * 20
    psi[::5] = 0
    counts = np.array([LLR_COUNTS[i % 5] for i in range(23)], dtype=np.int32)
    return en, te, psi, counts


def llr_trials(T, seed=0):
    rng = np.random.RandomState(900 + T + seed)
    ia, ib = rng.randint(0, 23, T).astype(np.int32), rng.randint(0, 31, T).astype(np.int32)
    ia[0], ib[0] = 0, 0
    ia[-1], ib[-1] = 22, 30             # first and last rows of both tables
    ia[T // 2] = 4                      # counts[4] = 7: the last table entry
    return ia, ib


POSTERIOR_DIMS = [(1, 1), (16, 16), (257, 1), (3, 512)]


# ==== C. eval.hip ===============================================================================================================
EVAL_THREADS = 256      # eval.hip:13; sweep_offsets_kernel scans `lo += EVAL_THREADS` blocks per trip with a carry (eval.hip:246)
SWEEP_MAX_COSTS = 8     # eval.hip:17
COSTS3 = [(0.01, 1.0, 1.0), (0.001, 1.0, 1.0), (0.05, 10.0, 1.0)]
COSTS8 = COSTS3 + [(0.5, 1.0, 1.0), (0.1, 2.0, 3.0), (0.02, 1.0, 5.0), (0.3, 7.0, 1.0), (0.9, 1.0, 2.0)]
COST9 = (0.25, 1.0, 1.0)
SWEEP_LAYOUTS = ["random", "random_ties", "high", "low"]


def sweep_block():
    return int(lib().spk_eval_tile(1))


def sort_tile():
    return int(lib().spk_eval_tile(0))


def sweep_sizes():
    blk = sweep_block()
    return [EVAL_THREADS * blk, EVAL_THREADS * blk + 1, 2 * EVAL_THREADS * blk + 5]


def sweep_blocks(T):
    return -(-T // sweep_block())


def sweep_case(T, layout, seed=0):
    """(scores float64 [T], labels uint8 [T]).  random / random_ties: labels at rate 0.2, scores randn + 2 label (rounded to
    quarters).  high / low: the sorted list is fixed first - distinct scores 0.25 k, targets at random sorted positions at or above
    / below `edge` = 256 scan blocks - and then shuffled; at T = 256 blocks there is no position above the edge, and `high` is the
    one target at the last position."""
    rng = np.random.RandomState(T % 9973 + 17 * SWEEP_LAYOUTS.index(layout) + seed)
    if layout in ("random", "random_ties"):
        lab = (rng.rand(T) < 0.2).astype(np.uint8)
        s = rng.randn(T) + 2.0 * lab
        return (np.round(s * 4) / 4 if layout == "random_ties" else s), lab
    edge = EVAL_THREADS * sweep_block()
    lo, hi = (min(edge, T - 1), T) if layout == "high" else (0, edge)
    pos = np.flatnonzero(rng.rand(hi - lo) < 0.2) + lo
    pos = np.union1d(pos, [lo if layout == "high" else hi - 1])      # the position next to the edge is a target
    lab_sorted = np.zeros(T, dtype=np.uint8)
    lab_sorted[pos] = 1
    perm = rng.permutation(T)
    s, lab = np.empty(T), np.empty(T, dtype=np.uint8)
    s[perm] = np.arange(T) * 0.25
    lab[perm] = lab_sorted
    return s, lab


def sorted_target_positions(s, lab):
    """positions of the targets in the reference's sorted list"""
    return np.flatnonzero(np.asarray(lab)[BR.sort_order(s)] != 0)


def sort_sizes():
    tile = sort_tile()
    return [2 * tile, 4 * tile, 4 * tile - 1]


# ==== D. cm.hip =================================================================================================================
CM_THREADS = 256        # cm.hip:34; the fold `for (int g = tid; g < F; g += CM_THREADS)` at cm.hip:213
CM_RUN = 16             # cm.hip:16: a lane takes 16 consecutive codes
CM_CLAMP = dict(B=4, F=3, T=37, lengths=[0, -5, 37, 1000])
CM_RUN_T = [7, 15, 16, 17, 31]
CM_RUN_B, CM_RUN_F = 2, 5
CM_WIDE_F = [256, 257, 300]
CM_WIDE_T, CM_WIDE_TCAP = [9, 0, 64], 67
CM_WIDE_KINDS = ["logmel", "constcol"]


def rows_crossed(T):
    """rows that a run of 16 codes starting at t = 0 of a row reaches beyond its first"""
    return (CM_RUN - 1) // T


def wide_matrix(kind, F, seed=0):
    """x [3][F][Tcap] float32 for cm_compress: cm_ref.make_matrix rows with the matrix's maximum moved into row 0 and its minimum
    into the last row (index >= 256 from F = 257 on: only the second trip of the fold sees it); NaN / +-1e30 past T[b]"""
    rng = np.random.default_rng(1000 + F + seed)
    x = np.empty((len(CM_WIDE_T), F, CM_WIDE_TCAP), dtype=np.float32)
    for b, t in enumerate(CM_WIDE_T):
        x[b] = (np.nan, 1e30, -1e30)[b % 3]
        if t:
            m = cm_ref.make_matrix(kind, t, F, rng).T                # [F, t]
            m[0, t // 3] = m.max() + np.float32(5)
            m[F - 1, t // 2] = m.min() - np.float32(5)
            x[b, :, :t] = m
    return x
