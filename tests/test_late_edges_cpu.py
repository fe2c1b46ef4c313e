"""The premises of the late edge cases (tests/late_edges_ref.py), proved without a GPU: every shape said to take a second loop
trip, another template instance, another chunk or another slab size takes it by the rule of the kernel - asked of the library
where it exports the rule, restated with its .hip line where it does not -, the label layouts of the sweep put the targets where
they say, the wide compressed matrices have their minimum where only the second trip of the fold sees it, and the reference gates
of the wide SE shapes are neither 0 nor 1."""
import numpy as np
import pytest
import torch

import cm_ref
import late_edges_ref as E
import plda_ref as PR
import se_ref as SR
import pytorch_kaldi_resnet_amd  # noqa: F401


# ---- A. se.hip -------------------------------------------------------------------------------------------------------------------
def test_wide_channels_take_more_trips_and_fewer_pixel_rows():
    assert [C for *_, C in E.SE_WIDE] == [512, 1024, 1024]
    assert [E.se_channel_trips(C) for C in (256, 512, 1024)] == [1, 2, 4]
    assert [E.se_rstep(C) for C in (256, 512, 1024)] == [4, 2, 1]
    assert all(C // 16 <= E.SE_MAX_CR for *_, C in E.SE_WIDE) and 1024 // 16 == E.SE_MAX_CR
    assert SR.chain(15, 512) == 8 + 2 and SR.chain(6, 1024) == 6 + 1           # the bound's addition count follows rstep


def test_hidden_widths_leave_a_wave_idle_or_turn_the_matrices_round():
    assert E.SE_HIDDEN == [(32, 1), (64, 3), (32, 64), (1024, 64)]
    for C, Cr in E.SE_HIDDEN:
        assert 1 <= Cr <= E.SE_MAX_CR
    assert 3 % E.SE_WAVES != 0 and 3 < E.SE_WAVES                             # Cr = 3: wave 3 never enters the `j += 4` loops
    assert 1 < E.SE_WAVES                                                      # Cr = 1: three waves idle
    assert E.SE_HIDDEN[2][1] > E.SE_HIDDEN[2][0]                               # Cr > C
    assert E.SE_MAX_CR // E.SE_WAVES == 16                                     # Cr = 64: sixteen trips per wave


@pytest.mark.parametrize("B,H,Wd,C,Cr", [s + (s[3] // 16,) for s in E.SE_WIDE] + [E.SE_HIDDEN_MAP + c for c in E.SE_HIDDEN])
def test_reference_gates_are_neither_zero_nor_one(B, H, Wd, C, Cr):
    """the scaled gate matrices keep the pre-activations small at every width: a gate that rounds to 0 or 1 has a zero
    derivative and would leave the backward chain nothing to compute"""
    d = E.se_block(B, H, Wd, C, Cr)
    ref = SR.excite_ref(d["raw"].double().sum((1, 2)), d["scale"], d["shift"], d["w1"], d["w2"], H, Wd)
    g, u = ref["g"][0], ref["u"][0]
    assert float(g.min()) > 1e-4 and float(g.max()) < 1 - 1e-4
    assert bool((u > 0).any()) and (Cr < 16 or bool((u == 0).any()))          # both sides of the hidden ReLU where there is room


def test_row_edges_give_the_chunk_counts():
    assert [H * Wd for H, Wd in E.SE_ROW_MAPS] == [511, 512, 513, 1025]
    assert [E.se_chunks(H * Wd) for H, Wd in E.SE_ROW_MAPS] == [1, 1, 2, 3]
    assert SR.SE_ROWS == 512 and E.se_chunks(SR.SE_ROWS) == 1 and E.se_chunks(SR.SE_ROWS + 1) == 2
    assert 513 - SR.SE_ROWS == 1 and 1025 - 2 * SR.SE_ROWS == 1                # the last chunk holds one pixel
    for H, Wd in E.SE_ROW_MAPS:
        wl = E.widths(E.SE_ROW_B, Wd)
        assert len(wl) == E.SE_ROW_B and all(1 <= v <= Wd for v in wl) and any(v < Wd for v in wl)


def test_big_shape_is_the_smallest_at_which_the_cap_binds():
    B, H, Wd, C = E.SE_BIG
    nq = H * Wd * C // 4
    assert nq == 8208 and nq % 8 == 0
    want, cap, launched = E.se_apply_grid(nq, B)
    assert (want, cap, launched) == (33, 32, 32)
    second = E.se_apply_second_trip(nq, B)
    assert (second.start, second.stop) == (8192, 8208)                         # threads 0 .. 15 of block 0 take a second trip
    assert [i % (launched * E.SE_THREADS) for i in second] == list(range(16))
    # the second trip is the last pixel, in the last column: it must be valid in some utterances (a value to compute) and masked in
    # others (a zero to store) - with every width below W the expected values there would all be 0, as fresh memory often is
    cols = {(i // (C // 4)) % Wd for i in second}
    wl = E.widths(B, Wd)
    assert cols == {Wd - 1} and sum(v == Wd for v in wl) >= B // 4 and sum(v < Wd for v in wl) >= B // 4
    assert E.se_chunks(H * Wd) == 2 and H * Wd - SR.SE_ROWS == 1               # the second chunk holds one pixel
    assert E.se_finalize_passes(B) == 32
    assert E.SE_BIG_LOUD // E.SE_FINAL_ROWS == 25 and E.SE_BIG_LOUD % 16 >= E.SE_FINAL_ROWS      # a late pass; lost to `b += 16`
    # the cap binds only when ceil(nq / 256) > 8192 / B, so B * nq must exceed 8192 * 256 groups: at batch 256 no map of 64
    # channels with fewer pixels has it, and at this map no batch below 249
    assert B * nq > E.SE_GRID_BLOCKS * E.SE_THREADS
    one_pixel = C // 4
    assert E.se_apply_grid(nq - one_pixel, B)[0] <= E.se_apply_grid(nq - one_pixel, B)[1]
    assert min(b for b in range(1, B + 1) if E.se_apply_grid(nq, b)[0] > E.se_apply_grid(nq, b)[1]) == 249
    assert [E.se_finalize_passes(b) for b in E.SE_PASS_B] == [1, 2, 3] and [E.se_finalize_passes(b) for b in (1, 3)] == [1, 1]


def test_bit_packing_round_trip():
    m = torch.from_numpy(np.random.RandomState(0).rand(2, 3, 5, 64) < 0.5)
    w = E.pack_bits(m)
    assert w.dtype == torch.int32 and w.numel() == 2 * 3 * 5 * 2
    assert np.array_equal(E.unpack_bits(w, m.shape), m.numpy())
    one = torch.zeros(1, 1, 1, 32, dtype=torch.bool)
    one[0, 0, 0, 5] = True
    assert int(E.pack_bits(one)[0]) == 1 << 5                                   # bit c % 32


# ---- B. plda.hip -----------------------------------------------------------------------------------------------------------------
def test_affine_dims_reach_every_instance():
    assert [E.affine_nt(Do) for Do, _ in E.AFFINE_DIMS] == E.AFFINE_NT == [1, 2, 2, 4, 4, 8, 8]
    assert {E.affine_nt(Do) for Do in (1, 17, 16, 200)} == {1, 4}             # what tests/test_plda_gpu.py reaches
    assert [E.affine_nt(D) for D in E.AFFINE_IDENTITY_D] == [2, 8, 8] and [E.affine_nt(Do) for Do, _ in E.AFFINE_EXACT] == [2, 8]
    assert E.affine_nt(E.AFFINE_RANGE_DO) == 8 and E.affine_nt(512) == 8 and E.affine_nt(64) == 1 and E.affine_nt(65) == 2


def test_scatter_dims_sit_on_the_wave_and_tile_edges():
    assert {31, 32, 33} <= set(E.SCATTER_D) and {63, 64, 65, 127, 128, 129} <= set(E.SCATTER_D)
    assert E.scatter_idle_waves(32) == [(0, 1), (1, 1)] and E.scatter_idle_waves(31) == [(0, 1), (1, 1)]
    assert E.scatter_idle_waves(33) == [] and E.scatter_idle_waves(64) == []
    assert E.scatter_idle_waves(65) == [(0, 1), (1, 1)] and E.scatter_idle_waves(128) == [] and E.scatter_idle_waves(129) != []
    assert E.scatter_idle_waves(511) == []
    assert all(D <= 512 for D in E.SCATTER_D + E.SCATTER_EXACT_D)


def test_scatter_slab_growth():
    assert [E.scatter_slab_rows(N) for N in E.SCATTER_SLAB_N] == E.SCATTER_SLAB_ROWS == [1024, 1028, 1028]
    assert [-(-N // E.scatter_slab_rows(N)) for N in E.SCATTER_SLAB_N] == [E.SC_MAX_SLABS] * 3
    assert E.SCATTER_SLAB_N[0] == E.SC_MAX_SLABS * 1024 and all(r % 4 == 0 for r in E.SCATTER_SLAB_ROWS)
    assert 131073 % 1028 == 517 and 131077 % 1028 == 521                      # the last slab ends inside a group of four rows
    X, mu, w, C = E.scatter_slab_case(1000)
    ref, _ = PR.scatter(X, mu, w)
    assert np.array_equal(ref, C) and np.abs(C).max() < 2.0 ** 53 and np.array_equal(X, np.round(X))
    assert set(np.unique(w)) == {1.0, 2.0} and np.array_equal(mu, np.round(mu)) and mu.any()


def test_segment_classes_and_their_means():
    seg = np.array(E.SEG_OFF)
    assert (np.diff(seg) == [0, 3, 0, 4, 0]).all()                             # empty first, in the middle, last
    x = np.arange(14.0).reshape(7, 2)
    ref, cnt, bound = PR.segment_sum(x, None, seg)
    assert cnt.tolist() == [0, 3, 0, 4, 0] and not ref[[0, 2, 4]].any() and not bound[[0, 2, 4]].any()
    mean, mb = E.segment_mean_ref(ref, cnt, bound)
    assert np.isfinite(mean).all() and not mean[[0, 2, 4]].any() and not mb[[0, 2, 4]].any()
    assert np.array_equal(mean[1], x[:3].mean(0)) and np.array_equal(mean[3], x[3:].mean(0))


def test_llr_counts_reach_the_last_table_entry():
    assert {D % 64 for D in E.LLR_D[:3]} == {63, 0, 1}
    assert [-(-T // 4) for T in E.LLR_T] == [1, 1, 2, 250]
    for D in E.LLR_D:
        en, te, psi, counts = E.llr_case(D)
        distinct = np.unique(counts)
        assert distinct.tolist() == E.LLR_COUNTS and len(distinct) == 5
        assert (psi == 0).any() and (psi > 0).any()
        for T in E.LLR_T:
            ia, ib = E.llr_trials(T)
            assert (counts[ia] == distinct[-1]).any() and (counts[ia] == distinct[0]).any()
            assert ia.min() >= 0 and ia.max() < len(en) and ib.min() >= 0 and ib.max() < len(te)


# ---- C. eval.hip -----------------------------------------------------------------------------------------------------------------
def test_sweep_sizes_need_the_carry():
    blk = E.sweep_block()
    assert blk >= 256 and [E.sweep_blocks(T) for T in E.sweep_sizes()] == [256, 257, 513]
    assert E.sweep_blocks(100003) <= E.EVAL_THREADS                            # the largest T of tests/test_backend_gpu.py: no carry
    assert E.sweep_sizes()[1] == 262145 or blk != 1024
    assert len(E.COSTS3) == 3 and len(set(E.COSTS8)) == E.SWEEP_MAX_COSTS == 8 and E.COST9 not in E.COSTS8
    assert all(0 < p < 1 and cm > 0 and cf > 0 for p, cm, cf in E.COSTS8 + [E.COST9])


@pytest.mark.parametrize("layout", E.SWEEP_LAYOUTS)
def test_sweep_layouts_put_the_targets_where_they_say(layout):
    edge = E.EVAL_THREADS * E.sweep_block()
    for T in E.sweep_sizes():
        s, lab = E.sweep_case(T, layout)
        assert s.shape == (T,) and lab.dtype == np.uint8
        pos = E.sorted_target_positions(s, lab)
        assert 0 < len(pos) < T                                                # both classes are non-empty
        if layout == "high":
            assert pos.min() == min(edge, T - 1)                               # no target below the edge: the carry into chunk 2 is 0
            assert T == edge or pos.min() >= edge
        elif layout == "low":
            assert pos.max() == edge - 1                                       # every target in the first 256 blocks
        else:
            assert pos.min() < edge and (T == edge or pos.max() >= edge)
            assert (len(np.unique(s)) < T // 4) == (layout == "random_ties")


def test_sort_sizes_have_no_padding():
    tile = E.sort_tile()
    assert tile & (tile - 1) == 0
    a, b, c = E.sort_sizes()
    assert (a, b, c) == (2 * tile, 4 * tile, 4 * tile - 1)
    for T in (a, b):                                                           # the padded size is T itself
        P = tile
        while P < T:
            P *= 2
        assert P == T
    assert lib_bytes(a) == a * 12 and lib_bytes(b) == b * 12 and lib_bytes(c) == b * 12


def lib_bytes(T):
    return E.lib().spk_sort_trials_workspace(T)


def test_sweep_workspace_refuses_a_ninth_triple():
    assert E.lib().spk_error_sweep_workspace(E.sweep_block() + 1, 8) > 0
    assert E.lib().spk_error_sweep_workspace(E.sweep_block() + 1, 9) == 0


# ---- D. cm.hip -------------------------------------------------------------------------------------------------------------------
def test_decode_widths_cross_rows():
    assert [E.rows_crossed(T) for T in E.CM_RUN_T] == [2, 1, 0, 0, 0]
    assert E.CM_RUN % 16 == 0 and 16 in E.CM_RUN_T                             # T = 16: a run ends exactly on the row end
    # a run that starts anywhere in a row: T = 7 reaches three further rows, the others one
    assert [max((t + E.CM_RUN - 1) // T for t in range(T)) for T in E.CM_RUN_T] == [3, 1, 1, 1, 1]
    assert [sum((t + E.CM_RUN) % T == 0 for t in range(T)) > 0 for T in E.CM_RUN_T] == [True] * 5   # some run ends on a row end
    c = E.CM_CLAMP
    assert c["lengths"][0] == 0 and c["lengths"][1] < 0 and c["lengths"][2] == c["T"] and c["lengths"][3] > c["T"]
    assert all(E.CM_RUN_B * E.CM_RUN_F * T >= 12 for T in E.CM_RUN_T)          # room for six special codes at both ends


@pytest.mark.parametrize("kind", E.CM_WIDE_KINDS)
@pytest.mark.parametrize("F", E.CM_WIDE_F)
def test_wide_matrices_hide_their_minimum_from_the_first_trip(F, kind):
    x = E.wide_matrix(kind, F)
    assert x.shape == (3, F, E.CM_WIDE_TCAP) and -(-F // E.CM_THREADS) == (1 if F == 256 else 2)
    for b, t in enumerate(E.CM_WIDE_T):
        if not t:
            continue
        m = x[b, :, :t]
        assert np.isfinite(m).all() and not (np.abs(x[b, :, t:]) < 1e29).any()  # the padding is NaN or +-1e30
        vmin, vrange, hdr, codes = cm_ref.compress(m.T)
        rmin, rmax = int(np.argmin(m.min(axis=1))), int(np.argmax(m.max(axis=1)))
        assert (rmin, rmax) == (F - 1, 0) and vmin == m[F - 1].min()
        assert (rmin >= E.CM_THREADS) == (F >= 257)
        assert m[:E.CM_THREADS].min() > vmin + 4 or F == 256                  # the first 256 rows alone give another minimum
        if kind == "constcol":
            assert (m[F // 2] == m[F // 2, 0]).all()                           # the constant column survived the two edits
