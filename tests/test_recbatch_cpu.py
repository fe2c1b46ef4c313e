"""The recording-batch object (recbatch.py), no device: its tables against spk_diar_tables, its one rule, sub(),
the chunking behind the three workspace splits of ops.py against boundaries worked by hand from the loops it replaced, and the host
dense scores with per-recording terms against the global form."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def RecBatch():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.recbatch import RecBatch
    return RecBatch


@pytest.mark.parametrize("rec_off", [[0, 1], [0, 16], [0, 17], [0, 1, 18, 50], [0, 46340]])
def test_tables_equal_the_librarys(RecBatch, rec_off):
    from pytorch_kaldi_resnet_amd import ops
    ro, tab = ops.diar_tables(rec_off, rec_off[-1])
    b = RecBatch(rec_off, rec_off[-1])
    assert b.tab.dtype == np.int64 and b.tab.shape == tab.shape and b.tab.tolist() == tab.tolist()
    assert b.rec_off.tolist() == ro.tolist() and b.rec_off.dtype == np.int64 and b.rec_off.flags.c_contiguous
    assert b.mat_off.tolist() == tab[1].tolist() and b.tile_off.tolist() == tab[2].tolist()
    assert b.R == len(rec_off) - 1 and b.Ntot == rec_off[-1] and b.n.tolist() == np.diff(rec_off).tolist()
    assert RecBatch(np.asarray(rec_off, dtype=np.int32)).tab.tolist() == tab.tolist()       # Ntot: the last entry


def test_one_rule(RecBatch):
    """every rec_off the library refuses (test_diar_cpu.py's list) is a ValueError here, with the messages diarize always gave"""
    for ro, N, msg in [([1, 5], 5, "start at 0"), ([0, 2, 2, 5], 5, "increase strictly"), ([0, 3, 2, 5], 5, "increase strictly"),
                       ([0, 2, 4], 5, "end at 5"), ([0, 46341], 46341, "fewer than 2\\^31"), ([0, 40000, 80000], 80000, "fewer than 2\\^31")]:
        with pytest.raises(ValueError, match=msg):
            RecBatch(ro, N)
    for ro in ([0], [], [0.0, 3.0], [[0, 3]]):
        with pytest.raises(ValueError, match="one-dimensional integer array of at least two entries"):
            RecBatch(ro)
    b = RecBatch([0, 3, 8])
    assert RecBatch.of(b) is b and RecBatch.of(b, 8) is b and RecBatch.of([0, 3, 8], 8).tab.tolist() == b.tab.tolist()
    with pytest.raises(ValueError):
        RecBatch.of(b, 9)


N5 = (3, 5, 2, 7, 1)                                                # rec_off 0 3 8 10 17 18, mat_off 0 9 34 38 87 88


def test_sub_rebases_and_the_whole_is_the_batch(RecBatch):
    b = RecBatch(np.concatenate([[0], np.cumsum(N5)]))
    s, r0, r1 = b.sub(1, 3)
    assert (r0, r1) == (3, 10) and s.rec_off.tolist() == [0, 5, 7] and s.Ntot == 7 and s.R == 2
    assert s.mat_off.tolist() == [0, 25, 29] and s.tile_off.tolist() == [0, 1, 2] and s is not b
    s, r0, r1 = b.sub(4, 5)
    assert (r0, r1) == (17, 18) and s.tab.tolist() == [[0, 1], [0, 1], [0, 1]]
    s, r0, r1 = b.sub(0, 5)
    assert s is b and (r0, r1) == (0, 18)


ONE = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]


def test_chunks_are_the_boundaries_of_the_loops_they_replace(RecBatch):
    """the expected lists: the `lo`/`hi` loops ahc_batch, vbx_batch and pca_plda_batch ran before, worked by hand on n = N5"""
    b = RecBatch(np.concatenate([[0], np.cumsum(N5)]))
    # ahc_batch: 8 bytes per matrix entry; the recordings cost 72, 200, 32, 392 and 8
    ahc = lambda lo, hi: 8 * int(b.mat_off[hi] - b.mat_off[lo])  # noqa: E731
    assert list(b.chunks(ahc, 7)) == ONE                            # below every recording: one always goes
    assert list(b.chunks(ahc, 8 * 38)) == [(0, 3), (3, 4), (4, 5)]  # 72 + 200 + 32 fits exactly; 392 alone exceeds it and goes alone
    assert list(b.chunks(ahc, 8 * 88)) == [(0, 5)] and list(b.chunks(ahc, 1 << 31)) == [(0, 5)]
    # vbx_batch with Smax = 2, D = 4: 56 bytes per row and 64 per recording; the recordings cost 232, 344, 176, 456 and 120
    per_row, per_rec = 8 * (3 + 2 * 2), 8 * 2 * 4
    vbx = lambda lo, hi: per_row * int(b.rec_off[hi] - b.rec_off[lo]) + per_rec * (hi - lo)  # noqa: E731
    assert list(b.chunks(vbx, 100)) == ONE
    assert list(b.chunks(vbx, 600)) == [(0, 2), (2, 3), (3, 5)]     # 576 | 176 (+ 456 = 632) | 456 + 120 = 576
    assert list(b.chunks(vbx, 1328)) == [(0, 5)] and list(b.chunks(vbx, 1327)) == [(0, 4), (4, 5)]
    # pca_plda_batch: `per` bytes per recording, min(budget // per, 65535) recordings per launch, at least one
    pca = lambda lo, hi: 1000 * (hi - lo)  # noqa: E731
    assert list(b.chunks(pca, 999, max_recs=65535)) == ONE
    assert list(b.chunks(pca, 2500, max_recs=65535)) == [(0, 2), (2, 4), (4, 5)]
    assert list(b.chunks(pca, 1 << 31, max_recs=65535)) == [(0, 5)]
    assert list(b.chunks(pca, 1 << 31, max_recs=2)) == [(0, 2), (2, 4), (4, 5)]     # the cap on the recordings of one launch
    assert list(b.chunks(pca, 1 << 31, max_recs=3)) == [(0, 3), (3, 5)] and list(b.chunks(pca, 1500, max_recs=3)) == ONE


def test_host_scores_broadcast_the_global_terms(RecBatch):
    """g tiled to [R][D] and K repeated to [R] give the bits of g [D] and a number"""
    from pytorch_kaldi_resnet_amd import diarize
    rng = np.random.RandomState(5)
    ro = np.concatenate([[0], np.cumsum((1, 17, 40))])
    D, R = 8, 3
    U, q, g, K = rng.randn(ro[-1], D), rng.randn(ro[-1]), rng.uniform(0.1, 1.0, D), 0.37
    one = diarize._score_rows(U, q, g, K, ro, "host", False)
    per = diarize._score_rows(U, q, np.tile(g, (R, 1)), np.full(R, K), RecBatch(ro), "host", False)
    assert one.dtype == np.float32 and one.size == 1 + 17 * 17 + 40 * 40 and one.tobytes() == per.tobytes()
    g2 = np.tile(g, (R, 1))
    g2[1] *= 2.0                                                    # and the terms are the recording's own
    two = diarize._score_rows(U, q, g2, np.full(R, K), ro, "host", False)
    assert two[:1].tobytes() == one[:1].tobytes() and two[290:].tobytes() == one[290:].tobytes()
    assert not np.array_equal(two[1:290], one[1:290])
