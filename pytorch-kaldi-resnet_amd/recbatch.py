"""The layout of a batch of recordings, derived and checked once: recording r owns the rows rec_off[r] ..
rec_off[r + 1] - 1 of every [Ntot] table, an n x n matrix at element mat_off[r] of the flat score array and its 16 x 16 upper-triangle
tiles from tile_off[r] on.  Needs neither torch nor the library to import; the device copy of the table is made on first use."""
import numpy as np


class RecBatch:
    """rec_off [R + 1] (contiguous int64), n [R], R, Ntot, mat_off and tile_off [R + 1], and tab int64 [3][R + 1] = rec_off, mat_off,
    tile_off: what spk_diar_tables writes and the kernels read.  One rule, spk_diar_check's: integers in one dimension, at least two
    of them, from 0 strictly up to Ntot (None: the last entry), sum of n^2 below 2^31; anything else raises ValueError."""

    def __init__(self, rec_off, Ntot=None):
        ro = np.asarray(rec_off)
        if ro.dtype.kind not in "iu" or ro.ndim != 1 or ro.size < 2:
            raise ValueError("rec_off must be a one-dimensional integer array of at least two entries")
        self.R, self.Ntot = ro.size - 1, int(ro[-1] if Ntot is None else Ntot)
        self.n = n = np.diff(ro.astype(np.int64))
        if ro[0] != 0 or ro[-1] != self.Ntot or (n < 1).any():
            raise ValueError("rec_off must start at 0, increase strictly (no empty recording) and end at %d" % self.Ntot)
        t = (n + 15) // 16
        self.tab = np.zeros((3, ro.size), dtype=np.int64)
        self.tab[0] = ro
        np.cumsum(n * n, out=self.tab[1, 1:])
        np.cumsum(t * (t + 1) // 2, out=self.tab[2, 1:])
        self.rec_off, self.mat_off, self.tile_off = self.tab
        if self.mat_off[-1] >= 1 << 31:
            raise ValueError("the score matrices of one batch must hold fewer than 2^31 entries, got %d" % self.mat_off[-1])
        self._dev = {}

    @classmethod
    def of(cls, rec, Ntot=None):
        """rec as it is where it is a batch already (of Ntot rows), else the batch of the host rec_off"""
        if isinstance(rec, cls) and Ntot is not None and rec.Ntot != Ntot:
            raise ValueError("the batch holds %d rows, the table %d" % (rec.Ntot, Ntot))
        return rec if isinstance(rec, cls) else cls(rec, Ntot)

    def _upload(self, device):
        import torch
        return torch.from_numpy(self.tab).to(device)

    def table(self, device):
        """tab on the device, uploaded on first use: every launch on this batch reads the one copy.  Its first row is rec_off."""
        if str(device) not in self._dev:
            self._dev[str(device)] = self._upload(device)
        return self._dev[str(device)]

    def sub(self, lo, hi):
        """-> (the batch of the recordings lo .. hi - 1 re-based at 0, its first row r0, one past its last row r1); all of them: the
        batch itself, whose table is already where it was used"""
        r0, r1 = int(self.rec_off[lo]), int(self.rec_off[hi])
        return (self if (lo, hi) == (0, self.R) else RecBatch(self.rec_off[lo:hi + 1] - r0, r1 - r0)), r0, r1

    def chunks(self, cost, budget, max_recs=None):
        """(lo, hi) ranges of consecutive recordings that cover the batch: each grows while cost(lo, hi + 1) <= budget and it holds
        fewer than max_recs recordings; one recording always goes"""
        lo = 0
        while lo < self.R:
            hi, top = lo + 1, self.R if max_recs is None else min(self.R, lo + max_recs)
            while hi < top and cost(lo, hi + 1) <= budget:
                hi += 1
            yield lo, hi
            lo = hi
