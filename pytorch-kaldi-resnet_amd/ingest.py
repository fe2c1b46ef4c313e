"""Native batch ingest (libspkio): scp/ark -> pinned [B, F, T] staging, cropped at read time.

Same sampling semantics as the reference's SequenceDataset + DataLoader(shuffle / DistributedSampler)
(scripts/datasets.py:10-72, scripts/train_resnet.py:237-247): class-balanced repetition of scp lines, a fresh
permutation per epoch (seeded with the epoch like DistributedSampler.set_epoch), equal shards per rank (padded by
wrap-around), a uniform random crop start per sample.  What changes is the mechanics: one C++ call reads a whole
batch with pread() on a small thread pool, reading only the cropped frames, and transposes them straight into pinned
memory; a background thread keeps the next batch ready while the GPU works on the current one.
"""
import ctypes
import os
import queue
import threading

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libspkio.so")
        if not os.path.exists(path):
            raise RuntimeError("libspkio.so is missing at %s: run `python __graft_entry__.py build`" % path)
        l = ctypes.CDLL(path)
        l.spk_io_last_error.restype = ctypes.c_char_p
        cpp, i64p, i32p = ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        l.spk_ark_probe.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i64p]
        l.spk_ark_read_crop.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_int]
        l.spk_ark_read_padded.argtypes = [ctypes.c_int, cpp, i64p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        l.spk_ark_probe_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i64p, i32p]
        l.spk_ark_read_crop_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_int]
        l.spk_ark_read_padded_kinds.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_int]
        l.spk_ark_read_crop_codes.argtypes = [ctypes.c_int, cpp, i64p, i32p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              ctypes.c_void_p, ctypes.c_int]
        l.spk_ark_read_padded_codes.argtypes = [ctypes.c_int, cpp, i64p, i32p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_int]
        l.spk_wav_probe.argtypes = [ctypes.c_int, cpp, ctypes.c_int, i32p, i64p, i64p]
        l.spk_wav_read_padded.argtypes = [ctypes.c_int, cpp, i64p, i64p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int]
        l.spk_text_vectors_bound.argtypes = [ctypes.c_int, ctypes.c_int, cpp]
        l.spk_text_vectors_bound.restype = ctypes.c_int64
        l.spk_format_text_vectors.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, cpp, ctypes.c_char_p, ctypes.c_int64,
                                              ctypes.c_int]
        l.spk_format_text_vectors.restype = ctypes.c_int64
        _LIB = l
    return _LIB


def format_text_vectors(keys, vecs, nthreads=4):
    """bytes of the text ark 'key [ v0 v1 ... ]\\n' per row of float32 vecs [n][D], every value printed exactly like
    numpy's str(np.float32) (the reference's scripts/decode.py:206 line format), formatted natively on `nthreads` threads."""
    vecs = np.ascontiguousarray(vecs, dtype=np.float32)
    n, D = vecs.shape
    assert len(keys) == n
    arr = (ctypes.c_char_p * n)(*[k.encode() for k in keys])
    cap = lib().spk_text_vectors_bound(n, D, arr)
    buf = ctypes.create_string_buffer(cap)
    w = lib().spk_format_text_vectors(n, D, vecs.ctypes.data, arr, buf, cap, int(nthreads))
    if w < 0:
        raise RuntimeError("spk_format_text_vectors: buffer too small")
    return buf.raw[:w]


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, lib().spk_io_last_error().decode()))


def _split_rx(rx):
    path, off = rx.rsplit(":", 1)
    return path, int(off)


KIND_FM, KIND_CM = 0, 1        # ArkTable.kind: float32 'FM ' / one-byte compressed 'CM ' 


def _i32p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _i64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


class ArkTable:
    """Parsed scp: per line the ark path, the payload offset, the frame count and the kind of the record - float32 'FM ' or
    Kaldi's one-byte compressed 'CM ', mixed freely (headers probed once)."""

    def __init__(self, rxfiles):
        paths, offs = zip(*[_split_rx(r) for r in rxfiles])
        uniq = sorted(set(paths))
        self._cpaths = {p: ctypes.c_char_p(p.encode()) for p in uniq}
        self.paths = list(paths)
        n = len(paths)
        self.rows = np.zeros(n, dtype=np.int32)
        self.cols = np.zeros(n, dtype=np.int32)
        self.data_off = np.zeros(n, dtype=np.int64)
        self.kind = np.zeros(n, dtype=np.int32)
        arr = (ctypes.c_char_p * n)(*[self._cpaths[p].value for p in paths])
        offs = np.asarray(offs, dtype=np.int64)
        _check(lib().spk_ark_probe_kinds(n, arr, _i64p(offs), _i32p(self.rows), _i32p(self.cols), _i64p(self.data_off),
                                         _i32p(self.kind)), "spk_ark_probe_kinds")
        self.all_cm = bool(n > 0 and (self.kind == KIND_CM).all())

    def _batch(self, idx):
        B = len(idx)
        F = int(self.cols[idx[0]])
        assert (self.cols[idx] == F).all()
        arr = (ctypes.c_char_p * B)(*[self._cpaths[self.paths[i]].value for i in idx])
        return (B, F, arr, np.ascontiguousarray(self.data_off[idx]), np.ascontiguousarray(self.rows[idx]),
                np.ascontiguousarray(self.kind[idx]))

    def read_crop(self, idx, starts, T, out, nthreads=4):
        """out: contiguous float32 host tensor [B, F, T] (ideally pinned).  'CM ' entries are decoded on the host, to the bits of
        kaldi_io.read_mat."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, F, T) and out.dtype == torch.float32
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        _check(lib().spk_ark_read_crop_kinds(B, arr, _i64p(doff), _i32p(rows), _i32p(st), _i32p(kind), F, T, out.data_ptr(), nthreads),
               "spk_ark_read_crop")
        return out

    def read_padded(self, idx, T, out, nthreads=4):
        """Whole utterances idx (each of 1..T frames) into a contiguous float32 host tensor out [B, F, T] (ideally pinned), the
        frames past each utterance's length zero-filled; self.rows[idx] are the lengths to pass to predict(x, lengths=...)."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, F, T) and out.dtype == torch.float32
        _check(lib().spk_ark_read_padded_kinds(B, arr, _i64p(doff), _i32p(rows), _i32p(kind), F, T, out.data_ptr(), nthreads),
               "spk_ark_read_padded")
        return out

    def read_crop_codes(self, idx, starts, T, codes, colhdr, nthreads=4):
        """'CM ' entries as stored, for features.decompress (the GPU decode): codes, a contiguous uint8 host tensor [B, F, T]
        (codes[b, f, t]: frame starts[b] + t, bin f), and colhdr, contiguous float32 [B, F, 4], the decoded column headers.  A
        quarter of read_crop's bytes and no transpose; an 'FM ' entry is an error."""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert codes.is_contiguous() and tuple(codes.shape) == (B, F, T) and codes.dtype == torch.uint8
        assert colhdr.is_contiguous() and tuple(colhdr.shape) == (B, F, 4) and colhdr.dtype == torch.float32
        st = np.ascontiguousarray(np.asarray(starts, dtype=np.int32))
        _check(lib().spk_ark_read_crop_codes(B, arr, _i64p(doff), _i32p(rows), _i32p(st), F, T, codes.data_ptr(), colhdr.data_ptr(),
                                             nthreads), "spk_ark_read_crop_codes")
        return codes, colhdr

    def read_padded_codes(self, idx, T, codes, colhdr, nthreads=4):
        """read_crop_codes for whole utterances idx (each of 1..T frames): codes zero past each utterance's length"""
        B, F, arr, doff, rows, kind = self._batch(idx)
        assert codes.is_contiguous() and tuple(codes.shape) == (B, F, T) and codes.dtype == torch.uint8
        assert colhdr.is_contiguous() and tuple(colhdr.shape) == (B, F, 4) and colhdr.dtype == torch.float32
        _check(lib().spk_ark_read_padded_codes(B, arr, _i64p(doff), _i32p(rows), F, T, codes.data_ptr(), colhdr.data_ptr(), nthreads),
               "spk_ark_read_padded_codes")
        return codes, colhdr


class WavTable:
    """Parsed wav.scp entries (file paths; Kaldi pipe entries 'cmd |' are refused): per file the sample count and the offset of the
    samples, probed once.  PCM 16-bit mono only, at `sample_rate` (0: any) - everything else is refused naming the file."""

    def __init__(self, paths, sample_rate=0):
        for p in paths:
            if p.rstrip().endswith("|"):
                raise ValueError("wav.scp pipe entries are not supported: %r" % p)
        self.paths = list(paths)
        n = len(self.paths)
        self._cpaths = [ctypes.c_char_p(p.encode()) for p in self.paths]
        self.rate = np.zeros(n, dtype=np.int32)
        self.nsamp = np.zeros(n, dtype=np.int64)
        self.data_off = np.zeros(n, dtype=np.int64)
        arr = (ctypes.c_char_p * max(n, 1))(*[c.value for c in self._cpaths])
        _check(lib().spk_wav_probe(n, arr, int(sample_rate), self.rate.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   self.nsamp.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                   self.data_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "spk_wav_probe")

    def read_padded(self, idx, Nmax, out, nthreads=4):
        """Files idx into a contiguous float32 host tensor out [B, Nmax] (ideally pinned) at int16 scale, zero past each file's
        sample count self.nsamp[idx] (each <= Nmax)."""
        B = len(idx)
        assert out.is_contiguous() and tuple(out.shape) == (B, Nmax) and out.dtype == torch.float32
        arr = (ctypes.c_char_p * B)(*[self._cpaths[i].value for i in idx])
        doff = np.ascontiguousarray(self.data_off[idx])
        ns = np.ascontiguousarray(self.nsamp[idx])
        _check(lib().spk_wav_read_padded(B, arr, doff.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         ns.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), int(Nmax), out.data_ptr(), nthreads),
               "spk_wav_read_padded")
        return out


def pad_batches(lengths, batch_size, max_pad_ratio=0.1, quantum=8):
    """Length-sorted padded batches for whole-utterance extraction: a list of (indices, T_pad).  Utterances are taken in order of
    length (stable) and a batch grows until it holds batch_size of them or one more would make its padded frames
    len * T_pad exceed (1 + max_pad_ratio) x its real frames; T_pad = the batch's longest utterance rounded up to `quantum`.
    Every index lands in exactly one batch; a batch of one may exceed the ratio by its rounding."""
    L = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if batch_size < 1 or quantum < 1 or max_pad_ratio < 0:
        raise ValueError("pad_batches: batch_size >= 1, quantum >= 1, max_pad_ratio >= 0")
    if L.size and L.min() < 1:
        raise ValueError("pad_batches: every length must be >= 1")
    order = np.argsort(L, kind="stable")
    batches, i, n = [], 0, len(order)
    while i < n:
        j, real = i + 1, int(L[order[i]])
        while j < n and j - i < batch_size:
            t_pad = -(-int(L[order[j]]) // quantum) * quantum
            if (j - i + 1) * t_pad > (1.0 + max_pad_ratio) * (real + int(L[order[j]])):
                break
            real += int(L[order[j]])
            j += 1
        idx = order[i:j]
        batches.append((idx, -(-int(L[idx[-1]]) // quantum) * quantum))
        i = j
    return batches


class NativeTrainLoader:
    """Iterable over (features [B,F,T] pinned, labels [B] int64) batches of one epoch for this rank."""

    def __init__(self, scp_file, utt2spkid_file, chunk_size, batch_size, rank=0, world=1, seed=0, threads=4,
                 drop_last=False, prefetch=2, device=None, chunk_range=None):
        """chunk_range=(lo, hi, quantum): variable-length training - one chunk length per batch from
        datasets.chunk_length_schedule (seeded by (seed, epoch) only: the same length on every rank); chunk_size is then
        ignored and the pinned ring is sized for hi.
        device=None: batches are fresh pageable host tensors (the caller copies them; a copy from pageable memory is
        staged by the runtime before .cuda() returns, so nothing can overwrite it early).
        device=cuda:N: the loader owns a ring of PINNED staging buffers and the host->device copy: it issues the copy on
        its own copy stream (overlapping the previous step's kernels), records an event per ring slot, and the reader
        thread waits for that event before it refills the slot - the training loop never syncs with the host, so
        without this guard the reader could overwrite a slot whose asynchronous copy has not executed yet.  Yields
        device tensors, already ordered after the copy on the consumer's current stream.
        When every entry of the scp is a one-byte compressed 'CM ' matrix the ring holds the codes as they
        lie in the archive (a quarter of the bytes, no transpose) plus the small column headers; both are copied and decoded to
        float32 by spk_cm_decode on the copy stream, ahead of the same event.  With device=None, or 'FM ' entries among them, the
        reader decodes on the host and the batches are float32 as before - the same bits either way."""
        self.device = torch.device(device) if device is not None else None
        utt2spk = {}
        for line in open(utt2spkid_file):
            u, s = line.split()
            utt2spk[u] = int(s)
        count = {}
        for s in utt2spk.values():
            count[s] = count.get(s, 0) + 1
        cap = min(500, int((max(count.values()) + 1) / 2))          # datasets.py:23-24
        rx, lab = [], []
        for line in open(scp_file):
            u, r = line.rstrip().split(None, 1)
            rep = max(1, cap // count[utt2spk[u]])
            rx.extend([r] * rep)
            lab.extend([utt2spk[u]] * rep)
        uniq = sorted(set(rx))
        pos = {r: i for i, r in enumerate(uniq)}
        self.table = ArkTable(uniq)
        self.sample_to_row = np.array([pos[r] for r in rx], dtype=np.int64)
        self.labels = np.array(lab, dtype=np.int64)
        self.chunk_range = tuple(int(v) for v in chunk_range) if chunk_range is not None else None
        self.T = int(chunk_size) if self.chunk_range is None else self.chunk_range[1]
        short = self.table.rows < self.T
        if short.any():
            raise AssertionError("%d utterances are shorter than the chunk size %d (reference: assert len(full_mat) >= seq_len)"
                                 % (int(short.sum()), self.T))
        self.bs, self.rank, self.world, self.seed, self.threads = batch_size, rank, world, seed, threads
        self.drop_last, self.prefetch = drop_last, prefetch
        self.epoch = 0
        print("Totally " + str(len(rx)) + " samples with at most " + str(cap) + " samples for one class")

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _indices(self):
        n = len(self.labels)
        g = np.random.RandomState(self.seed + self.epoch)
        perm = g.permutation(n)
        total = -(-n // self.world) * self.world
        perm = np.concatenate([perm, perm[: total - n]])               # DistributedSampler pads by wrap-around
        return perm[self.rank: total: self.world]

    def __len__(self):
        n = -(-len(self.labels) // self.world)
        return n // self.bs if self.drop_last else -(-n // self.bs)

    def __iter__(self):
        idx = self._indices()
        rng = np.random.RandomState((self.seed + self.epoch) * 7919 + self.rank)
        F = int(self.table.cols[0])
        q = queue.Queue(maxsize=self.prefetch)
        dev = self.device
        nslot = self.prefetch + 2
        as_codes = dev is not None and self.table.all_cm
        if as_codes:
            from . import features
            ring = [torch.empty(self.bs * F * self.T, dtype=torch.uint8).pin_memory() for _ in range(nslot)]
            hring = [torch.empty(self.bs * F * 4).pin_memory() for _ in range(nslot)]
        else:
            ring = [torch.empty(self.bs * F * self.T).pin_memory() for _ in range(nslot)] if dev is not None else None
        copied = [None] * nslot          # per slot: event recorded after the H2D copy that last read the slot
        if self.chunk_range is not None:
            from .datasets import chunk_length_schedule
            lens = chunk_length_schedule(self.chunk_range[0], self.chunk_range[1], self.chunk_range[2], len(self) + 1, self.seed,
                                         self.epoch)
        else:
            lens = None

        def producer():
            try:
                k = 0
                for b0 in range(0, len(idx), self.bs):
                    sel = idx[b0:b0 + self.bs]
                    if len(sel) < self.bs and self.drop_last:
                        break
                    rows = self.sample_to_row[sel]
                    T = self.T if lens is None else int(lens[k])          # one chunk length per batch
                    starts = [int(rng.randint(0, int(self.table.rows[r]) - T + 1)) for r in rows]   # datasets.py:66
                    slot = k % nslot
                    if ring is not None:
                        ev = copied[slot]
                        if ev is not None:
                            ev.synchronize()            # the device has finished reading this pinned buffer
                        buf = ring[slot][:len(sel) * F * T].view(len(sel), F, T)
                    else:
                        buf = torch.empty(len(sel), F, T)
                    if as_codes:
                        buf = (buf, hring[slot][:len(sel) * F * 4].view(len(sel), F, 4))
                        self.table.read_crop_codes(rows, starts, T, buf[0], buf[1], self.threads)
                    else:
                        self.table.read_crop(rows, starts, T, buf, self.threads)
                    q.put((slot, buf, torch.from_numpy(self.labels[sel])))
                    k += 1
                q.put(None)
            except BaseException as e:      # surface reader errors in the training loop
                q.put(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        copy_stream = torch.cuda.Stream(device=dev) if dev is not None else None
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            slot, buf, lab = item
            if dev is None:
                yield buf, lab
                continue
            cur = torch.cuda.current_stream(dev)
            with torch.cuda.stream(copy_stream):
                if as_codes:         # bytes and headers across, then the decode, all before the event below
                    xg = features.decompress(buf[0].to(dev, non_blocking=True), buf[1].to(dev, non_blocking=True))
                else:
                    xg = buf.to(dev, non_blocking=True)
                yg = lab.pin_memory().to(dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            copied[slot] = ev
            cur.wait_event(ev)
            xg.record_stream(cur)
            yg.record_stream(cur)
            yield xg, yg
        th.join()
