"""Independent numpy restatement of Kaldi's compressed matrix ('CM ', one byte per value) - DESIGN.md section 6g - the
counterpart of tests/resample_ref.py for csrc/cm.hip and the 'CM ' paths of libspkio.

Everything is float32 and every operation is rounded on its own (numpy never fuses a multiply with an add), in the order the
kernels and the host reader use:
    U(u)   = min + (range * 1.52590218966964e-05f) * (float)u
    decode : c <= 64: P0 + (P25 - P0) * c * (1/64.f);  c <= 192: P25 + (P75 - P25) * (c - 64) * (1/128.f);
             else P75 + (P100 - P75) * (c - 192) * (1/63.f)
compress() takes a [rows, cols] matrix of finite values and returns the parts of a record; decode() takes them back."""
import struct

import numpy as np

f32 = np.float32
INV65535 = f32(1.52590218966964e-05)


def uint16_to_float(vmin, vrange, u):
    """U(u): the value a 16-bit header entry stands for"""
    scale = f32(vrange) * INV65535
    return (f32(vmin) + (scale * np.asarray(u).astype(f32)).astype(f32)).astype(f32)


def decode(vmin, vrange, hdr, codes):
    """hdr [cols, 4] uint16, codes [cols, rows] uint8 (the payload as stored) -> [rows, cols] float32"""
    P = uint16_to_float(vmin, vrange, hdr)                    # [cols, 4]
    return decode_p(P, codes)


def decode_p(P, codes):
    """decode with the column headers already converted: P [cols, 4] float32"""
    P = np.asarray(P, dtype=f32)
    c = np.asarray(codes).astype(f32)
    p0, p25, p75, p100 = (P[:, i:i + 1] for i in range(4))
    lo = (p0 + (((p25 - p0).astype(f32) * c).astype(f32) * f32(1 / 64.0)).astype(f32)).astype(f32)
    mid = (p25 + (((p75 - p25).astype(f32) * (c - f32(64)).astype(f32)).astype(f32) * f32(1 / 128.0)).astype(f32)).astype(f32)
    hi = (p75 + (((p100 - p75).astype(f32) * (c - f32(192)).astype(f32)).astype(f32) * f32(1 / 63.0)).astype(f32)).astype(f32)
    out = np.where(c <= 64, lo, np.where(c <= 192, mid, hi)).astype(f32)
    return np.ascontiguousarray(out.T)


def _q(v, vmin, vrange):
    """Q(v) = (int)(clamp((v - min) / range, 0, 1) * 65535 + 0.499f)"""
    with np.errstate(all="ignore"):
        f = ((np.asarray(v, dtype=f32) - vmin).astype(f32) / vrange).astype(f32)
    f = np.minimum(np.maximum(f, f32(0)), f32(1))
    return ((f * f32(65535)).astype(f32) + f32(0.499)).astype(f32).astype(np.int64)


def _clamp_trunc(f, lo, hi):
    """clamp the float to [lo, hi] first (NaN -> lo), then truncate"""
    f = np.where(f >= f32(lo), np.where(f <= f32(hi), f, f32(hi)), f32(lo)).astype(f32)
    return f.astype(np.int64)


def compress(m):
    """m [rows, cols] finite float32 -> (min, range, hdr [cols, 4] uint16, codes [cols, rows] uint8)"""
    m = np.asarray(m, dtype=f32)
    rows, cols = m.shape
    assert rows >= 1 and cols >= 1 and np.isfinite(m).all()
    vmin, vmax = f32(m.min()), f32(m.max())
    if vmin == 0:
        vmin = f32(0.0)               # a minimum of zero is stored as +0: which of -0 / +0 a reduction returns depends on its order
    if vmax == vmin:
        vmax = f32(vmin + f32(f32(1) + np.abs(vmin)))
    vrange = f32(vmax - vmin)
    s = np.sort(m, axis=0)                                    # a selection is enough; the reference sorts
    if rows >= 5:
        q = rows // 4
        r25, r75, r100 = q, 3 * q, rows - 1
    else:
        r25, r75, r100 = 1, 2, 3
    hdr = np.zeros((cols, 4), dtype=np.int64)
    hdr[:, 0] = np.minimum(_q(s[0], vmin, vrange), 65532)
    hdr[:, 1] = np.minimum(np.maximum(_q(s[r25], vmin, vrange), hdr[:, 0] + 1), 65533) if r25 < rows else hdr[:, 0] + 1
    hdr[:, 2] = np.minimum(np.maximum(_q(s[r75], vmin, vrange), hdr[:, 1] + 1), 65534) if r75 < rows else hdr[:, 1] + 1
    hdr[:, 3] = np.maximum(_q(s[r100], vmin, vrange), hdr[:, 2] + 1) if r100 < rows else hdr[:, 2] + 1
    hdr = hdr.astype(np.uint16)
    P = uint16_to_float(vmin, vrange, hdr)
    p0, p25, p75, p100 = (P[:, i:i + 1] for i in range(4))
    v = m.T                                                   # [cols, rows]
    with np.errstate(all="ignore"):
        lo = ((((v - p0).astype(f32) / (p25 - p0).astype(f32)).astype(f32) * f32(64)).astype(f32) + f32(0.5)).astype(f32)
        mid = ((((v - p25).astype(f32) / (p75 - p25).astype(f32)).astype(f32) * f32(128)).astype(f32) + f32(0.5)).astype(f32)
        hi = ((((v - p75).astype(f32) / (p100 - p75).astype(f32)).astype(f32) * f32(63)).astype(f32) + f32(0.5)).astype(f32)
    codes = np.where(v < p25, _clamp_trunc(lo, 0, 64),
                     np.where(v < p75, 64 + _clamp_trunc(mid, 0, 128), 192 + _clamp_trunc(hi, 0, 63)))
    return vmin, vrange, hdr, np.ascontiguousarray(codes.astype(np.uint8))


def record(vmin, vrange, hdr, codes):
    """the bytes of one record from the \\0B flag on"""
    cols, rows = codes.shape
    return (b"\0BCM " + struct.pack("<ffii", float(vmin), float(vrange), rows, cols)
            + np.ascontiguousarray(hdr, dtype="<u2").tobytes() + np.ascontiguousarray(codes, dtype=np.uint8).tobytes())


def parse_record(raw, off):
    """(min, range, hdr [cols, 4] uint16, codes [cols, rows] uint8) of the 'CM ' record whose \\0B flag is at raw[off]"""
    assert raw[off:off + 5] == b"\0BCM "
    vmin, vrange = np.frombuffer(raw[off + 5:off + 13], dtype="<f4")
    rows, cols = struct.unpack("<ii", raw[off + 13:off + 21])
    hdr = np.frombuffer(raw[off + 21:off + 21 + cols * 8], dtype="<u2").reshape(cols, 4)
    codes = np.frombuffer(raw[off + 21 + cols * 8:off + 21 + cols * 8 + cols * rows], dtype=np.uint8).reshape(cols, rows)
    return vmin, vrange, hdr, codes


def ulp_of_matrix(vmin, vrange):
    """ulp(M), M = max(|min|, |min + range|)"""
    return float(np.spacing(np.float32(max(abs(np.float32(vmin)), abs(np.float32(vmin) + np.float32(vrange))))))


def segment_steps(P):
    """per column the widest of the three segment steps of the decoded headers P [cols, 4] (float64)"""
    P = np.asarray(P, dtype=np.float64)
    return np.maximum(np.maximum((P[:, 1] - P[:, 0]) / 64.0, (P[:, 2] - P[:, 1]) / 128.0), (P[:, 3] - P[:, 2]) / 63.0)


# ---- the matrix kinds of the tests (tests/golden/cm, tests/test_cm_cpu.py, tests/test_cm_gpu.py) ----
KINDS = ("logmel", "cmn", "ties", "const", "constcol", "tight")


def make_matrix(kind, rows, cols, rng):
    """[rows, cols] float32.  logmel: N(8, 3^2); cmn: zero-mean with a 50x spread of the per-bin scale; ties: integer-rounded
    values; const: one value everywhere (max == min); constcol: a constant column inside a varying matrix; tight: N(20, 1e-3^2)
    with a constant first column: the range is so far below the offset that neighbouring 16-bit points decode to the same float,
    and the forced points of the constant column (and of the ranks that fewer than 5 rows lack) make zero-width segments."""
    if kind == "logmel":
        m = rng.normal(8.0, 3.0, (rows, cols))
    elif kind == "cmn":
        m = rng.normal(0.0, 1.0, (rows, cols)) * np.geomspace(0.1, 5.0, cols)[None, :]
    elif kind == "ties":
        m = np.round(rng.normal(8.0, 3.0, (rows, cols)))
    elif kind == "const":
        m = np.full((rows, cols), -3.25)
    elif kind == "constcol":
        m = rng.normal(8.0, 3.0, (rows, cols))
        m[:, cols // 2] = 7.5
    elif kind == "tight":
        m = rng.normal(20.0, 1e-3, (rows, cols))
        m[:, 0] = m[0, 0]             # a constant column: its points are forced to p, p + 1, p + 2, p + 3
    else:
        raise ValueError(kind)
    return m.astype(f32)
