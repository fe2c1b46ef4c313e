"""Kaldi's one-byte compressed matrices ('CM ') on the host: the fixture written by tools/make_cm_golden.py
against the reference reader's output, the Python reader against tests/cm_ref.py, and libspkio's probe, float readers and code
readers against both."""
import io
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

import pytorch_kaldi_resnet_amd  # noqa: F401
from pytorch_kaldi_resnet_amd import hip, ingest, kaldi_io

import cm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cm")
ARK = os.path.join(GOLD, "cases.ark")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))
RAW = open(ARK, "rb").read()


parse_record = cm_ref.parse_record


ulp_of_matrix = cm_ref.ulp_of_matrix


def rx(c):
    return "%s:%d" % (ARK, c["offset"])


def test_fixture_decodes_to_the_reference_readers_arrays():
    """Both decoders of this project against what the reference's scripts/kaldi_io.py returned for the same records
    (expected.npz).  The reference divides a segment's width by 64 / 128 / 63 before it multiplies by the code, Kaldi and this
    project multiply first: at most three float32 roundings of intermediates no larger than 2M apart, bound 8 ulp(M) with
    M = max(|min|, |min + range|) of the matrix.  Largest difference seen over the fixture: 3.0 ulp(M) (cmn_203x40)."""
    exp = np.load(os.path.join(GOLD, "expected.npz"))
    assert len(CASES) >= 20 and {c["kind"] for c in CASES} == set(cm_ref.KINDS)
    worst = 0.0
    for c in CASES:
        parts = parse_record(RAW, c["offset"])
        ulp = ulp_of_matrix(parts[0], parts[1])
        e = exp[c["key"]]
        assert e.shape == (c["rows"], c["cols"]) and e.dtype == np.float32
        for got in (kaldi_io.read_mat(rx(c)), cm_ref.decode(*parts)):
            assert got.shape == e.shape and got.dtype == np.float32
            d = float(np.abs(got.astype(np.float64) - e.astype(np.float64)).max()) / ulp
            worst = max(worst, d)
            assert d <= 8.0, (c["key"], d)
    print("largest difference to the reference reader: %.2f ulp(M)" % worst)


def test_python_reader_and_cm_ref_agree_bit_for_bit():
    rng = np.random.default_rng(5)
    for c in CASES:
        np.testing.assert_array_equal(kaldi_io.read_mat(rx(c)).view(np.uint32), cm_ref.decode(*parse_record(RAW, c["offset"])).view(np.uint32))
    # and over ranges whose 16-bit scale rounds differently in float32 and in float64 (the scale is a float32 product)
    for i in range(40):
        m = (cm_ref.make_matrix(cm_ref.KINDS[i % 6], 7 + i, 5, rng) * np.float32(np.exp(rng.normal(0, 3)))).astype(np.float32)
        parts = cm_ref.compress(m)
        got = kaldi_io.read_mat(io.BytesIO(cm_ref.record(*parts)))
        np.testing.assert_array_equal(got.view(np.uint32), cm_ref.decode(*parts).view(np.uint32))


def _mixed_corpus(tmp_path, F=23, n=12, compressed="alternate", lo=30, hi=50):
    """ark of n utterances of lo..hi-1 frames x F, 'CM ' / 'FM ' alternating (or all of one kind); returns (scp path, utt2spk path,
    the rxfilenames, the kinds, the matrices as kaldi_io.read_mat decodes them)"""
    rng = np.random.default_rng(11)
    ark = str(tmp_path / "m.ark")
    rxs, kinds, scp, u2s = [], [], [], []
    with open(ark, "wb") as f:
        for i in range(n):
            m = cm_ref.make_matrix(("logmel", "cmn", "ties")[i % 3], int(rng.integers(lo, hi)), F, rng)
            cm = compressed == "all" or (compressed == "alternate" and i % 2 == 0)
            if cm:
                vmin, vrange, hdr, codes = cm_ref.compress(m)
                off = kaldi_io.write_cm(f, vmin, vrange, hdr, codes, key="u%d" % i)
            else:
                off = kaldi_io.write_mat(f, m, key="u%d" % i)
            rxs.append("%s:%d" % (ark, off))
            kinds.append(ingest.KIND_CM if cm else ingest.KIND_FM)
            scp.append("u%d %s:%d" % (i, ark, off))
            u2s.append("u%d %d" % (i, i % 3))
    open(str(tmp_path / "m.scp"), "w").write("\n".join(scp) + "\n")
    open(str(tmp_path / "u2s"), "w").write("\n".join(u2s) + "\n")
    return str(tmp_path / "m.scp"), str(tmp_path / "u2s"), rxs, kinds, [kaldi_io.read_mat(r) for r in rxs]


def test_write_cm_writes_the_record_cm_ref_describes(tmp_path):
    m = cm_ref.make_matrix("logmel", 33, 5, np.random.default_rng(2))
    parts = cm_ref.compress(m)
    p = str(tmp_path / "one.ark")
    with open(p, "wb") as f:
        off = kaldi_io.write_cm(f, *parts, key="k")
    raw = open(p, "rb").read()
    assert raw[:2] == b"k " and off == 2 and raw[2:] == cm_ref.record(*parts)
    with pytest.raises(TypeError):
        kaldi_io.write_cm(str(tmp_path / "x.ark"), parts[0], parts[1], parts[2], parts[3].astype(np.int32))


def test_probe_reports_rows_cols_and_kind(tmp_path):
    tab = ingest.ArkTable([rx(c) for c in CASES])
    assert [int(v) for v in tab.rows] == [c["rows"] for c in CASES] and [int(v) for v in tab.cols] == [c["cols"] for c in CASES]
    assert (tab.kind == ingest.KIND_CM).all() and tab.all_cm
    assert [int(v) for v in tab.data_off] == [c["offset"] + 21 for c in CASES]
    _, _, rxs, kinds, mats = _mixed_corpus(tmp_path)
    mixed = ingest.ArkTable(rxs)
    assert [int(k) for k in mixed.kind] == kinds and not mixed.all_cm
    assert [int(r) for r in mixed.rows] == [m.shape[0] for m in mats] and (mixed.cols == 23).all()
    fm = ingest.ArkTable([r for r, k in zip(rxs, kinds) if k == ingest.KIND_FM])
    assert (fm.kind == ingest.KIND_FM).all() and not fm.all_cm


@pytest.mark.parametrize("threads", [1, 3])
def test_float_readers_equal_the_python_reader_bit_for_bit(tmp_path, threads):
    """read_crop / read_padded with a float32 out over 'CM ' records (and 'FM ' mixed in): kaldi_io.read_mat(rx)[s:s+T].T, starts
    0, 1, rows - T and T in {1, 20, rows}"""
    tab = ingest.ArkTable([rx(c) for c in CASES])
    for i, c in enumerate(CASES):
        ref = kaldi_io.read_mat(rx(c))
        rows, F = c["rows"], c["cols"]
        for T in sorted({1, 20, rows}):
            if T > rows:
                continue
            for s in sorted({0, 1, rows - T}):
                if s + T > rows:
                    continue
                out = torch.full((1, F, T), 7.0)
                tab.read_crop(np.array([i]), [s], T, out, nthreads=threads)
                np.testing.assert_array_equal(out[0].numpy().view(np.uint32), np.ascontiguousarray(ref[s:s + T].T).view(np.uint32))
        out = torch.full((1, F, rows + 3), 7.0)
        tab.read_padded(np.array([i]), rows + 3, out, nthreads=threads)
        np.testing.assert_array_equal(out[0, :, :rows].numpy().view(np.uint32), np.ascontiguousarray(ref.T).view(np.uint32))
        assert (out[0, :, rows:] == 0).all()
    # batches of mixed kinds; rows > 4 T takes the strip reads, rows <= 4 T the single read of the span
    _, _, rxs, kinds, mats = _mixed_corpus(tmp_path)
    mixed = ingest.ArkTable(rxs)
    idx = np.arange(len(rxs))
    for T in (1, 7, 20, 30):
        starts = [min((0, 1, m.shape[0] - T)[b % 3], m.shape[0] - T) for b, m in enumerate(mats)]
        out = torch.full((len(idx), 23, T), 7.0)
        mixed.read_crop(idx, starts, T, out, nthreads=threads)
        for b, (m, s) in enumerate(zip(mats, starts)):
            np.testing.assert_array_equal(out[b].numpy().view(np.uint32), np.ascontiguousarray(m[s:s + T].T).view(np.uint32))
    out = torch.full((len(idx), 23, 56), 7.0)
    mixed.read_padded(idx, 56, out, nthreads=threads)
    for b, m in enumerate(mats):
        np.testing.assert_array_equal(out[b, :, :m.shape[0]].numpy().view(np.uint32), np.ascontiguousarray(m.T).view(np.uint32))
        assert (out[b, :, m.shape[0]:] == 0).all()
    with pytest.raises(RuntimeError, match="outside utterance"):
        mixed.read_crop(idx[:1], [int(mixed.rows[0]) - 5], 20, torch.empty(1, 23, 20))


def test_plain_entry_points_find_the_kind_themselves(tmp_path):
    """spk_ark_read_crop / spk_ark_read_padded keep their signatures (no kinds argument) and take 'CM ' entries too"""
    import ctypes
    _, _, rxs, kinds, mats = _mixed_corpus(tmp_path)
    tab = ingest.ArkTable(rxs)
    B, T = len(rxs), 20
    arr = (ctypes.c_char_p * B)(*[tab._cpaths[p].value for p in tab.paths])
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    starts = np.ones(B, dtype=np.int32)
    out = torch.empty(B, 23, T)
    rc = ingest.lib().spk_ark_read_crop(B, arr, tab.data_off.ctypes.data_as(i64p), tab.rows.ctypes.data_as(i32p),
                                        starts.ctypes.data_as(i32p), 23, T, out.data_ptr(), 2)
    assert rc == 0, ingest.lib().spk_io_last_error()
    for b, m in enumerate(mats):
        np.testing.assert_array_equal(out[b].numpy().view(np.uint32), np.ascontiguousarray(m[1:1 + T].T).view(np.uint32))
    out = torch.empty(B, 23, 50)
    rc = ingest.lib().spk_ark_read_padded(B, arr, tab.data_off.ctypes.data_as(i64p), tab.rows.ctypes.data_as(i32p), 23, 50,
                                          out.data_ptr(), 2)
    assert rc == 0, ingest.lib().spk_io_last_error()
    for b, m in enumerate(mats):
        np.testing.assert_array_equal(out[b, :, :m.shape[0]].numpy().view(np.uint32), np.ascontiguousarray(m.T).view(np.uint32))


@pytest.mark.parametrize("threads", [1, 3])
def test_code_readers_return_the_payload_bytes_and_decoded_headers(tmp_path, threads):
    tab = ingest.ArkTable([rx(c) for c in CASES])
    for i, c in enumerate(CASES):
        vmin, vrange, hdr, payload = parse_record(RAW, c["offset"])
        rows, F = c["rows"], c["cols"]
        P = cm_ref.uint16_to_float(vmin, vrange, hdr)
        for T in sorted({1, 20, rows}):
            if T > rows:
                continue
            for s in sorted({0, 1, rows - T}):
                if s + T > rows:
                    continue
                codes, colhdr = torch.full((1, F, T), 9, dtype=torch.uint8), torch.full((1, F, 4), 7.0)
                tab.read_crop_codes(np.array([i]), [s], T, codes, colhdr, nthreads=threads)
                np.testing.assert_array_equal(codes[0].numpy(), payload[:, s:s + T])
                np.testing.assert_array_equal(colhdr[0].numpy().view(np.uint32), P.view(np.uint32))
        codes, colhdr = torch.full((1, F, rows + 5), 9, dtype=torch.uint8), torch.full((1, F, 4), 7.0)
        tab.read_padded_codes(np.array([i]), rows + 5, codes, colhdr, nthreads=threads)
        np.testing.assert_array_equal(codes[0, :, :rows].numpy(), payload)
        assert (codes[0, :, rows:] == 0).all()
        np.testing.assert_array_equal(colhdr[0].numpy().view(np.uint32), P.view(np.uint32))
        # decoding what the code readers return gives the float readers' bits
        np.testing.assert_array_equal(cm_ref.decode_p(colhdr[0].numpy(), codes[0, :, :rows].numpy()).view(np.uint32),
                                      kaldi_io.read_mat(rx(c)).view(np.uint32))
    # a batch, both read strategies (rows <= 4 T: one read of the span; else strips)
    _, _, rxs, kinds, mats = _mixed_corpus(tmp_path, compressed="all")
    allcm = ingest.ArkTable(rxs)
    raw = open(rxs[0].rsplit(":", 1)[0], "rb").read()
    for T in (5, 20):
        starts = [min((0, 1, m.shape[0] - T)[b % 3], m.shape[0] - T) for b, m in enumerate(mats)]
        codes, colhdr = torch.empty(len(rxs), 23, T, dtype=torch.uint8), torch.empty(len(rxs), 23, 4)
        allcm.read_crop_codes(np.arange(len(rxs)), starts, T, codes, colhdr, nthreads=threads)
        for b, r in enumerate(rxs):
            vmin, vrange, hdr, payload = parse_record(raw, int(r.rsplit(":", 1)[1]))
            np.testing.assert_array_equal(codes[b].numpy(), payload[:, starts[b]:starts[b] + T])
            np.testing.assert_array_equal(colhdr[b].numpy().view(np.uint32), cm_ref.uint16_to_float(vmin, vrange, hdr).view(np.uint32))
    # an 'FM ' entry has no codes
    _, _, rxs, kinds, mats = _mixed_corpus(tmp_path)
    mixed = ingest.ArkTable(rxs)
    with pytest.raises(RuntimeError, match="m.ark"):
        mixed.read_crop_codes(np.array([0, 1]), [0, 0], 5, torch.empty(2, 23, 5, dtype=torch.uint8), torch.empty(2, 23, 4))


def test_loader_over_a_compressed_corpus_yields_true_windows(tmp_path):
    """NativeTrainLoader(device=None) over 'CM ' entries: every crop is a window of a decoded utterance (what
    tests/test_ingest_cpu.py::test_loader_semantics checks for 'FM ')"""
    scp, u2s, rxs, kinds, mats = _mixed_corpus(tmp_path, F=12, n=15, compressed="all")
    ld = ingest.NativeTrainLoader(scp, u2s, 16, batch_size=4, seed=1)
    assert ld.table.all_cm
    seen = 0
    for x, y in ld:
        assert x.shape[1:] == (12, 16) and x.dtype == torch.float32 and y.dtype == torch.int64
        for i in range(x.shape[0]):
            w = x[i].numpy().T
            assert any(any(np.array_equal(w, m[s:s + 16]) for s in range(m.shape[0] - 15)) for m in mats)
        seen += x.shape[0]
    assert seen == len(ld.labels)


def test_bad_records_fail_naming_the_file(tmp_path):
    c = next(c for c in CASES if c["key"] == "logmel_33x23")
    rec = RAW[c["offset"]:c["offset"] + 21 + 23 * 8 + 23 * 33]
    cut = str(tmp_path / "cut.ark")
    open(cut, "wb").write(b"k " + rec[:-10])
    with pytest.raises(RuntimeError, match=r"cut\.ark:2.*truncated"):
        ingest.ArkTable([cut + ":2"])
    cut2 = str(tmp_path / "cut2.ark")
    open(cut2, "wb").write(b"k " + rec[:18])              # inside the global header
    with pytest.raises(RuntimeError, match=r"cut2\.ark:2"):
        ingest.ArkTable([cut2 + ":2"])
    neg = str(tmp_path / "neg.ark")
    open(neg, "wb").write(b"k " + rec[:13] + struct.pack("<ii", -4, 23) + rec[21:])
    with pytest.raises(RuntimeError, match=r"neg\.ark:2.*shape"):
        ingest.ArkTable([neg + ":2"])
    cm2 = str(tmp_path / "cm2.ark")
    open(cm2, "wb").write(b"k " + b"\0BCM2" + rec[5:])
    with pytest.raises(RuntimeError, match=r"cm2\.ark:2.*CM2.*unsupported.*float32"):
        ingest.ArkTable([cm2 + ":2"])
    dm = str(tmp_path / "dm.ark")
    with open(dm, "wb") as f:
        off = kaldi_io.write_mat(f, np.zeros((3, 2)), key="k")
    with pytest.raises(RuntimeError, match=r"dm\.ark:2.*DM .*unsupported.*float32"):
        ingest.ArkTable(["%s:%d" % (dm, off)])
    # a file cut after the probe: the readers name it too
    whole = str(tmp_path / "whole.ark")
    open(whole, "wb").write(b"k " + rec)
    tab = ingest.ArkTable([whole + ":2"])
    ingest.lib().spk_ark_close_all()
    open(whole, "wb").write(b"k " + rec[:-100])
    with pytest.raises(RuntimeError, match=r"whole\.ark"):
        tab.read_crop(np.array([0]), [13], 20, torch.empty(1, 23, 20))
    with pytest.raises(RuntimeError, match=r"whole\.ark"):
        tab.read_crop_codes(np.array([0]), [13], 20, torch.empty(1, 23, 20, dtype=torch.uint8), torch.empty(1, 23, 4))
    ingest.lib().spk_ark_close_all()


def test_new_symbols_are_declared_exported_and_bound():
    io_hdr = open(os.path.join(ROOT, "include", "spkio.h")).read()
    for name in ("spk_ark_probe_kinds", "spk_ark_read_crop_kinds", "spk_ark_read_padded_kinds", "spk_ark_read_crop_codes",
                 "spk_ark_read_padded_codes"):
        assert re.search(r"\b%s\s*\(" % name, io_hdr) and hasattr(ingest.lib(), name), name
    assert re.search(r"\bspk_ark_probe\s*\(", io_hdr) and hasattr(ingest.lib(), "spk_ark_probe")      # the old probe stays
    hip_hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    for name in ("spk_cm_decode", "spk_cm_compress"):
        assert re.search(r"\b%s\s*\(" % name, hip_hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
    # argument validation happens on the host before any launch
    assert hip.lib().spk_cm_decode(None, None, None, 1, 1, 1, None, None) < 0 and b"spk_cm_decode" in hip.lib().spk_last_error()
    assert hip.lib().spk_cm_compress(None, None, 1, 1, 1, None, None, None, None, None) < 0


def test_a_zero_minimum_is_stored_as_plus_zero():
    m = np.array([[0.0, 3.0], [-0.0, 1.0], [2.0, 0.0]], dtype=np.float32)
    for mm in (m, m[::-1], -m[:, ::-1] * np.float32(-1)):
        vmin = cm_ref.compress(mm)[0]
        assert vmin.dtype == np.float32 and vmin.view(np.uint32) == 0


def test_round_trip_error_of_the_restatement():
    """compress then decode (tests/cm_ref.py), per column with `step` the widest of its three segment steps: a value inside
    [P0, P100] comes back within step / 2 + 4 ulp(M), a value outside (the 16-bit rounding of the end points, the ranks that
    fewer than 5 rows lack) within range / 65535 + 4 ulp(M).  Largest seen here: 1.059 x step / 2 inside (tight: the steps are a few
    ulp(M) wide), 0.50 x range / 65535 outside."""
    rng = np.random.default_rng(3)
    worst_in, worst_out = 0.0, 0.0
    for kind in cm_ref.KINDS:
        for rows, cols in ((1, 3), (2, 1), (3, 23), (4, 3), (5, 40), (7, 3), (9, 80), (33, 23), (203, 40)):
            m = cm_ref.make_matrix(kind, rows, cols, rng)
            vmin, vrange, hdr, codes = cm_ref.compress(m)
            back = cm_ref.decode(vmin, vrange, hdr, codes).astype(np.float64)
            P = cm_ref.uint16_to_float(vmin, vrange, hdr).astype(np.float64)
            ulp = ulp_of_matrix(vmin, vrange)
            step = cm_ref.segment_steps(P)[None, :]
            err = np.abs(back - m.astype(np.float64))
            inside = (m >= P[:, 0][None, :]) & (m <= P[:, 3][None, :])
            q = float(vrange) / 65535.0
            assert (err[inside] <= (step / 2 + 4 * ulp + 0 * err)[inside]).all(), (kind, rows, cols)
            assert (err[~inside] <= q + 4 * ulp).all(), (kind, rows, cols)
            if inside.any():
                worst_in = max(worst_in, float((err / (step / 2 + 1e-300))[inside].max()))
            if (~inside).any():
                worst_out = max(worst_out, float(err[~inside].max() / q))
    print("round trip: %.3f x step/2 inside, %.3f x range/65535 outside" % (worst_in, worst_out))
