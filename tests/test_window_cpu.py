"""Windowed extraction, host side: ingest.plan_windows against the frame-by-frame rule of tests/window_ref.py,
ingest.window_batches, decode.py's parser errors and the two exports of csrc/window.hip in the C ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import window_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = [(8, 8, 8), (8, 8, 3), (8, 4, 1), (8, 3, 5), (8, 11, 2), (1, 1, 1), (40, 7, 40)]


@pytest.fixture(scope="module")
def ingest():
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import ingest
    return ingest


def check_plan(ingest, lengths, W, P, M):
    p = ingest.plan_windows(lengths, W, P, M)
    utt, start, length, skipped = R.brute_plan(lengths, W, P, M)
    assert p.utt.tolist() == utt and p.start.tolist() == start and p.length.tolist() == length, (lengths, W, P, M)
    assert p.skipped.tolist() == skipped
    assert all(a.dtype == np.int64 for a in p)
    return p


@pytest.mark.parametrize("W,P,M", RULES)
def test_plan_matches_the_brute_force(ingest, W, P, M):
    check_plan(ingest, list(range(1, 41)), W, P, M)
    edges = [M - 1, M, W, W + 1] + [k * P + W for k in range(1, 5)] + [k * P + W + 1 for k in range(1, 3)]
    edges = [n for n in edges if n >= 1]
    p = check_plan(ingest, edges, W, P, M)
    assert p.skipped.tolist() == ([0] if M > 1 else [])         # n = M - 1 alone is skipped; n = M is one window of M frames
    at_m = p.utt == edges.index(M)
    assert p.start[at_m].tolist() == [0] and p.length[at_m].tolist() == [M]
    for i, n in enumerate(edges):                               # n = k P + W exactly: k + 1 whole windows, the last ends at n
        if n >= W and (n - W) % P == 0:
            sel = p.utt == i
            assert sel.sum() == (n - W) // P + 1 and (p.length[sel] == W).all() and p.start[sel][-1] + W == n


@pytest.mark.parametrize("W,P,M", RULES)
def test_plan_properties(ingest, W, P, M):
    """With min_window = 1 and period <= window every frame of an utterance of at least `window` frames lies in a window; with a
    larger min_window the rule drops a last window shorter than it, so what stays uncovered is a tail of fewer than min_window
    frames and nothing before it."""
    lengths = np.arange(1, 41)
    p = ingest.plan_windows(lengths, W, P, M)
    for u, n in enumerate(lengths):
        sel = p.utt == u
        s, l = p.start[sel], p.length[sel]
        if n < M:
            assert u in p.skipped and not sel.any()
            continue
        assert sel.any() and (l >= 1).all() and (s + l <= n).all() and (l <= W).all()
        assert (l[1:] >= M).all() and (l[:-1] == W).all()
        # no window is a subset of its predecessor
        assert ((s[1:] + l[1:]) > (s[:-1] + l[:-1])).all() and (s[1:] > s[:-1]).all()
        if P <= W and n >= W and M == 1:
            covered = np.zeros(n, dtype=bool)
            for a, b in zip(s, l):
                covered[a:a + b] = True
            assert covered.all(), (u, n)
        if P <= W and n >= W:          # whatever M: the frames up to the last window's end are covered without a hole
            assert s[0] == 0 and (s[1:] <= s[:-1] + l[:-1]).all()
            assert n - (s[-1] + l[-1]) < max(M, 1)              # what is dropped is a tail shorter than min_window
        if P == W:                     # a partition of [0, last_end)
            assert s.tolist() == np.concatenate([[0], np.cumsum(l)[:-1]]).tolist()


def test_plan_empty_and_all_skipped(ingest):
    p = ingest.plan_windows([], 8, 4, 2)
    assert all(a.size == 0 for a in p)
    p = ingest.plan_windows([3, 1, 7, 0], 8, 8, 8)
    assert p.utt.size == 0 and p.start.size == 0 and p.length.size == 0 and p.skipped.tolist() == [0, 1, 2, 3]


def test_plan_refuses_bad_rules(ingest):
    for W, P, M in [(0, 1, 1), (8, 0, 1), (8, 8, 0), (8, 8, 9)]:
        with pytest.raises(ValueError):
            ingest.plan_windows([10], W, P, M)
    with pytest.raises(ValueError):
        ingest.plan_windows([10, -1], 8, 8, 1)


@pytest.mark.parametrize("bs", [1, 5, 64])
def test_window_batches(ingest, bs):
    rng = np.random.RandomState(3)
    p = ingest.plan_windows(rng.randint(1, 400, size=50), 24, 8, 3)
    batches = ingest.window_batches(p.length, bs)
    order = np.concatenate([idx for idx, _ in batches])
    assert sorted(order.tolist()) == list(range(p.utt.size))                 # every row once
    for idx, wcap in batches:
        l = p.length[idx]
        assert 1 <= len(idx) <= bs and wcap % 8 == 0 and wcap - 8 < l.max() <= wcap
        if len(idx) > 1:
            assert len(idx) * wcap <= 1.1 * l.sum()
    inv = np.empty(order.size, dtype=np.int64)
    inv[order] = np.arange(order.size)
    assert (order[inv] == np.arange(order.size)).all()                       # plan order is recoverable
    assert ingest.window_batches(p.length[:0], bs) == []


def _decode(*flags):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--arch", "resnet18", "--input-dim", "40", "--pooling", "mean+std"]
    return subprocess.run(cmd + list(flags), env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("flags,words", [
    (["--window", "24"], ["--window", "--native-reader", "--pad-batches", "--wav-scp"]),
    (["--native-reader", "--window", "24"], ["--window", "--pad-batches"]),
    (["--native-reader", "--pad-batches", "--window", "24", "--chunk-size", "100"], ["--window", "--chunk-size"]),
    (["--native-reader", "--pad-batches", "--window", "24", "--min-window", "25"], ["--min-window", "--window"]),
    (["--native-reader", "--pad-batches", "--window", "24", "--period", "0"], ["--period"]),
    (["--native-reader", "--pad-batches", "--period", "4"], ["--period", "--window"]),
    (["--native-reader", "--pad-batches", "--average-windows"], ["--average-windows", "--window"]),
])
def test_decode_parser_errors(flags, words):
    r = _decode(*flags)
    assert r.returncode == 2, r.stdout[-1000:] + r.stderr[-1000:]
    assert "error:" in r.stderr and all(w in r.stderr for w in words), r.stderr


def test_decode_help_names_the_frames_the_model_sees():
    r = _decode("--help")
    assert r.returncode == 0
    text = " ".join(r.stdout.split())
    assert "--window" in text and "--frame-shift" in text and "after the VAD's frame selection" in text


def test_exports_are_declared_bound_and_exported():
    from helpers import header_params
    from pytorch_kaldi_resnet_amd import hip
    names = ["spk_window_gather", "spk_window_mean"]
    hdr = open(os.path.join(ROOT, "include", "spkhip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in hip.exported_symbols() and hasattr(hip.lib(), name), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        assert len(header_params(name)) == len(hip._SIGS[name]), name


def test_plans_are_refused_on_the_host_before_any_launch():
    """the argument checks need no device: with every device pointer NULL a good plan gets as far as the pointer check"""
    from pytorch_kaldi_resnet_amd import hip
    lib = hip.lib()
    ip = ctypes.POINTER(ctypes.c_int)

    def gather(row, start, length, Wcap=8, B=3, T=37):
        a = [np.asarray(v, dtype=np.int32) for v in (row, start, length)]
        rc = lib.spk_window_gather(None, B, 5, T, a[0].ctypes.data_as(ip), a[1].ctypes.data_as(ip), a[2].ctypes.data_as(ip), None, None,
                                   len(row), Wcap, None)
        return rc, lib.spk_last_error().decode()

    for plan, word in [(([3], [0], [4]), "row"), (([-1], [0], [4]), "row"), (([0], [-1], [4]), "start"), (([0], [0], [0]), "len"),
                       (([0], [34], [4]), "> T"), (([0], [0], [9]), "Wcap"), (([0, 1, 2], [0, 0, 30], [8, 8, 8]), "window 2")]:
        rc, msg = gather(*plan)
        assert rc < 0 and word in msg, (plan, msg)
    rc, msg = gather([0, 2], [0, 33], [8, 4])
    assert rc < 0 and "null device pointer" in msg

    def mean(seg_off, N):
        so = np.asarray(seg_off, dtype=np.int32)
        rc = lib.spk_window_mean(None, N, 4, so.ctypes.data_as(ip), None, None, None, len(seg_off) - 1, None)
        return rc, lib.spk_last_error().decode()

    for so, N, word in [([0, 2, 2, 5], 5, "empty"), ([1, 2, 5], 5, "seg_off"), ([0, 2, 4], 5, "seg_off"), ([0, 3, 2, 5], 5, "empty")]:
        rc, msg = mean(so, N)
        assert rc < 0 and word in msg, (so, msg)
    rc, msg = mean([0, 2, 5], 5)
    assert rc < 0 and "null device pointer" in msg
