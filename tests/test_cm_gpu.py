"""Kaldi's one-byte compressed matrices ('CM ') on the GPU: spk_cm_decode and spk_cm_compress (csrc/cm.hip)
against tests/cm_ref.py bit for bit, and the paths that use them - compute_fbank.py --compress, decode.py --native-reader over a
'CM ' archive, NativeTrainLoader(device="cuda")."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import cm_ref
from oracle import weights as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB = os.path.join(ROOT, "tests", "golden", "fbank")
SPECIAL = [0, 64, 65, 192, 193, 255]            # the ends of the three segments


def _headers(B, F, rng, variant):
    """(minrange [B, 2], hdr [B, F, 4] uint16): random increasing points, one forced-degenerate header (p, p+1, p+2, p+3) and one
    full-range header (0 .. 65535), at the first and the last row (swapped in variant 1)"""
    mr = np.stack([rng.normal(0, 5, B), np.exp(rng.normal(2, 1, B))], axis=1).astype(np.float32)
    hdr = np.sort(rng.integers(0, 65536, (B, F, 4)), axis=2)
    for k in range(1, 4):
        hdr[:, :, k] = np.maximum(hdr[:, :, k], hdr[:, :, k - 1] + 1)
    hdr = np.minimum(hdr, np.array([65532, 65533, 65534, 65535]))
    p = int(rng.integers(0, 65000))
    special = [np.array([p, p + 1, p + 2, p + 3]), np.array([0, 21845, 43690, 65535])]
    flat = hdr.reshape(B * F, 4)
    flat[0] = special[variant]
    flat[-1] = special[1 - variant] if B * F > 1 else flat[-1]
    return mr, hdr.astype(np.uint16)


@pytest.mark.parametrize("B,F,T,lengths", [(1, 1, 1, [1]), (2, 3, 5, [5, 1]), (3, 23, 203, [203, 64, 17]), (2, 40, 64, None),
                                           (4, 80, 300, None)])
def test_decode_is_bit_equal_to_the_restatement(B, F, T, lengths):
    from pytorch_kaldi_resnet_amd import features
    rng = np.random.default_rng(B * 1000 + T)
    N = B * F * T
    for variant in range(6 if N < 6 else 2):
        mr, hdr = _headers(B, F, rng, variant % 2)
        P = np.stack([cm_ref.uint16_to_float(mr[b, 0], mr[b, 1], hdr[b]) for b in range(B)])           # [B, F, 4]
        np.testing.assert_array_equal(features.column_headers(mr, hdr).view(np.uint32), P.view(np.uint32))
        codes = rng.integers(0, 256, N).astype(np.uint8)
        sp = np.roll(SPECIAL, variant)
        codes[:min(6, N)] = sp[:min(6, N)]
        codes[N - min(6, N):] = sp[::-1][:min(6, N)]
        codes = codes.reshape(B, F, T)
        ref = np.stack([cm_ref.decode_p(P[b], codes[b]).T for b in range(B)])                            # [B, F, T]
        if lengths is not None:
            for b in range(B):
                ref[b, :, lengths[b]:] = 0
        Pd = torch.from_numpy(P).cuda()
        # (code buffer offset, output offset in floats): aligned; the output 4 bytes off a 16-byte boundary; the codes 5 bytes off
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
            assert (guard[:ooff] == 7.0).all() and (guard[ooff + N:] == 7.0).all()          # nothing outside the tensor
    got = features.decompress(torch.from_numpy(codes).cuda(), Pd, None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda())
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _check_compressed(x, T, mr, hdr, codes):
    """the GPU's parts of every row against cm_ref.compress of x[b, :, :T[b]].T, byte for byte"""
    mr, hdr, codes = mr.cpu().numpy(), hdr.cpu().numpy(), codes.cpu().numpy()
    for b in range(x.shape[0]):
        if T[b] == 0:
            assert (mr[b] == 0).all() and (hdr[b] == 0).all() and (codes[b] == 0).all()
            continue
        vmin, vrange, h, c = cm_ref.compress(x[b, :, :T[b]].T)
        assert mr[b, 0].view(np.uint32) == vmin.view(np.uint32) and mr[b, 1].view(np.uint32) == vrange.view(np.uint32), (b, T[b])
        np.testing.assert_array_equal(hdr[b], h.astype(np.int32), err_msg="row %d of %d frames" % (b, T[b]))
        np.testing.assert_array_equal(codes[b, :, :T[b]], c, err_msg="row %d of %d frames" % (b, T[b]))
        assert (codes[b, :, T[b]:] == 0).all()


@pytest.mark.parametrize("kind", cm_ref.KINDS)
def test_compress_is_byte_equal_to_the_restatement(kind):
    """one batch per matrix kind: every row count where the rule changes (1 .. 5), around the quartile ranks (7, 8, 9), more than
    one pass of the workgroup over the row (1000), and an empty row; the padding past T[b] is NaN or +-1e30 and must not matter.
    Tcap = 1003 is odd: the rows start at every alignment."""
    from pytorch_kaldi_resnet_amd import features
    rng = np.random.default_rng(17)
    T = [1, 2, 3, 4, 0, 5, 7, 8, 9, 33, 64, 203, 1000]
    F, Tcap = 7, 1003
    x = np.empty((len(T), F, Tcap), dtype=np.float32)
    for b, t in enumerate(T):
        x[b] = (np.nan, 1e30, -1e30)[b % 3]
        if t:
            x[b, :, :t] = cm_ref.make_matrix(kind, t, F, rng).T
    mr, hdr, codes = features.compress(torch.from_numpy(x).cuda(), T)
    assert mr.shape == (len(T), 2) and hdr.shape == (len(T), F, 4) and codes.shape == (len(T), F, Tcap) and codes.dtype == torch.uint8
    _check_compressed(x, T, mr, hdr, codes)
    # the parts decode (on the GPU) to what the restatement decodes
    back = features.decompress(codes, torch.from_numpy(features.column_headers(mr, hdr)).cuda(), T).cpu().numpy()
    for b, t in enumerate(T):
        if t:
            np.testing.assert_array_equal(back[b, :, :t].T.view(np.uint32), cm_ref.decode(*cm_ref.compress(x[b, :, :t].T)).view(np.uint32))
        assert (back[b, :, t:] == 0).all()


def test_compress_long_rows_unaligned_input_and_refusals():
    from pytorch_kaldi_resnet_amd import features
    rng = np.random.default_rng(23)
    # 20 000 frames: far past anything a workgroup could stage in LDS; the select re-reads the row
    x = np.concatenate([cm_ref.make_matrix("logmel", 20000, 1, rng), cm_ref.make_matrix("ties", 20000, 1, rng)], axis=1).T[None].copy()
    mr, hdr, codes = features.compress(torch.from_numpy(x).cuda(), [20000])
    _check_compressed(x, [20000], mr, hdr, codes)
    # an input that starts 4 bytes off a 16-byte boundary (no 16-byte loads), T < Tcap
    y = np.stack([cm_ref.make_matrix("cmn", 50, 5, rng).T, cm_ref.make_matrix("tight", 50, 5, rng).T])
    base = torch.zeros(2 * 5 * 50 + 4, device="cuda")
    yd = base[1:1 + 500].view(2, 5, 50)
    yd.copy_(torch.from_numpy(y))
    assert yd.data_ptr() % 16 == 4
    mr, hdr, codes = features.compress(yd, torch.tensor([50, 37]))
    _check_compressed(y, [50, 37], mr, hdr, codes)
    # a minimum of zero among zeros of both signs is stored as +0, whichever comes first
    w = np.abs(cm_ref.make_matrix("ties", 40, 3, rng).T)[None].repeat(2, axis=0).copy()
    w[0, 0, 5], w[0, 2, 30], w[1, 0, 5], w[1, 2, 30] = -0.0, 0.0, 0.0, -0.0
    mr, hdr, codes = features.compress(torch.from_numpy(w).cuda(), [40, 40])
    assert (mr[:, 0].cpu().numpy().view(np.uint32) == 0).all()
    _check_compressed(w, [40, 40], mr, hdr, codes)
    # a non-finite value inside T[b] is refused naming the row; past T[b] it is padding
    z = y.copy()
    z[1, 2, 40] = np.inf
    features.compress(torch.from_numpy(z).cuda(), [50, 37])
    with pytest.raises(ValueError, match="row 1"):
        features.compress(torch.from_numpy(z).cuda(), [50, 41])
    z[1, 2, 40] = np.nan
    with pytest.raises(ValueError, match="row 1"):
        features.compress(torch.from_numpy(z).cuda(), [50, 41])
    with pytest.raises(ValueError, match="outside"):
        features.compress(torch.from_numpy(y).cuda(), [50, 51])


def _write_wavs(d, n=6, seed=3):
    """the synthetic wav set of tests/test_frontend_gpu.py (its sixth file is silent: skipped with --egs)"""
    rng = np.random.default_rng(seed)
    x = np.load(os.path.join(FB, "conf16k_f40.npz"))["wave"].astype(np.float64)
    y = np.load(os.path.join(FB, "nosnip_f80.npz"))["wave"].astype(np.float64)
    lines = []
    for i in range(n):
        parts = [x if rng.random() < 0.5 else y for _ in range(int(rng.integers(2, 7)))]
        s = np.concatenate(parts)[: int(rng.integers(16000, 60000))]
        s = np.clip(s + rng.normal(0, 30, s.size), -32768, 32767).astype(np.int16)
        if i == 5:
            s = np.zeros(20000, dtype=np.int16)
        p = os.path.join(d, "u%02d.wav" % i)
        with wave.open(p, "wb") as wf:
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(16000)
            wf.writeframes(s.tobytes())
        lines.append("utt%02d %s\n" % (i, p))
    scp = os.path.join(d, "wav.scp")
    open(scp, "w").writelines(lines)
    return scp


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT
    return env


def test_compute_fbank_compress_writes_readable_archives(tmp_path):
    """compute_fbank.py --compress against the same run without it: the same keys, frame counts and scp lines up to the offsets,
    every record readable by kaldi_io.read_mat and within the round-trip bound of the uncompressed features (per column, step =
    the widest segment step: step / 2 + 4 ulp(M) inside [P0, P100], range / 65535 + 4 ulp(M) outside)"""
    from pytorch_kaldi_resnet_amd import ingest, kaldi_io
    scp = _write_wavs(str(tmp_path))
    cfg = ["--fbank-config", os.path.join(FB, "fbank.conf"), "--vad-config", os.path.join(FB, "vad.conf"), "--egs", "--cmn-window",
           "300", "--batch-size", "4", "--seed", "5"]
    outs = []
    for name, extra in (("fm", []), ("cm", ["--compress"])):
        out = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "compute_fbank.py"), scp, out] + cfg + extra, env=_env(),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "utt05" in r.stdout and "no voiced frames" in r.stdout
        outs.append(out)
    fm, cm = outs
    assert open(os.path.join(fm, "utt2num_frames")).read() == open(os.path.join(cm, "utt2num_frames")).read()
    a = [l.split() for l in open(os.path.join(fm, "feats.scp"))]
    b = [l.split() for l in open(os.path.join(cm, "feats.scp"))]
    assert [k for k, _ in a] == [k for k, _ in b] == ["utt%02d" % i for i in range(5)]
    assert all(os.path.basename(r.rsplit(":", 1)[0]) == "feats.ark" for _, r in a + b)
    assert os.path.getsize(os.path.join(cm, "feats.ark")) < 0.3 * os.path.getsize(os.path.join(fm, "feats.ark"))
    raw = open(os.path.join(cm, "feats.ark"), "rb").read()
    tab = ingest.ArkTable([r for _, r in b])
    assert tab.all_cm
    for (k, ra), (_, rb) in zip(a, b):
        m, c = kaldi_io.read_mat(ra), kaldi_io.read_mat(rb)
        vmin, vrange, hdr, codes = cm_ref.parse_record(raw, int(rb.rsplit(":", 1)[1]))
        assert c.shape == m.shape == (codes.shape[1], codes.shape[0]) and m.shape[1] == 40
        # the record is what the restatement makes of the uncompressed features
        assert cm_ref.record(*cm_ref.compress(m)) == cm_ref.record(vmin, vrange, hdr, codes), k
        P = cm_ref.uint16_to_float(vmin, vrange, hdr).astype(np.float64)
        ulp = cm_ref.ulp_of_matrix(vmin, vrange)
        err = np.abs(c.astype(np.float64) - m.astype(np.float64))
        inside = (m >= P[:, 0][None, :]) & (m <= P[:, 3][None, :])
        bound = np.where(inside, cm_ref.segment_steps(P)[None, :] / 2, float(vrange) / 65535.0) + 4 * ulp
        assert (err <= bound).all(), (k, float((err / bound).max()))


def _feature_archives(tmp_path, n=8, F=40):
    """a 'CM ' archive of n utterances of 40 .. 90 frames (two pairs of equal length) and an 'FM ' archive of the decoded values"""
    from pytorch_kaldi_resnet_amd import kaldi_io
    rng = np.random.default_rng(29)
    lens = [int(v) for v in rng.integers(40, 91, n)]
    lens[1], lens[5] = lens[0], lens[4]
    cm, fm = str(tmp_path / "cm.ark"), str(tmp_path / "fm.ark")
    lc, lf, u2s = [], [], []
    with open(cm, "wb") as fc, open(fm, "wb") as ff:
        for i, t in enumerate(lens):
            parts = cm_ref.compress(cm_ref.make_matrix(("logmel", "cmn")[i % 2], t, F, rng))
            off = kaldi_io.write_cm(fc, *parts, key="u%d" % i)
            lc.append("u%d %s:%d\n" % (i, cm, off))
            off = kaldi_io.write_mat(ff, cm_ref.decode(*parts), key="u%d" % i)
            lf.append("u%d %s:%d\n" % (i, fm, off))
            u2s.append("u%d %d\n" % (i, i % 3))
    open(str(tmp_path / "cm.scp"), "w").writelines(lc)
    open(str(tmp_path / "fm.scp"), "w").writelines(lf)
    open(str(tmp_path / "u2s"), "w").writelines(u2s)
    return str(tmp_path / "cm.scp"), str(tmp_path / "fm.scp"), str(tmp_path / "u2s")


def test_decode_over_a_compressed_archive_writes_identical_embeddings(tmp_path):
    """decode.py --native-reader, with and without --pad-batches, over a 'CM ' archive (codes through the pinned buffer, decoded
    on the GPU with the batch's lengths) against the same command over an 'FM ' archive holding the decoded values: the same
    bytes out"""
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    cm, fm, _ = _feature_archives(tmp_path)
    S, F = 10, 40
    npst = W.make_state(41, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    ckpt = str(tmp_path / "model.pth.tar")
    torch.save({"state_dict": m.state_dict(), "epoch": 1}, ckpt)
    base = [sys.executable, os.path.join(ROOT, "scripts", "decode.py"), "--spk_num", str(S), "--arch", "resnet34", "--input-dim",
            str(F), "--pooling", "mean+std", "--model-path", ckpt, "--batch-size", "4", "--native-reader"]
    for mode in (["--pad-batches"], []):
        outs = []
        for name, scp in (("cm", cm), ("fm", fm)):
            out = str(tmp_path / (name + ("_pad" if mode else "")))
            r = subprocess.run(base + mode + ["--decode-scp", scp, "--out-path", out], env=_env(), capture_output=True, text=True,
                               timeout=300)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            outs.append(open(os.path.join(out, "alone"), "rb").read())
        assert outs[0] == outs[1] and outs[0].count(b"\n") == 8


def test_train_loader_on_the_device_yields_the_host_paths_tensors(tmp_path):
    """NativeTrainLoader(device="cuda") over a 'CM ' corpus - byte ring, copy and spk_cm_decode on the copy stream - against
    device=None (decoded by the reader threads): the same tensors bit for bit, over 2 epochs of 4 batches with prefetch=1 (3 ring
    slots: every slot is refilled)"""
    from pytorch_kaldi_resnet_amd import ingest
    cm, _, u2s = _feature_archives(tmp_path)
    host = ingest.NativeTrainLoader(cm, u2s, 32, batch_size=2, seed=4, prefetch=1)
    dev = ingest.NativeTrainLoader(cm, u2s, 32, batch_size=2, seed=4, prefetch=1, device="cuda")
    assert dev.table.all_cm and len(host) == 4
    for epoch in range(2):
        host.set_epoch(epoch)
        dev.set_epoch(epoch)
        n = 0
        for (xh, yh), (xd, yd) in zip(host, dev):
            assert xd.is_cuda and xd.dtype == torch.float32 and xd.shape == xh.shape == (2, 40, 32)
            np.testing.assert_array_equal(xd.cpu().numpy().view(np.uint32), xh.numpy().view(np.uint32))
            assert torch.equal(yd.cpu(), yh)
            n += 1
        assert n == 4
