#!/usr/bin/env python3
"""Extraction from audio: decode.py --wav-scp's path (WAV read, GPU fbank + sliding CMN + VAD selection, length-masked predict)
against the precomputed-features path (decode.py --native-reader --pad-batches on the archives the front end wrote), in ONE GPU
process, plus the front-end kernels alone at batch 512 x 3 s.

A seeded synthetic WAV set (--n utterances of 2-20 s, harmonic bursts with noise, written with the stdlib `wave`) is made in a
temporary directory.  Each pass runs sequentially over length-sorted batches, timed with a host clock around work that ends in a
device synchronise; after a warm-up of both paths each is timed twice.  The kernel-only leg times Frontend on a resident batch of
512 x 3 s with CUDA events (fbank alone with and without dither, and fbank + VAD + CMN + selection) and predict on its
output.  --input-rate R synthesises the WAVs at R Hz and extracts them as decode.py --wav-scp --allow-downsample / --allow-upsample
does (one resampling launch per batch in front of the fbank; the kernel-only leg then times the resampler too).  Prints one JSON line.
usage: python tools/wav_extract_bench.py [--n 2000] [--batch-size 64] [--input-rate 44100] [--out FILE]
"""
import argparse
import dataclasses
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(rng, n, rate=16000):
    t = np.arange(n) / float(rate)
    f0 = rng.uniform(90, 220) * (1 + 0.1 * np.sin(2 * np.pi * rng.uniform(0.5, 2) * t))
    ph = 2 * np.pi * np.cumsum(f0) / float(rate)
    x = sum((0.5 / h) * np.sin(h * ph) for h in range(1, 8))
    env = (np.sin(2 * np.pi * rng.uniform(1, 3) * t + rng.uniform(0, 6)) > -0.3)
    return np.clip(2500 * x * env + rng.normal(0, 100, n), -32768, 32767).astype(np.int16)


def make_wavs(d, n, seed, rate=16000):
    rng = np.random.default_rng(seed)
    secs = rng.uniform(2.0, 20.0, n)
    keys, paths = [], []
    for i, s in enumerate(secs):
        p = os.path.join(d, "u%05d.wav" % i)
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(rate)
            w.writeframes(synth(rng, int(s * rate), rate).tobytes())
        keys.append("u%05d" % i)
        paths.append(p)
    return keys, paths, secs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--input-rate", type=int, default=16000, help="sample rate of the synthesised WAVs (resampled to 16 kHz on the GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "wav_extract_bench needs a GPU"
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from oracle import weights as W
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io, ops
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    F, S = 40, 1211
    npst = W.make_state(3, S, F, "mean+std", "AAM", "resnet34")
    m = NeuralSpeakerModel(S, F, "mean+std", "AAM", 0.2, 30)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in npst.items()})
    m = m.cuda().eval()
    fb = features.FbankOptions(num_mel_bins=F, high_freq=7600, snip_edges=False)     # the recipe's conf/fbank.conf
    vo = features.VadOptions(5.5, 0.5, 2, 0.12)                                        # conf/vad.conf
    cmn = features.CmnOptions(cmn_window=300)
    rate = args.input_rate
    fe = features.Frontend(fb, vo, cmn, input_rate=rate)
    with tempfile.TemporaryDirectory() as d, torch.no_grad():
        keys, paths, secs = make_wavs(d, args.n, args.seed, rate)
        table = ingest.WavTable(paths, rate)
        wb = [(b, int(nm)) for b, nm in ingest.pad_batches(table.nsamp, args.batch_size, quantum=1)]
        ids = np.array([features.utt_id(k) for k in keys], dtype=np.int64)

        def wav_pass():
            out = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b, nmax in wb:
                buf = torch.empty(len(b), nmax).pin_memory()
                table.read_padded(b, nmax, buf)
                x, L = fe(buf.cuda(non_blocking=True), table.nsamp[b], ids[b], 0)
                e = m.predict(x, lengths=L).cpu().numpy()
                for j, i in enumerate(b):
                    out[int(i)] = (e[j], x[j, :, :L[j]].T.cpu().numpy() if feats_out is not None else None)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        feats_out = {}
        _, first = wav_pass()                   # warm-up, and the features of the precomputed path
        ark = os.path.join(d, "feats.ark")
        rx = []
        with open(ark, "wb") as f:
            for i in range(args.n):
                f.write(keys[i].encode() + b" ")
                off = kaldi_io.write_mat(f, np.ascontiguousarray(first[i][1]))
                rx.append("%s:%d" % (ark, off))
        feats_out = None
        atab = ingest.ArkTable(rx)
        fbat = ingest.pad_batches(atab.rows, args.batch_size)

        def feat_pass():
            out = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b, T in fbat:
                buf = torch.empty(len(b), F, T).pin_memory()
                atab.read_padded(b, T, buf)
                e = m.predict(buf.cuda(non_blocking=True), lengths=atab.rows[b]).cpu().numpy()
                for j, i in enumerate(b):
                    out[int(i)] = e[j]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        feat_pass()
        times = {"wav": [], "feats": []}
        for _ in range(2):
            tw, ow = wav_pass()
            tf, of = feat_pass()
            times["wav"].append(tw)
            times["feats"].append(tf)
        a = np.stack([ow[i][0] for i in range(args.n)]).astype(np.float64)
        b = np.stack([of[i] for i in range(args.n)]).astype(np.float64)
        cos = 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
        # kernels alone: a resident batch of 512 x 3 s
        B, N = 512, 3 * rate
        rng = np.random.default_rng(1)
        wave_t = torch.from_numpy(np.stack([synth(rng, N, rate) for _ in range(B)]).astype(np.float32)).cuda()
        nsamp = np.full(B, N, dtype=np.int64)
        kid = np.arange(B, dtype=np.int64)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def timed(fn, reps=20):
            fn()
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(reps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) / reps

        fb0 = dataclasses.replace(fb, dither=0.0)
        ms_resample = timed(lambda: features.resample(wave_t, nsamp, rate, 16000)) if rate != 16000 else 0.0
        w16, n16 = features.resample(wave_t, nsamp, rate, 16000)
        ms_fbank = timed(lambda: features.fbank(w16, n16, fb, kid, 0))
        ms_fbank_nodither = timed(lambda: features.fbank(w16, n16, fb0, kid, 0))
        ms_front = timed(lambda: fe(wave_t, nsamp, kid, 0))
        x512, L512 = fe(wave_t, nsamp, kid, 0)
        ms_predict = timed(lambda: m.predict(x512, lengths=L512), reps=5)
    audio = float(secs.sum())
    res = {
        "metric": "extraction from %d Hz WAV, ResNet-34 mean+std, 40 mel (conf/fbank.conf, conf/vad.conf, CMN 300), one process" % rate,
        "input_rate": rate,
        "utterances": args.n, "audio_seconds": audio, "batch_size": args.batch_size,
        "wav_utt_per_s": args.n / min(times["wav"]), "wav_audio_s_per_s": audio / min(times["wav"]),
        "feats_utt_per_s": args.n / min(times["feats"]), "feats_audio_s_per_s": audio / min(times["feats"]),
        "wav_pass_s": times["wav"], "feats_pass_s": times["feats"],
        "max_cos_dist_wav_vs_feats": float(cos.max()),
        # event times around the Python calls: they include the small H2D copies of the per-row counts and, for the whole front
        # end, the host read of the voiced counts (kernel-only times: rocprofv3 --kernel-trace --stats)
        "calls_b512_3s": {"resample_ms": ms_resample, "fbank_ms": ms_fbank, "fbank_nodither_ms": ms_fbank_nodither, "frontend_ms": ms_front, "predict_ms": ms_predict,
                            "frontend_share_of_predict": ms_front / ms_predict, "voiced_frames_max": int(L512.max()),
                            "audio_s_per_s_frontend": B * 3.0 / (ms_front / 1e3)},
        "operand_mode": os.environ.get("SPK_MFMA", "f16x3"), "device": torch.cuda.get_device_name(0), "split": ops.SPLIT,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
