#!/usr/bin/env python3
"""Cost of the GPU augmentation (features.augment, csrc/augment.hip).

--trace   one resident batch of 512 utterances x 3 s at 16 kHz, each with an impulse response of 1 s and one background noise:
          a warm-up, then --reps rounds of augment(quantize=True) + fbank.  Run it under `rocprofv3 --kernel-trace --stats -- python
          tools/augment_bench.py --trace` to get the augmentation kernels' time next to the fbank kernel's in one trace; the JSON
          line it prints holds the bytes the kernels move (so the trace can be set against the streaming rate) and the time per
          call by CUDA events.
default   end to end: a seeded synthetic set of --n utterances of 2-20 s (tools/wav_extract_bench.py's signals), 40 impulse
          responses of 1 s and 40 noises of 2-12 s are written as 16-bit WAV, and scripts/compute_fbank.py --egs runs on three
          wav.scp files over the same speech: plain, reverberated (every entry one impulse response) and noise (every entry
          foreground noises every few seconds, or 3-7 background signals with --duration, half and half).  After one untimed
          plain run (page cache, first-use costs) each runs twice; the figure is utterances per second of the script's own batch
          loop (`--time-batches`), best of the two.
Prints one JSON line.
usage: python tools/augment_bench.py [--trace] [--n 2000] [--batch-size 128] [--out FILE]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FS = 16000


def impulse_response(rng, n):
    h = 0.3 * rng.normal(0, 1, n) * np.exp(-np.arange(n) / (0.15 * n))
    h[:40] *= 0.05
    h[40] = 1.0
    return np.clip(h, -1.0, 1.0)


def write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(np.asarray(samples).astype(np.int16).tobytes())
    return path


def trace(args):
    import torch
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from wav_extract_bench import synth
    B, N, R = 512, 3 * FS, FS
    rng = np.random.default_rng(1)
    wave_t = torch.from_numpy(np.stack([synth(rng, N) for _ in range(B)]).astype(np.float32)).cuda()
    nsamp = np.full(B, N, dtype=np.int64)
    rirs = [impulse_response(rng, R).astype(np.float32) for _ in range(B)]
    pool = [np.round(rng.normal(0, 800, int(rng.uniform(2, 12) * FS))).astype(np.float32) for _ in range(40)]
    noises = [[(pool[b % 40], 3.0, 0.0, 10.0)] for b in range(B)]
    fb = features.FbankOptions(num_mel_bins=40, high_freq=7600, snip_edges=False)
    kid = np.arange(B, dtype=np.int64)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(reps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps

    ms_aug = timed(lambda: features.augment(wave_t, nsamp, rirs, noises, quantize=True), args.reps)
    ms_rvb = timed(lambda: features.augment(wave_t, nsamp, rirs, None, quantize=True), args.reps)
    ms_noise = timed(lambda: features.augment(wave_t, nsamp, None, noises, quantize=True), args.reps)
    out, clipped = features.augment(wave_t, nsamp, rirs, noises, quantize=True)
    ms_fbank = timed(lambda: features.fbank(out, nsamp, fb, kid, 0), args.reps)
    # bytes the kernels read and write per call: P = 1024, spectra of 1025 bins x 8 bytes
    P, bins = 1024, 1025
    M = N + R - 1
    nwx, npart, nb = -(-N // P) + 1, -(-R // P), -(-M // P)
    e = features.early_window(rirs[0], FS)
    nep, nbe = -(-(e[2] - e[1]) // P), -(-(N + e[2] - e[1] - 1) // P)
    spectra_w = (nwx + npart + nep) * bins * 8 + (N + R + (e[2] - e[1])) * 4          # written once, inputs read once
    nmac = sum(min(npart - 1, m) - max(0, m - (nwx - 1)) + 1 for m in range(nb)) \
        + sum(min(nep - 1, m) - max(0, m - (nwx - 1)) + 1 for m in range(nbe))              # (output block, partition) products
    conv_r = nmac * 2 * bins * 8
    rest = N * 4 + 3 * FS * 4 + M * 4 * 2 + M * 4 + 3 * FS * 4 + M * 4 + N * 4      # sums, mix (read y, noise; write y), output
    res = {"metric": "augment 512 x 3 s at 16 kHz, impulse response 1 s, one background noise (quantize=True), CUDA events around the call",
           "reps": args.reps, "augment_ms": ms_aug, "reverb_only_ms": ms_rvb, "noise_only_ms": ms_noise, "fbank_ms": ms_fbank,
           "bytes_per_call": {"spectra_kernel": B * spectra_w, "conv_kernel_reads": B * conv_r, "conv_kernel_writes": B * M * 4,
                              "other_kernels": B * rest},
           "us_at_6TBps": (B * (spectra_w + conv_r + M * 4 + rest)) / 6.0e12 * 1e6,
           "flop_per_call": B * (5 * 2048 * 11 * (nwx + npart + nep + nb + nbe) + 8 * bins * nmac),
           "clipped": int(clipped.sum()), "device": torch.cuda.get_device_name(0)}
    return res


def end_to_end(args):
    from wav_extract_bench import make_wavs
    rng = np.random.default_rng(args.seed)
    script = os.path.join(ROOT, "scripts", "compute_fbank.py")
    res = {"metric": "compute_fbank.py --egs, utterances per second of its batch loop, best of 2 (after one untimed plain run)",
           "utterances": args.n, "batch_size": args.batch_size}
    with tempfile.TemporaryDirectory() as d:
        keys, paths, secs = make_wavs(d, args.n, args.seed)
        rirs = [write_wav(os.path.join(d, "rir%02d.wav" % i), 20000 * impulse_response(rng, FS)) for i in range(40)]
        nz = [write_wav(os.path.join(d, "noise%02d.wav" % i), rng.normal(0, 800, int(rng.uniform(2, 12) * FS))) for i in range(40)]
        nz_dur = [wave.open(p).getnframes() / FS for p in nz]
        for name in ("fbank.conf", "vad.conf"):
            open(os.path.join(d, name), "w").write(open(os.path.join(ROOT, "tests", "golden", "fbank", name)).read())
        scp = {k: os.path.join(d, k + ".scp") for k in ("plain", "reverb", "noise")}
        with open(scp["plain"], "w") as f:
            f.writelines("%s %s\n" % kv for kv in zip(keys, paths))
        with open(scp["reverb"], "w") as f:
            f.writelines('%s cat %s | wav-reverberate --shift-output=true --impulse-response="%s"  - - |\n' % (
                k, p, rirs[int(rng.integers(40))]) for k, p in zip(keys, paths))
        with open(scp["noise"], "w") as f:
            for k, p, s in zip(keys, paths, secs):
                items, starts, snrs = [], [], []
                if rng.random() < 0.5:               # foreground noises, one after the other with a second between them
                    t = 0.0
                    while t < s:
                        j = int(rng.integers(40))
                        items.append(nz[j])
                        starts.append(t)
                        snrs.append(int(rng.choice([15, 10, 5, 0])))
                        t += nz_dur[j] + 1
                else:                                # background signals over the whole utterance
                    for _ in range(int(rng.integers(3, 8))):
                        items.append('wav-reverberate --duration=%s "%s" - |' % (s, nz[int(rng.integers(40))]))
                        starts.append(0)
                        snrs.append(int(rng.choice([20, 17, 15, 13])))
                f.write("%s wav-reverberate --shift-output=true --additive-signals='%s' --start-times='%s' --snrs='%s' %s - |\n" % (
                    k, ",".join(items), ",".join(str(v) for v in starts), ",".join(str(v) for v in snrs), p))
        env = dict(os.environ, PYTHONPATH=ROOT)

        def run(kind, tag):
            r = subprocess.run([sys.executable, script, scp[kind], os.path.join(d, "out_" + tag), "--egs", "--fbank-config",
                                os.path.join(d, "fbank.conf"), "--vad-config", os.path.join(d, "vad.conf"), "--batch-size",
                                str(args.batch_size), "--time-batches"], env=env, capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
            m = re.search(r"wrote (\d+) of \d+ utterances", r.stdout)
            t = re.search(r"([0-9.]+) s for the batches", r.stdout)            # --time-batches
            c = re.search(r"(\d+) samples clipped", r.stdout)
            return int(m.group(1)), float(t.group(1)), int(c.group(1)) if c else 0

        run("plain", "warm")
        for kind in ("plain", "reverb", "noise"):
            runs = [run(kind, "%s%d" % (kind, i)) for i in range(2)]
            res[kind] = {"utt_per_s": args.n / min(t for _, t, _ in runs), "batch_loop_s": [t for _, t, _ in runs],
                         "written": runs[0][0], "clipped_samples": runs[0][2]}
        res["audio_seconds"] = float(secs.sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = trace(args) if args.trace else end_to_end(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
