#!/usr/bin/env python3
"""Training from audio against training from the archive: loader-inclusive step throughput of
ingest.WavTrainLoader and of ingest.NativeTrainLoader (the --native-reader path) in front of the ResNet-34 training step, and the
rate of the step on a resident input, in one process on one box; the two loaders alternate (`--pairs` pairs).

A seeded synthetic corpus is written first: --files WAV files of 4-12 s at 16 kHz (tools/wav_extract_bench.py's signals), a quarter
of the wav.scp entries augmented (an impulse response of 0.5 s, or two foreground noises, half and half), the vad.scp of
features.vad on the clean files, and the float32 archive of the CMN'd voiced frames of the CLEAN files (the archive leg measures the
reader, whose cost does not depend on what the matrices hold).  Batch 256 x 300 frames x 80 mel bins, CMN window 300.

Then, from audio, the stages of the copy stream per batch by device events - H2D, spk_pcm16_to_f32, the augmentation, the span
front end, spk_cmn_select - and the reader thread's host time (planning and pread), with no training step beside them.
Prints one JSON line.

    python tools/wav_train_bench.py --out profiles/wav_train_bench.json

--speed adds a second wav.scp of the same files with two thirds of the entries as the speed-perturbed lines of
local/perturb_data_dir_speed.sh (`sox -t wav PATH -t wav - speed 0.9 |` / `1.1`, keys sp<F>-<utt>, in turn; the remaining third
keeps its plain or augmented entry) and the VAD vectors of the perturbed audio, and measures the loader over it ("audio_speed")
alternating with the from-audio leg in the same process, then the stages of its copy stream, the span resampler among them:

    python tools/wav_train_bench.py --speed --out profiles/wav_train_speed_bench.json
"""
import argparse
import contextlib
import json
import os
import shutil
import sys
import tempfile
import time
import wave

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
FS, FEAT, SPK, W = 16000, 80, 200, 300


def write_wav(path, samples):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(np.asarray(samples).astype(np.int16).tobytes())
    return path


def speed_of(i):
    """the factor of entry i of the --speed wav.scp"""
    return (None, "0.9", "1.1")[i % 3]


def write_corpus(d, n, opts, vad_opts, cmn, threads, min_voiced, speed=False):
    """wav.scp (a quarter augmented), vad.scp, utt2spkid, feats.scp of the clean egs matrices; speed: also speed.wav.scp,
    speed.vad.scp and speed.utt2spkid, two thirds of their entries speed-perturbed lines with the VAD of the perturbed audio"""
    from augment_bench import impulse_response
    from wav_extract_bench import synth
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io
    rng = np.random.default_rng(3)
    rirs = [write_wav(os.path.join(d, "rir%02d.wav" % i), 20000 * impulse_response(rng, FS // 2)) for i in range(20)]
    noises = [write_wav(os.path.join(d, "noise%02d.wav" % i), 900 * rng.normal(0, 1, int(rng.uniform(2, 6) * FS))) for i in range(20)]
    keys, paths, entries = [], [], []
    for i in range(n):
        k = "utt%05d" % i
        p = write_wav(os.path.join(d, k + ".wav"), synth(rng, int(rng.uniform(4, 12) * FS)))
        if i % 8 == 1:
            e = 'cat %s | wav-reverberate --shift-output=true --impulse-response="%s" - - |' % (p, rirs[i % 20])
        elif i % 8 == 5:
            e = ("wav-reverberate --shift-output=true --additive-signals='%s,%s' --start-times='0,2.5' --snrs='12,8' %s - |"
                 % (noises[i % 20], noises[(i + 7) % 20], p))
        else:
            e = p
        keys.append(k)
        paths.append(p)
        entries.append(e)
    open(os.path.join(d, "utt2spkid"), "w").writelines("%s %d\n" % (k, i % SPK) for i, k in enumerate(keys))
    table = ingest.WavTable(paths, FS)
    vad_lines, feat_lines, voiced = [""] * n, [""] * n, np.zeros(n, dtype=np.int64)
    sp_vad_lines, sp_voiced = [""] * n, np.zeros(n, dtype=np.int64)
    with open(os.path.join(d, "vad.ark"), "wb") as fv, open(os.path.join(d, "feats.ark"), "wb") as fa:
        for idx, nmax in ingest.pad_batches(table.nsamp, 64, quantum=1):
            buf = torch.empty(len(idx), nmax).pin_memory()
            table.read_padded(idx, nmax, buf, threads)
            wave_dev = buf.cuda(non_blocking=True)
            feats, T, loge = features.fbank(wave_dev, table.nsamp[idx], opts, [features.utt_id(keys[i]) for i in idx], 0)
            for sp in ("0.9", "1.1") if speed else ():
                rows = [r for r, i in enumerate(idx) if speed_of(i) == sp]
                if not rows:
                    continue
                w2, n2 = features.resample(wave_dev[rows], table.nsamp[idx[rows]], *features.speed_rates(sp, FS))
                _, T2, loge2 = features.fbank(w2, n2, opts, [features.utt_id(features.speed_key(sp, keys[idx[r]])) for r in rows], 0)
                v2, _, cnt2 = features.vad(loge2, T2, vad_opts)
                v2 = v2.cpu().numpy()
                for j, r in enumerate(rows):
                    i = idx[r]
                    sp_voiced[i] = cnt2[j]
                    fv.write((features.speed_key(sp, keys[i]) + " ").encode())
                    sp_vad_lines[i] = "%s %s:%d\n" % (features.speed_key(sp, keys[i]), os.path.join(d, "vad.ark"), fv.tell())
                    kaldi_io.write_vec_flt(fv, v2[j, :T2[j]].astype(np.float32))
            v, vidx, cnt = features.vad(loge, T, vad_opts)
            egs, lens = features.select_voiced(feats, T, vidx, cnt, cmn)
            v, egs = v.cpu().numpy(), egs.cpu().numpy()
            for r, i in enumerate(idx):
                voiced[i] = lens[r]
                fv.write((keys[i] + " ").encode())
                vad_lines[i] = "%s %s:%d\n" % (keys[i], os.path.join(d, "vad.ark"), fv.tell())
                kaldi_io.write_vec_flt(fv, v[r, :T[r]].astype(np.float32))
                off = kaldi_io.write_mat(fa, np.ascontiguousarray(egs[r, :, :lens[r]].T), key=keys[i])
                feat_lines[i] = "%s %s:%d\n" % (keys[i], os.path.join(d, "feats.ark"), off)
    # an entry with fewer voiced frames than the chunk cannot be drawn from
    keep = np.nonzero((voiced >= min_voiced) & np.asarray([not speed or speed_of(i) is None or sp_voiced[i] >= min_voiced
                                                           for i in range(n)]))[0]
    if speed:
        def line(i):
            sp = speed_of(i)
            return (keys[i], entries[i], vad_lines[i]) if sp is None else \
                (features.speed_key(sp, keys[i]), "sox -t wav %s -t wav - speed %s |" % (paths[i], sp), sp_vad_lines[i])
        open(os.path.join(d, "speed.wav.scp"), "w").writelines("%s %s\n" % line(i)[:2] for i in keep)
        open(os.path.join(d, "speed.vad.scp"), "w").writelines(line(i)[2] for i in keep)
        open(os.path.join(d, "speed.utt2spkid"), "w").writelines("%s %d\n" % (line(i)[0], i % SPK) for i in keep)
    open(os.path.join(d, "wav.scp"), "w").writelines("%s %s\n" % (keys[i], entries[i]) for i in keep)
    open(os.path.join(d, "vad.scp"), "w").writelines(vad_lines[i] for i in keep)
    open(os.path.join(d, "feats.scp"), "w").writelines(feat_lines[i] for i in keep)
    names = ("wav.scp", "vad.scp", "utt2spkid", "feats.scp") + (("speed.wav.scp", "speed.vad.scp", "speed.utt2spkid") if speed else ())
    return {k: os.path.join(d, k) for k in names}, int(table.nsamp[keep].sum()) * 2, len(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--speed", action="store_true", help="also the leg with two thirds of the entries as 0.9 / 1.1 speed lines")
    ap.add_argument("--out")
    args = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features
    from pytorch_kaldi_resnet_amd.engine import GraphedTrainStep
    from pytorch_kaldi_resnet_amd.ingest import NativeTrainLoader, WavTrainLoader
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    from pytorch_kaldi_resnet_amd.optim import FlatSGD
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    opts = features.FbankOptions(num_mel_bins=FEAT, snip_edges=False, dither=1.0)
    vad_opts, cmn = features.VadOptions(), features.CmnOptions(cmn_window=W)
    d = tempfile.mkdtemp(prefix="spk_wav_train_")
    try:
        t0 = time.perf_counter()
        files, wav_bytes, kept = write_corpus(d, args.files, opts, vad_opts, cmn, args.threads, args.frames, args.speed)
        sys.stderr.write("wrote %d files (%d with enough voiced frames, %.0f MB of audio) and their archive in %.1f s\n" % (args.files, kept, wav_bytes / 1e6,
                                                                                              time.perf_counter() - t0))
        kw = dict(seed=5, threads=args.threads, drop_last=True, prefetch=3, device=str(dev))
        with contextlib.redirect_stdout(sys.stderr):
            loaders = {"archive": NativeTrainLoader(files["feats.scp"], files["utt2spkid"], args.frames, args.batch, **kw),
                       "audio": WavTrainLoader(files["wav.scp"], files["utt2spkid"], args.frames, args.batch, opts, cmn,
                                               vad_scp=files["vad.scp"], **kw)}
            if args.speed:
                loaders["audio_speed"] = WavTrainLoader(files["speed.wav.scp"], files["speed.utt2spkid"], args.frames, args.batch, opts,
                                                        cmn, vad_scp=files["speed.vad.scp"], **kw)
            torch.manual_seed(0)
            model = NeuralSpeakerModel(SPK, FEAT, "mean+std", "AAM", 0.2, 30, arch="resnet34").to(dev)
            model.train()
            opt = FlatSGD(model, 0.1, momentum=0.9, weight_decay=5e-4)
            graphed = GraphedTrainStep(model.engine(), args.batch, args.frames)

        def step(xb, yb):
            loss, _, _ = graphed(xb, yb, None)
            opt.step()
            return loss

        def batches(loader):
            ep = 0
            while True:
                loader.set_epoch(ep)
                ep += 1
                for xb, yb in loader:
                    yield xb, yb
        its = {k: batches(loaders[k]) for k in loaders}

        def leg(kind):
            it = its[kind] if kind != "resident" else None
            xb, yb = next(its["archive"]) if it is None else (None, None)
            for _ in range(args.warmup):
                step(*(next(it) if it is not None else (xb, yb)))
            torch.cuda.synchronize()
            c0, t1 = os.times(), time.perf_counter()
            for _ in range(args.steps):
                step(*(next(it) if it is not None else (xb, yb)))
            torch.cuda.synchronize()
            dt, c1 = time.perf_counter() - t1, os.times()
            return {"kind": kind, "ms_per_step": dt / args.steps * 1e3, "utt_per_s": args.batch * args.steps / dt,
                    "cpu_s": (c1.user - c0.user) + (c1.system - c0.system)}
        legs = [leg("resident")]
        for _ in range(args.pairs):
            legs += [leg("archive"), leg("audio")] + ([leg("audio_speed")] if args.speed else [])
        legs.append(leg("resident"))

        def copy_stream_stages(wl):
            """the stages of the copy stream of one loader, with nothing else on the device"""
            wl.times, wl.reader_seconds = [], []
            it = batches(wl)
            for _ in range(args.warmup + args.steps):
                xb, _ = next(it)
                xb.sum()
            torch.cuda.synchronize()
            stages = {}
            for name in ("h2d", "convert", "augment", "resample", "frontend", "cmn"):
                ms = [t[name][0].elapsed_time(t[name][1]) for t in wl.times[args.warmup:] if name in t]
                stages[name + "_ms"] = float(np.mean(ms)) if ms else None
            stages["reader_host_ms"] = float(np.mean(wl.reader_seconds[args.warmup:])) * 1e3
            stages["batches"] = len(wl.times) - args.warmup
            wl.times = None
            return stages
        wl = loaders["audio"]
        stages = copy_stream_stages(wl)

        def best(kind):
            return min(l["ms_per_step"] for l in legs if l["kind"] == kind)
        out = {"tool": "wav_train_bench", "files": args.files, "files_used": kept, "audio_bytes": wav_bytes, "batch": args.batch, "frames": args.frames,
               "mel_bins": FEAT, "cmn_window": W, "augmented_share": 0.25, "arch": "resnet34", "steps": args.steps, "pairs": args.pairs,
               "threads": args.threads, "legs": legs, "best_ms_per_step": {k: best(k) for k in ["resident", "archive", "audio"] + ["audio_speed"] * args.speed},
               "audio_over_archive": best("audio") / best("archive"), "copy_stream_stages": stages,
               "clipped_samples": int(wl.pool.clipped) if wl.pool is not None and wl.pool.clipped is not None else 0,
               "aux_files_read": wl.pool.reads if wl.pool is not None else 0, "device": torch.cuda.get_device_name(0)}
        if args.speed:
            out.update({"speed_share": 2 / 3, "speed_factors": ["0.9", "1.1"], "audio_speed_over_audio": best("audio_speed") / best("audio"),
                        "copy_stream_stages_speed": copy_stream_stages(loaders["audio_speed"])})
        line = json.dumps(out)
        print(line)
        if args.out:
            open(args.out, "w").write(line + "\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
