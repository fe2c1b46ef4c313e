#!/usr/bin/env python3
"""Embedding extraction on MI355X - same flags and output format as the reference's scripts/decode.py
(argparse :26-61, main_worker :101-182, SequenceGenerator :185-208): load a checkpoint through loadParameters,
run predict() under eval(), write text-ark lines 'utt [ v0 ... v255 ]' with str(np.float32) to <out-path>/<gpu>.
One process per GPU shards the scp with a DistributedSampler; no collective is issued.
Unlike the reference (decode.py:204 is only correct at per-process batch size 1) batches of equal-length
utterances are supported: --chunk-size T crops, --chunk-size -1 needs equal lengths within a batch.
"""
import argparse
import os
import time
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

parser = argparse.ArgumentParser(description="speaker-embedding extraction (MI355X-native)")
parser.add_argument("--spk_num", type=int, help="number of speakers")
parser.add_argument("--arch", type=str, required=True, help="resnet18/34/50/101 or se_resnet34")
parser.add_argument("--input-dim", type=int, required=True)
parser.add_argument("--pooling", type=str, required=True, help="mean or mean+std")
parser.add_argument("--chunk-size", default=-1, type=int)
parser.add_argument("--model-path", help="checkpoint (.pth.tar)")
parser.add_argument("--world-size", default=-1, type=int)
parser.add_argument("--rank", default=-1, type=int)
parser.add_argument("-j", "--workers", default=2, type=int)
parser.add_argument("-b", "--batch-size", default=128, type=int, help="total batch size over the node's GPUs")
parser.add_argument("--dist-url", default="tcp://127.0.0.1:23456", type=str)
parser.add_argument("--dist-backend", default="nccl", type=str)
parser.add_argument("--seed", default=None, type=int)
parser.add_argument("--gpu", type=int)
parser.add_argument("--gpu-num", default=-1, type=int)
parser.add_argument("--decode-scp", help="decode.scp")
parser.add_argument("--out-path", help="output directory")
parser.add_argument("--multiprocessing-distributed", action="store_true")
parser.add_argument("--native-reader", action="store_true",
                    help="read whole utterances with the C++ ark reader, bucketed by length so that any --batch-size works "
                         "with variable-length utterances (the reference is limited to per-process batch 1)")
parser.add_argument("--pad-batches", action="store_true",
                    help="with --native-reader and --chunk-size -1: length-sorted batches of up to --batch-size utterances padded to a "
                         "common length (at most 10%% padded frames, T rounded up to 8) and run through the length-masked "
                         "predict(x, lengths=...): each embedding is that of its utterance alone")
parser.add_argument("--wav-scp", help="extract from audio: a wav.scp of PCM 16-bit mono files (instead of --decode-scp); the "
                    "Kaldi fbank (or, with --mfcc-config, MFCC; + sliding CMN, + energy VAD frame selection) runs on the GPU (pytorch_kaldi_resnet_amd.features)")
parser.add_argument("--allow-downsample", action="store_true",
                    help="with --wav-scp: resample files above the fbank's --sample-frequency on the GPU instead of refusing them")
parser.add_argument("--allow-upsample", action="store_true",
                    help="with --wav-scp: resample files below the fbank's --sample-frequency on the GPU instead of refusing them")
parser.add_argument("--fbank-config", help="with --wav-scp: Kaldi compute-fbank-feats config (conf/fbank.conf)")
parser.add_argument("--mfcc-config", help="with --wav-scp: Kaldi compute-mfcc-feats config (conf/mfcc.conf): the model input is the "
                    "MFCC (--input-dim = its num-ceps) instead of the fbank; not together with --fbank-config")
parser.add_argument("--vad-config", help="with --wav-scp: Kaldi compute-vad config (conf/vad.conf): keep voiced frames only")
parser.add_argument("--cmn-window", type=int, default=0,
                    help="with --wav-scp: apply-cmvn-sliding --norm-vars=false --center=true window (0: none; the recipe uses 300)")
parser.add_argument("--half", action="store_true",
                    help="extract with predict(precision='f16'): fp16 activations, one fp16 product per multiply-accumulate.  "
                         "Utterances whose activations leave fp16's range are detected on the GPU and extracted again in fp32 "
                         "(resnet18/34/50/101; not se_resnet34)")
parser.add_argument("--window", type=int, default=None,
                    help="windowed extraction (with --native-reader --pad-batches, or with --wav-scp): a window of W frames every "
                         "--period frames, each embedded alone; the last, shorter window of an utterance is kept when it has at "
                         "least --min-window frames.  One vector per window under the key <utt>-<start:08d>-<end:08d> (frame "
                         "indices, end exclusive) and a file segments.<name> next to the embeddings with lines '<key> <utt> "
                         "<start s> <end s>'.  With --wav-scp the indices count the frames the model sees, that is after the VAD's "
                         "frame selection; --vad-segments or --segments keep times in the recording")
parser.add_argument("--vad-segments", action="store_true",
                    help="with --wav-scp --vad-config --window: diarization-style extraction.  The VAD decisions become speech "
                         "segments on the GPU (--seg-padding / --seg-max-gap / --seg-min-length), no frame is removed (the sliding "
                         "CMN runs over the whole recording) and the windows slide inside every segment: keys and segments.<name> "
                         "carry frames and times of the recording, and speech_segments.<name> lists the segments used")
parser.add_argument("--seg-padding", type=int, default=None, help="with --vad-segments: frames added on both sides of a voiced run (default 10)")
parser.add_argument("--seg-max-gap", type=int, default=None,
                    help="with --vad-segments: padded runs at most this many frames apart are joined into one segment (default 30)")
parser.add_argument("--seg-min-length", type=int, default=None, help="with --vad-segments: segments shorter than this are dropped (default 50)")
parser.add_argument("--segments", default=None,
                    help="with --wav-scp --window, instead of --vad-config / --vad-segments: a Kaldi segments file '<segment-id> "
                         "<recording> <start s> <end s>' (recordings: the keys of --wav-scp); the windows slide inside these segments. "
                         "Frame of a time t: floor(t / --frame-shift + 0.5); ends are clipped to the recording's frame count")
parser.add_argument("--period", type=int, default=None, help="with --window: frames between window starts (default: --window)")
parser.add_argument("--min-window", type=int, default=None,
                    help="with --window: shortest last window that is kept, and shortest utterance that is extracted at all "
                         "(default: --window with --average-windows, else 1)")
parser.add_argument("--average-windows", action="store_true",
                    help="with --window: one vector per utterance under its own key, the mean of its window embeddings weighted "
                         "by window length (with --period = --window: nnet3-xvector-compute --chunk-size W --min-chunk-size M); "
                         "utterances shorter than --min-window are listed on stderr and counted")
parser.add_argument("--frame-shift", type=float, default=0.01,
                    help="with --window: seconds per frame, used only for the times in segments.<name> (default 0.01)")
parser.add_argument("--out-format", default="text", choices=["text", "fv"],
                    help="text = the reference's 'utt [ v0 ... ]' lines (str(np.float32), ~0.2 ms/utt of Python formatting); "
                         "fv = binary Kaldi float-vector ark, read by the same scoring scripts")


def main():
    args = parser.parse_args()
    if args.half and args.arch == "se_resnet34":
        parser.error("--half does not support --arch se_resnet34 (squeeze-and-excitation blocks run in fp32 only)")
    if args.wav_scp and args.decode_scp:
        parser.error("--wav-scp and --decode-scp are mutually exclusive")
    if (args.fbank_config or args.vad_config or args.cmn_window or args.allow_downsample or args.allow_upsample) and not args.wav_scp:
        parser.error("--fbank-config / --vad-config / --cmn-window / --allow-downsample / --allow-upsample need --wav-scp")
    if args.mfcc_config and args.fbank_config:
        parser.error("--mfcc-config and --fbank-config are mutually exclusive")
    if args.mfcc_config and not args.wav_scp:
        parser.error("--mfcc-config needs --wav-scp")
    if args.mfcc_config:        # before the model is built: a config whose num-ceps is not the model's input dimension
        import pytorch_kaldi_resnet_amd  # noqa: F401
        from pytorch_kaldi_resnet_amd import features
        try:
            num_ceps = features.MfccOptions.from_kaldi_config(args.mfcc_config).num_ceps
        except (OSError, ValueError) as e:
            parser.error("--mfcc-config: %s" % e)
        if num_ceps != args.input_dim:
            parser.error("--input-dim %d differs from the num-ceps %d of --mfcc-config %s" % (args.input_dim, num_ceps, args.mfcc_config))
    if args.window is None:
        if args.period is not None or args.min_window is not None or args.average_windows:
            parser.error("--period / --min-window / --average-windows need --window")
    else:
        if not (args.wav_scp or (args.native_reader and args.pad_batches)):
            parser.error("--window needs --native-reader --pad-batches or --wav-scp")
        if args.chunk_size >= 0:
            parser.error("--window and --chunk-size >= 0 are mutually exclusive (--chunk-size crops, --window covers the utterance)")
        if args.period is None:
            args.period = args.window
        if args.min_window is None:
            args.min_window = args.window if args.average_windows else 1
        if args.window < 1 or args.period < 1:
            parser.error("--window and --period must be >= 1, got --window %d --period %d" % (args.window, args.period))
        if not 1 <= args.min_window <= args.window:
            parser.error("--min-window must lie in [1, --window %d], got %d" % (args.window, args.min_window))
    if args.vad_segments and not (args.wav_scp and args.vad_config and args.window is not None):
        parser.error("--vad-segments needs --wav-scp, --vad-config and --window")
    for flag in ("seg_padding", "seg_max_gap", "seg_min_length"):
        if getattr(args, flag) is not None and not args.vad_segments:
            parser.error("--%s needs --vad-segments" % flag.replace("_", "-"))
    if args.segments is not None:
        if args.vad_config or args.vad_segments:
            parser.error("--segments and --vad-config / --vad-segments are mutually exclusive (the file gives the segments)")
        if not (args.wav_scp and args.window is not None):
            parser.error("--segments needs --wav-scp and --window")
    if args.vad_segments or args.segments is not None:
        import pytorch_kaldi_resnet_amd  # noqa: F401
        from pytorch_kaldi_resnet_amd import features, ingest
        try:
            if args.vad_segments:
                d = features.SegmentOptions()
                args.segment_opts = features.SegmentOptions(
                    padding=d.padding if args.seg_padding is None else args.seg_padding,
                    max_gap=d.max_gap if args.seg_max_gap is None else args.seg_max_gap,
                    min_length=d.min_length if args.seg_min_length is None else args.seg_min_length)
            else:
                args.file_segments = ingest.read_segments_file(args.segments, features.read_wav_scp(args.wav_scp)[0], args.frame_shift)
        except (OSError, ValueError) as e:
            parser.error("--%s: %s" % ("vad-segments" if args.vad_segments else "segments", e))
    if args.pad_batches and not args.native_reader:
        parser.error("--pad-batches needs --native-reader")
    if args.pad_batches and args.chunk_size >= 0:
        parser.error("--pad-batches extracts whole utterances: use --chunk-size -1")
    if args.dist_url == "env://" and args.world_size == -1:
        args.world_size = int(os.environ["WORLD_SIZE"])
    args.distributed = args.world_size > 1 or args.multiprocessing_distributed
    ngpus = torch.cuda.device_count() if args.gpu_num == -1 else min(torch.cuda.device_count(), args.gpu_num)
    if args.multiprocessing_distributed:
        args.world_size = ngpus * args.world_size
        mp.spawn(main_worker, nprocs=ngpus, args=(ngpus, args))
    else:
        main_worker(args.gpu if args.gpu is not None else 0, ngpus, args)


def collate(batch):
    feats = [b[0] for b in batch]
    t0 = feats[0].shape[1]
    if any(f.shape[1] != t0 for f in feats):
        raise RuntimeError("utterances of different length in one batch: use --batch-size = number of GPUs "
                           "(per-process batch 1, as the reference's recipes do) or --chunk-size T")
    return torch.from_numpy(np.stack(feats)), [b[1] for b in batch]


def main_worker(gpu, ngpus_per_node, args):
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd.datasets import EmbeddingDataset
    from pytorch_kaldi_resnet_amd.model import NeuralSpeakerModel
    args.gpu = gpu
    if args.distributed:
        if args.dist_url == "env://" and args.rank == -1:
            args.rank = int(os.environ["RANK"])
        if args.multiprocessing_distributed:
            args.rank = args.rank * ngpus_per_node + gpu
        dist.init_process_group(backend=args.dist_backend, init_method=args.dist_url, world_size=args.world_size,
                                rank=args.rank)
        args.batch_size = max(1, int(args.batch_size / ngpus_per_node))
        args.workers = int((args.workers + ngpus_per_node - 1) / ngpus_per_node)
    torch.cuda.set_device(args.gpu)
    print("=> creating model '{}'".format(args.arch))
    model = NeuralSpeakerModel(spk_num=args.spk_num, feat_dim=args.input_dim, pooling=args.pooling, arch=args.arch)
    if not (args.model_path and os.path.isfile(args.model_path)):
        print("=> no checkpoint found at '{}'".format(args.model_path))
        return
    print("=> loading checkpoint '{}'".format(args.model_path))
    ckpt = torch.load(args.model_path, map_location="cpu", weights_only=True)
    model.loadParameters(ckpt["state_dict"])
    print("=> loaded checkpoint '{}' (epoch {})".format(args.model_path, ckpt.get("epoch")))
    model.cuda(args.gpu)
    os.makedirs(args.out_path, exist_ok=True)
    if args.wav_scp:
        wav_generator(model, args)
        if args.distributed:
            dist.destroy_process_group()
        return
    if args.native_reader:
        native_generator(model, args)
        if args.distributed:
            dist.destroy_process_group()
        return
    ds = EmbeddingDataset(scp_file=args.decode_scp, chunk_size=args.chunk_size)
    sampler = None
    if args.distributed:
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=args.world_size, rank=args.rank,
                                                                  shuffle=True)
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=args.workers,
                                         pin_memory=True, sampler=sampler, collate_fn=collate)
    print("=> args.world_size: {}, args.rank: {}, loaded embedding samples num: {}".format(args.world_size, args.rank,
                                                                                         len(loader)))
    sequence_generator(loader, model, args.out_path, args)
    if args.distributed:
        dist.destroy_process_group()


def _write(f, utts, pred, fmt):
    from pytorch_kaldi_resnet_amd import kaldi_io
    for i in range(pred.shape[0]):
        if fmt == "text":
            f.write(utts[i] + " [ " + " ".join(map(str, pred[i, :].flatten())) + " ]\n")
        else:
            kaldi_io.write_vec_flt(f, np.ascontiguousarray(pred[i]), key=utts[i])


class Predictor:
    """predict() of one batch -> numpy embeddings.  --half: the half-precision predict; the per-utterance overflow counts come back
    with the embeddings in the same device-to-host copy, and the rows whose activations left fp16's range are predicted again
    in fp32 (x[idx], lengths[idx]) - their embeddings replace the half ones."""

    def __init__(self, model, half):
        self.model, self.half = model, half
        self.redone = self.total = 0

    def __call__(self, x, lengths=None):
        if not self.half:
            return self.model.predict(x, lengths=lengths).cpu().numpy()
        emb = self.model.predict(x, lengths=lengths, precision="f16")
        ovf = self.model.engine().half_overflow
        both = torch.cat([emb, (ovf > 0).to(emb.dtype)[:, None]], dim=1).cpu().numpy()
        pred = np.ascontiguousarray(both[:, :-1])
        idx = np.nonzero(both[:, -1])[0]
        self.total += pred.shape[0]
        if idx.size:
            self.redone += idx.size
            sub = x[torch.from_numpy(idx).to(x.device)].contiguous()
            pred[idx] = self.model.predict(sub, lengths=None if lengths is None else np.asarray(lengths)[idx]).cpu().numpy()
        return pred

    def report(self):
        if self.half:
            print("=> {} of {} utterances left the fp16 range and were extracted in fp32".format(self.redone, self.total))


class WindowPredictor:
    """--window: predict_windows() of one padded batch -> (numpy embeddings, their keys, their segments lines or None).  Without
    --average-windows a row per window, keyed <utt>-<start:08d>-<end:08d>; with it a row per utterance, the length-weighted mean
    of its windows (spk_window_mean).  --half: the windows whose activations left fp16's range (engine().half_overflow, one count
    per window) are gathered and predicted again in fp32, before any averaging.  Utterances shorter than --min-window are named
    on stderr and counted.  segments (--vad-segments / --segments): (row, start, end) speech segments of the batch in frames of the
    recording; the windows slide inside them, the segments shorter than --min-window are the ones named and counted, and
    self.speech_lines holds the speech_segments lines of the segments that were used."""

    def __init__(self, model, args):
        self.model, self.a = model, args
        self.redone = self.total = self.skipped = self.utts = self.segs = 0
        self.speech_lines = []

    def __call__(self, x, lengths, names, segments=None):
        from pytorch_kaldi_resnet_amd import ingest, ops
        a, m = self.a, self.model
        x = x.contiguous()
        lengths = np.asarray(lengths, dtype=np.int64)
        kw = dict(window=a.window, period=a.period, min_window=a.min_window, batch_size=a.batch_size)
        if segments is not None:
            kw["segments"] = segments
        if a.average_windows and not a.half:
            emb, utt = m.predict_windows(x, lengths, average=True, **kw)
        else:
            emb, utt, start, length = m.predict_windows(x, lengths, precision="f16" if a.half else "f32", **kw)
            if a.half and utt.size:
                idx = np.nonzero(m.engine().half_overflow.cpu().numpy())[0]
                self.total += utt.size
                self.redone += idx.size
                for sub, wcap in (ingest.window_batches(length[idx], a.batch_size) if idx.size else []):
                    rows = idx[sub]
                    xw = ops.window_gather(x, utt[rows], start[rows], length[rows], wcap)
                    emb[torch.from_numpy(rows).to(emb.device)] = m.predict(xw, lengths=length[rows].tolist())
            if a.average_windows and utt.size:
                uu, first = np.unique(utt, return_index=True)
                emb, utt = ops.window_mean(emb, np.append(first, utt.size), length.astype(np.float32)), uu
        skipped = m.engine().windows_skipped
        if segments is None:
            for b in skipped:
                sys.stderr.write("=> skipping {}: {} frames, shorter than --min-window {}\n".format(names[b], int(lengths[b]), a.min_window))
        else:
            row, s0, s1 = segments
            for j in skipped:
                sys.stderr.write("=> skipping segment {}-{:08d}-{:08d}: shorter than --min-window {}\n".format(
                    names[row[j]], int(s0[j]), int(s1[j]), a.min_window))
            used = np.setdiff1d(np.arange(len(row)), skipped)
            self.speech_lines = ["%s-%08d-%08d %s %.3f %.3f\n" % (names[row[j]], s0[j], s1[j], names[row[j]], s0[j] * a.frame_shift,
                                                                  s1[j] * a.frame_shift) for j in used]
            self.segs += len(row)
        self.skipped += len(skipped)
        self.utts += len(names)
        pred = emb.cpu().numpy()
        if a.average_windows:
            return pred, [names[b] for b in utt], None
        keys = ["%s-%08d-%08d" % (names[b], s, s + l) for b, s, l in zip(utt, start, length)]
        seg = ["%s %s %.3f %.3f\n" % (k, names[b], s * a.frame_shift, (s + l) * a.frame_shift)
               for k, b, s, l in zip(keys, utt, start, length)]
        return pred, keys, seg

    def report(self):
        if self.a.half:
            print("=> {} of {} windows left the fp16 range and were extracted in fp32".format(self.redone, self.total))
        if self.a.vad_segments or self.a.segments is not None:
            print("=> {} of {} segments shorter than --min-window were skipped".format(self.skipped, self.segs))
        else:
            print("=> {} of {} utterances shorter than --min-window were skipped".format(self.skipped, self.utts))


def _emit(f, seg, keys, pred, seglines, args):
    """one batch of vectors (text: formatted natively; fv: binary Kaldi vectors) and, with --window, its segments lines"""
    from pytorch_kaldi_resnet_amd import ingest, kaldi_io
    if pred.shape[0] == 0:
        return
    if args.out_format == "text":
        f.write(ingest.format_text_vectors(keys, pred, max(1, args.workers)))
    else:
        for i in range(pred.shape[0]):
            kaldi_io.write_vec_flt(f, np.ascontiguousarray(pred[i]), key=keys[i])
    if seg is not None and seglines:
        seg.write("".join(seglines))


def _segments_file(args, name):
    if args.window is None or args.average_windows:
        return None
    return open(os.path.join(args.out_path, "segments." + name), "w")


def sequence_generator(loader, model, out_path, args):
    model.eval()
    name = str(args.gpu) if args.distributed else "alone"
    predict = Predictor(model, args.half)
    with open(os.path.join(out_path, name), "w" if args.out_format == "text" else "wb") as f, torch.no_grad():
        for audios, utts in loader:
            pred = predict(audios.cuda(args.gpu, non_blocking=True))
            _write(f, utts, pred, args.out_format)
    predict.report()


def native_generator(model, args):
    """Length-bucketed extraction through libspkio: utterances of equal frame count share a batch (whole utterance when
    --chunk-size -1, else the first chunk-size frames... the reference crops at random; extraction of a fixed window is
    deterministic here), each rank takes every world-th batch.  --pad-batches: length-sorted batches of unequal lengths padded
    to a common T (ingest.pad_batches) and the length-masked predict instead of equal-length buckets.
    An scp of one-byte compressed 'CM ' matrices only is read as codes + column headers - a quarter of the
    bytes through the pinned buffer and the copy - and decoded on the GPU (features.decompress) with the batch's lengths."""
    from pytorch_kaldi_resnet_amd import features, ingest
    from pytorch_kaldi_resnet_amd.ingest import ArkTable
    tab = [l.rstrip().split(None, 1) for l in open(args.decode_scp)]
    utts = [u for u, _ in tab]
    table = ArkTable([r for _, r in tab])
    print("Totally " + str(len(utts)) + " samples")
    T_of = table.rows if args.chunk_size < 0 else np.minimum(table.rows, args.chunk_size)
    if args.chunk_size >= 0:
        assert (table.rows >= args.chunk_size).all(), "utterance shorter than --chunk-size"
    if args.pad_batches:
        # length-sorted batches padded to a common T_pad, each utterance masked to its own length inside the model
        batches = ingest.pad_batches(table.rows, args.batch_size)
        real = int(table.rows.sum())
        print("=> {} padded batches, padding overhead {:.3f} (padded / real frames)".format(
            len(batches), sum(len(b) * T for b, T in batches) / max(real, 1)))
    else:
        order = np.argsort(T_of, kind="stable")
        batches, i = [], 0
        while i < len(order):
            j = i
            while j < len(order) and j - i < args.batch_size and T_of[order[j]] == T_of[order[i]]:
                j += 1
            batches.append((order[i:j], int(T_of[order[i]])))
            i = j
    rank, world = (max(args.rank, 0), max(args.world_size, 1)) if args.distributed else (0, 1)
    model.eval()
    name = str(args.gpu) if args.distributed else "alone"
    F = int(table.cols[0])
    mine = batches[rank::world]
    # three-stage pipeline: a reader thread fills the next pinned batch (pread + transpose in libspkio, GIL released)
    # and a writer thread formats the previous batch's embeddings (natively, byte-identical to the reference's
    # str(np.float32) text) while the GPU works on the current one
    from concurrent.futures import ThreadPoolExecutor
    from pytorch_kaldi_resnet_amd import kaldi_io
    pinned = {}

    def load(n):
        b, T = mine[n]
        key = (n & 1, len(b), T)
        buf = pinned.get(key)
        if buf is None:
            for k in [k for k in pinned if k[0] == key[0]]:
                del pinned[k]                    # one live buffer per parity: its previous batch has been consumed
            if table.all_cm:
                buf = pinned[key] = (torch.empty(len(b), F, T, dtype=torch.uint8).pin_memory(), torch.empty(len(b), F, 4).pin_memory())
            else:
                buf = pinned[key] = torch.empty(len(b), F, T).pin_memory()
        if table.all_cm and args.pad_batches:
            table.read_padded_codes(b, T, buf[0], buf[1], max(1, args.workers))
        elif table.all_cm:
            table.read_crop_codes(b, [0] * len(b), T, buf[0], buf[1], max(1, args.workers))
        elif args.pad_batches:
            table.read_padded(b, T, buf, max(1, args.workers))
        else:
            table.read_crop(b, [0] * len(b), T, buf, max(1, args.workers))
        return buf

    predict = Predictor(model, args.half) if args.window is None else WindowPredictor(model, args)
    seg = _segments_file(args, name)
    with open(os.path.join(args.out_path, name), "wb") as f, torch.no_grad(), ThreadPoolExecutor(1) as rd, \
            ThreadPoolExecutor(1) as wr:
        nxt = rd.submit(load, 0) if mine else None
        pending = None
        t0, done = time.time(), 0
        for n, (b, _) in enumerate(mine):
            buf = nxt.result()
            nxt = rd.submit(load, n + 1) if n + 1 < len(mine) else None
            lengths = table.rows[b] if args.pad_batches else None
            if table.all_cm:
                x = features.decompress(buf[0].cuda(args.gpu, non_blocking=True), buf[1].cuda(args.gpu, non_blocking=True), lengths)
            else:
                x = buf.cuda(args.gpu, non_blocking=True)
            keys, seglines = [utts[k] for k in b], None
            if args.window is None:
                pred = predict(x, lengths)
            else:
                pred, keys, seglines = predict(x, lengths, keys)
            if pending is not None:
                pending.result()
            pending = wr.submit(_emit, f, seg, keys, pred, seglines, args)
            done += len(b)
        if pending is not None:
            pending.result()
        if seg is not None:
            seg.close()
        dt = time.time() - t0
        print("=> extracted {} utterances in {:.2f} s ({:.0f} utt/s, read + predict + write)".format(done, dt, done / max(dt, 1e-9)))
    predict.report()


def _file_segments(per, names, lengths):
    """--segments: the (row, start, end) of a batch of recordings from ingest.read_segments_file's table, ends clipped to the
    recording's frame count; a segment that starts at or beyond it is reported and left out"""
    row, start, end = [], [], []
    for r, name in enumerate(names):
        s, e = per.get(name, (np.zeros(0, dtype=np.int64),) * 2)
        e = np.minimum(e, int(lengths[r]))
        for j in np.nonzero(e <= s)[0]:
            sys.stderr.write("=> skipping segment {}-{:08d}: it starts beyond the {} frames of the recording\n".format(name, int(s[j]), int(lengths[r])))
        ok = e > s
        row.append(np.full(int(ok.sum()), r, dtype=np.int64))
        start.append(s[ok])
        end.append(e[ok])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)
    return cat(row), cat(start), cat(end)


def wav_generator(model, args):
    """--wav-scp: batches of utterances of one sample rate sorted by sample count (at most 10 % padded samples; files at another
    rate than the fbank's are resampled on the GPU, given --allow-downsample / --allow-upsample) read by the native WAV reader into
    pinned memory - the next batch while the GPU runs the front end and the length-masked predict of the current one.  Output
    format as native_generator; utterances shorter than one frame or without voiced frames are reported and skipped."""
    from concurrent.futures import ThreadPoolExecutor
    from pytorch_kaldi_resnet_amd import features, ingest, kaldi_io
    fb, vad_opts, cmn = features.options_from_configs(args.fbank_config, args.vad_config, args.cmn_window,
                                                      mfcc_config=args.mfcc_config or None)
    by_segment = args.vad_segments or args.segments is not None
    frontend = features.Frontend(fb, vad_opts, cmn, segments=args.segment_opts if args.vad_segments else None)
    keys, table, batches, short = features.wav_scp_batches(args.wav_scp, fb, args.batch_size, args.allow_downsample,
                                                           args.allow_upsample)
    print("Totally " + str(len(keys)) + " samples")
    for i in short:
        print("=> skipping {}: {} samples at {} Hz, shorter than one frame".format(keys[i], int(table.nsamp[i]), int(table.rate[i])))
    rank, world = (max(args.rank, 0), max(args.world_size, 1)) if args.distributed else (0, 1)
    mine = batches[rank::world]
    seed = 0 if args.seed is None else args.seed
    model.eval()
    name = str(args.gpu) if args.distributed else "alone"

    def load(n):
        b, nmax = mine[n]
        buf = torch.empty(len(b), nmax).pin_memory()
        table.read_padded(b, nmax, buf, max(1, args.workers))
        return buf

    predict = Predictor(model, args.half) if args.window is None else WindowPredictor(model, args)
    seg = _segments_file(args, name)
    speech = open(os.path.join(args.out_path, "speech_segments." + name), "w") if by_segment else None
    with open(os.path.join(args.out_path, name), "wb") as f, torch.no_grad(), ThreadPoolExecutor(1) as rd, \
            ThreadPoolExecutor(1) as wr:
        nxt = rd.submit(load, 0) if mine else None
        pending = None
        t0, done = time.time(), 0
        for n, (b, _) in enumerate(mine):
            buf = nxt.result()
            nxt = rd.submit(load, n + 1) if n + 1 < len(mine) else None
            wave = buf.cuda(args.gpu, non_blocking=True)
            out = frontend(wave, table.nsamp[b], [features.utt_id(keys[i]) for i in b], seed,
                           input_rate=int(table.rate[b[0]]))        # a batch holds files of one rate
            if by_segment:      # every frame is kept: the windows slide inside the speech segments, times stay the recording's
                feats, lengths = out[0], np.asarray(out[1], dtype=np.int64)
                segments = out[2] if args.vad_segments else _file_segments(args.file_segments, [keys[i] for i in b], lengths)
                for r in np.setdiff1d(np.arange(len(b)), segments[0]):
                    print("=> skipping {}: no speech segment".format(keys[b[r]]))
                pred, ks, seglines = predict(feats, lengths, [keys[i] for i in b], segments)
                speech.write("".join(predict.speech_lines))
                if pending is not None:
                    pending.result()
                pending = wr.submit(_emit, f, seg, ks, pred, seglines, args)
                done += len(b)
                continue
            feats, lengths = out
            keep = np.nonzero(lengths > 0)[0]
            for r in np.nonzero(lengths == 0)[0]:
                print("=> skipping {}: no voiced frames".format(keys[b[r]]))
            if keep.size == 0:
                continue
            if keep.size < len(b):
                feats = feats[torch.from_numpy(keep).to(feats.device)].contiguous()
            ks, seglines = [keys[b[r]] for r in keep], None
            if args.window is None:
                pred = predict(feats, lengths[keep])
            else:          # the windows count the frames the model sees: after the VAD's frame selection
                pred, ks, seglines = predict(feats, lengths[keep], ks)
            if pending is not None:
                pending.result()
            pending = wr.submit(_emit, f, seg, ks, pred, seglines, args)
            done += keep.size
        if pending is not None:
            pending.result()
        if seg is not None:
            seg.close()
        if speech is not None:
            speech.close()
        dt = time.time() - t0
        print("=> extracted {} utterances in {:.2f} s ({:.0f} utt/s, read + front end + predict + write)".format(
            done, dt, done / max(dt, 1e-9)))
    predict.report()


if __name__ == "__main__":
    main()
