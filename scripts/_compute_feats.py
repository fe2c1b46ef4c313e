"""What scripts/compute_fbank.py and scripts/compute_mfcc.py share: wav.scp -> Kaldi feature archives on the GPU.  The two scripts
differ in the feature config they take (--fbank-config / --mfcc-config) and in the kernel that runs (features.fbank / features.mfcc);
reading, augmentation, resampling, VAD, CMN, voiced-frame selection, compression and the files written are the same code."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_parser(kind):
    """the arguments of compute_<kind>.py, kind = "fbank" or "mfcc": the same but for the feature config"""
    parser = argparse.ArgumentParser(description="Kaldi-compatible %s / VAD / CMN on the GPU" % kind)
    parser.add_argument("wav_scp")
    parser.add_argument("out_dir")
    if kind == "fbank":
        parser.add_argument("--fbank-config", help="Kaldi config file of compute-fbank-feats options (conf/fbank.conf)")
    else:
        parser.add_argument("--mfcc-config", help="Kaldi config file of compute-mfcc-feats options (conf/mfcc.conf)")
    parser.add_argument("--vad-config", help="Kaldi config file of compute-vad options (conf/vad.conf)")
    parser.add_argument("--cmn-window", type=int, default=300, help="apply-cmvn-sliding --cmn-window (with --egs)")
    parser.add_argument("--egs", action="store_true", help="CMN'd, voiced frames only (prepare_feats_for_egs.sh); needs --vad-config")
    parser.add_argument("--batch-size", type=int, default=128)
    parser.add_argument("--seed", type=int, default=0, help="dither seed")
    parser.add_argument("--threads", type=int, default=4, help="WAV reader threads")
    parser.add_argument("--gpu", type=int, default=0)
    parser.add_argument("--allow-downsample", action="store_true", help="resample files above --sample-frequency instead of refusing them")
    parser.add_argument("--allow-upsample", action="store_true", help="resample files below --sample-frequency instead of refusing them")
    parser.add_argument("--speed", help="speed perturbation factor as a decimal, e.g. 0.9 or 1.1: keys become sp<F>-<utt>")
    parser.add_argument("--vad-scp", help="with --egs: vad.scp of 0/1 vectors per written key; the voiced frames come from it, not from compute-vad")
    parser.add_argument("--time-batches", action="store_true", help="also print the seconds the batch loop took (tools/augment_bench.py)")
    parser.add_argument("--compress", action="store_true", help="write feats.ark as Kaldi's one-byte compressed matrices ('CM ', what "
                        "Kaldi's own feature scripts write by default): a quarter of the bytes, lossy; compressed on the GPU")
    parser.add_argument("--utt2spk", help="with --speed: 'utt spk' lines; writes <out-dir>/utt2spk and <out-dir>/utt2uniq of the copies")
    return parser


def main(kind):
    """scripts/compute_fbank.py (kind "fbank") and scripts/compute_mfcc.py (kind "mfcc")"""
    name = "compute_" + kind
    parser = make_parser(kind)
    args = parser.parse_args()
    if args.egs and not args.vad_config and not args.vad_scp:
        parser.error("--egs needs --vad-config")
    if args.vad_scp and not args.egs:
        parser.error("--vad-scp needs --egs")
    if args.utt2spk and not args.speed:
        parser.error("--utt2spk needs --speed")
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    try:
        parsed = features.read_wav_scp(args.wav_scp)
        augmented = any(e.augmented for e in parsed[1])
    except ValueError as e:
        parser.error(str(e))
    if augmented and args.speed:
        parser.error("--speed does not combine with wav-reverberate entries in %s" % args.wav_scp)
    if args.speed and any(e.speed is not None for e in parsed[1]):
        parser.error("--speed does not combine with the `sox ... speed` entries in %s: their keys and factors are the wav.scp's own"
                     % args.wav_scp)
    torch.cuda.set_device(args.gpu)
    cmn_window = args.cmn_window if args.egs else 0
    if kind == "fbank":
        fb, vad_opts, cmn = features.options_from_configs(args.fbank_config, args.vad_config, cmn_window)
        compute = features.fbank
    else:
        fb, vad_opts, cmn = features.options_from_configs(None, args.vad_config, cmn_window, mfcc_config=args.mfcc_config or "")
        compute = features.mfcc
    fo = int(fb.sample_frequency)
    try:
        if args.speed:
            features.speed_rates(args.speed, fo)
        keys, table, batches, short = features.wav_scp_batches(parsed, fb, args.batch_size, args.allow_downsample,
                                                               args.allow_upsample, args.speed, augment=True, speed_entries=True)
    except ValueError as e:
        parser.error(str(e))
    vad_scp = dict(l.split(None, 1) for l in open(args.vad_scp) if l.strip()) if args.vad_scp else None
    utt2spk = dict(l.split()[:2] for l in open(args.utt2spk) if l.strip()) if args.utt2spk else None
    if args.speed:              # the written keys; the dither stream of a copy is keyed by its own key
        orig = keys
        keys = [features.speed_key(args.speed, k) for k in orig]

    def rate_in(i):             # the rate entry i is resampled FROM (to fo): --speed, or the factor of its own `sox ... speed` line
        f = args.speed or table.speed[i]
        return features.speed_rates(f, fo, int(table.rate[i]))[0] if f else int(table.rate[i])
    for i in short:
        print(name + ": skipping %s: %d samples at %d Hz, shorter than one frame (%d)" % (
            keys[i], features.num_resampled(int(table.nsamp[i]), rate_in(i), fo), fo, fb.frame_len))
    os.makedirs(args.out_dir, exist_ok=True)
    ark = os.path.abspath(os.path.join(args.out_dir, "feats.ark"))
    vark = os.path.abspath(os.path.join(args.out_dir, "vad.ark"))
    # each batch goes to the arks as soon as it reaches the host (batches come in length order); only (offsets, frames) per
    # utterance is kept, and feats.scp / vad.scp / utt2num_frames are written in wav.scp order at the end - an scp line may
    # point anywhere in its ark
    where = {}                  # utterance index -> (feats offset, frames, vad offset or None)
    clipped = 0                 # samples the 16-bit quantisation of augmented entries clipped
    write_vad = vad_opts is not None and not args.egs
    t_start = time.perf_counter()
    with torch.no_grad(), open(ark, "wb") as fa, open(vark if write_vad else os.devnull, "wb") as fv:
        for idx, nmax in batches:
            buf = torch.empty(len(idx), nmax).pin_memory()
            table.read_padded(idx, nmax, buf, args.threads)
            wave = buf.cuda(non_blocking=True)
            ids = [features.utt_id(keys[i]) for i in idx]
            if augmented:
                rir, noises, names = features.augment_inputs(table, idx)
                try:
                    wave, nclip = features.augment(wave, table.nsamp[idx], rir, noises, quantize=True,
                                                   sample_rate=int(table.rate[idx[0]]), names=names)
                except ValueError as e:
                    sys.exit(name + ": %s" % e)
                clipped += int(nclip.sum())
            wave, nsamp = features.resample(wave, table.nsamp[idx], rate_in(idx[0]), fo)     # one (rate, speed) per batch
            feats, T, loge = compute(wave, nsamp, fb, ids, args.seed)
            v = None
            if vad_scp is not None:
                vidx = np.zeros((len(idx), feats.shape[2]), dtype=np.int32)
                cnt = np.zeros(len(idx), dtype=np.int64)
                for r, i in enumerate(idx):
                    if keys[i] not in vad_scp:
                        sys.exit(name + ": %s has no entry in %s" % (keys[i], args.vad_scp))
                    vv = kaldi_io.read_vec_flt(vad_scp[keys[i]].strip())
                    if vv.shape[0] != T[r]:
                        sys.exit(name + ": %s has %d frames but its vector in %s has %d" % (keys[i], T[r], args.vad_scp,
                                                                                                 vv.shape[0]))
                    nz = np.nonzero(vv != 0)[0]
                    cnt[r] = nz.size
                    vidx[r, :nz.size] = nz
                feats, T = features.select_voiced(feats, T, torch.from_numpy(vidx).cuda(), cnt, cmn)
            elif vad_opts is not None:
                v, vidx, cnt = features.vad(loge, T, vad_opts)
                if args.egs:
                    feats, T = features.select_voiced(feats, T, vidx, cnt, cmn)
            if args.compress:       # after the CMN / voiced-frame selection: what is written is what gets compressed
                try:
                    mr, hd, cd = features.compress(feats, T)
                except ValueError as e:
                    fin = torch.isfinite(feats).all(dim=1).cpu().numpy()
                    bad = [keys[i] for r, i in enumerate(idx) if T[r] > 0 and not fin[r, :T[r]].all()]
                    sys.exit(name + ": --compress: non-finite feature value in %s (%s)" % (", ".join(bad) or "a batch", e))
                mr, hd, cd = mr.cpu().numpy(), hd.cpu().numpy(), cd.cpu().numpy()
            else:
                feats = feats.cpu().numpy()
            v = v.cpu().numpy() if write_vad else None
            for r, i in enumerate(idx):
                if T[r] == 0:
                    print(name + ": skipping %s: no voiced frames" % keys[i])
                    continue
                if args.compress:
                    off = kaldi_io.write_cm(fa, mr[r, 0], mr[r, 1], hd[r], cd[r, :, :T[r]], key=keys[i])
                else:
                    off = kaldi_io.write_mat(fa, np.ascontiguousarray(feats[r, :, :T[r]].T), key=keys[i])
                voff = None
                if write_vad:
                    fv.write((keys[i] + " ").encode())
                    voff = fv.tell()
                    kaldi_io.write_vec_flt(fv, v[r, :T[r]].astype(np.float32))
                where[i] = (off, int(T[r]), voff)
    t_batches = time.perf_counter() - t_start
    with open(os.path.join(args.out_dir, "feats.scp"), "w") as fs, \
            open(os.path.join(args.out_dir, "utt2num_frames"), "w") as fn:
        for i, k in enumerate(keys):
            if i in where:
                fs.write("%s %s:%d\n" % (k, ark, where[i][0]))
                fn.write("%s %d\n" % (k, where[i][1]))
    if write_vad:
        with open(os.path.join(args.out_dir, "vad.scp"), "w") as vs:
            for i, k in enumerate(keys):
                if i in where:
                    vs.write("%s %s:%d\n" % (k, vark, where[i][2]))
    if args.speed:
        done = [k for i, k in enumerate(orig) if i in where]
        u2s, u2u = features.speed_side_files(args.speed, done, utt2spk)
        open(os.path.join(args.out_dir, "utt2uniq"), "w").write(u2u)
        if u2s is not None:
            open(os.path.join(args.out_dir, "utt2spk"), "w").write(u2s)
    if augmented:
        print(name + ": %d samples clipped by the 16-bit quantisation of the augmented entries" % clipped)
    if args.time_batches:
        print(name + ": %.3f s for the batches" % t_batches)
    print(name + ": wrote %d of %d utterances to %s" % (len(where), len(keys), args.out_dir))
