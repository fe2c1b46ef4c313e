#!/usr/bin/env python3
"""wav.scp -> Kaldi feature archives on the GPU: what stage 1 of the reference's feature_pre.sh:77-104 makes with compute-fbank-feats
(+ compute-vad), and with --egs what local/nnet3/xvector/prepare_feats_for_egs.sh:68-70 makes (apply-cmvn-sliding
--norm-vars=false --center=true --cmn-window=W, then select-voiced-frames).

Writes <out-dir>/feats.ark + feats.scp ([T, F] float32 matrices that train_resnet.py / decode.py read), utt2num_frames, and with
--vad-config vad.ark + vad.scp (float vectors of 0/1 per frame; without --egs).  Utterances shorter than one frame and (--egs) without
voiced frames are reported and skipped.  Dither noise is keyed by (--seed, a stable hash of the utterance key): the features of an
utterance do not depend on its batch.

    python scripts/compute_fbank.py data/train/wav.scp out --fbank-config conf/fbank.conf --vad-config conf/vad.conf --egs
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

parser = argparse.ArgumentParser(description="Kaldi-compatible fbank / VAD / CMN on the GPU")
parser.add_argument("wav_scp")
parser.add_argument("out_dir")
parser.add_argument("--fbank-config", help="Kaldi config file of compute-fbank-feats options (conf/fbank.conf)")
parser.add_argument("--vad-config", help="Kaldi config file of compute-vad options (conf/vad.conf)")
parser.add_argument("--cmn-window", type=int, default=300, help="apply-cmvn-sliding --cmn-window (with --egs)")
parser.add_argument("--egs", action="store_true", help="CMN'd, voiced frames only (prepare_feats_for_egs.sh); needs --vad-config")
parser.add_argument("--batch-size", type=int, default=128)
parser.add_argument("--seed", type=int, default=0, help="dither seed")
parser.add_argument("--threads", type=int, default=4, help="WAV reader threads")
parser.add_argument("--gpu", type=int, default=0)


def main():
    args = parser.parse_args()
    if args.egs and not args.vad_config:
        parser.error("--egs needs --vad-config")
    import pytorch_kaldi_resnet_amd  # noqa: F401
    from pytorch_kaldi_resnet_amd import features, kaldi_io
    torch.cuda.set_device(args.gpu)
    fb, vad_opts, cmn = features.options_from_configs(args.fbank_config, args.vad_config, args.cmn_window if args.egs else 0)
    keys, table, batches, short = features.wav_scp_batches(args.wav_scp, fb, args.batch_size)
    for i in short:
        print("compute_fbank: skipping %s: %d samples, shorter than one frame (%d)" % (keys[i], table.nsamp[i], fb.frame_len))
    os.makedirs(args.out_dir, exist_ok=True)
    ark = os.path.abspath(os.path.join(args.out_dir, "feats.ark"))
    vark = os.path.abspath(os.path.join(args.out_dir, "vad.ark"))
    # each batch goes to the arks as soon as it reaches the host (batches come in length order); only (offsets, frames) per
    # utterance is kept, and feats.scp / vad.scp / utt2num_frames are written in wav.scp order at the end - an scp line may
    # point anywhere in its ark
    where = {}                  # utterance index -> (feats offset, frames, vad offset or None)
    write_vad = vad_opts is not None and not args.egs
    with torch.no_grad(), open(ark, "wb") as fa, open(vark if write_vad else os.devnull, "wb") as fv:
        for idx, nmax in batches:
            buf = torch.empty(len(idx), nmax).pin_memory()
            table.read_padded(idx, nmax, buf, args.threads)
            wave = buf.cuda(non_blocking=True)
            ids = [features.utt_id(keys[i]) for i in idx]
            feats, T, loge = features.fbank(wave, table.nsamp[idx], fb, ids, args.seed)
            v = None
            if vad_opts is not None:
                v, vidx, cnt = features.vad(loge, T, vad_opts)
                if args.egs:
                    feats, T = features.select_voiced(feats, T, vidx, cnt, cmn)
            feats = feats.cpu().numpy()
            v = v.cpu().numpy() if write_vad else None
            for r, i in enumerate(idx):
                if T[r] == 0:
                    print("compute_fbank: skipping %s: no voiced frames" % keys[i])
                    continue
                off = kaldi_io.write_mat(fa, np.ascontiguousarray(feats[r, :, :T[r]].T), key=keys[i])
                voff = None
                if write_vad:
                    fv.write((keys[i] + " ").encode())
                    voff = fv.tell()
                    kaldi_io.write_vec_flt(fv, v[r, :T[r]].astype(np.float32))
                where[i] = (off, int(T[r]), voff)
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
    print("compute_fbank: wrote %d of %d utterances to %s" % (len(where), len(keys), args.out_dir))


if __name__ == "__main__":
    main()
