#!/usr/bin/env python3
"""wav.scp -> Kaldi feature archives on the GPU: what stage 1 of the reference's feature_pre.sh:77-104 makes with compute-fbank-feats
(+ compute-vad), and with --egs what local/nnet3/xvector/prepare_feats_for_egs.sh:68-70 makes (apply-cmvn-sliding
--norm-vars=false --center=true --cmn-window=W, then select-voiced-frames).

Writes <out-dir>/feats.ark + feats.scp ([T, F] float32 matrices that train_resnet.py / decode.py read; with --compress Kaldi's
one-byte compressed matrices, which they read as well - DESIGN.md section 6g), utt2num_frames, and with
--vad-config vad.ark + vad.scp (float vectors of 0/1 per frame; without --egs).  Utterances shorter than one frame and (--egs) without
voiced frames are reported and skipped.  Dither noise is keyed by (--seed, a stable hash of the utterance key): the features of an
utterance do not depend on its batch.

Files at another sample rate than --sample-frequency of the fbank config are an error unless --allow-downsample / --allow-upsample
(compute-fbank-feats' flags) is given; they are then resampled on the GPU with Kaldi's LinearResample.  --speed F writes the
speed-perturbed copy of the set as the reference's local/perturb_data_dir_speed.sh lays it out: keys sp<F>-<utt>, and with --utt2spk
the files utt2spk (sp<F>-<utt> sp<F>-<spk>) and utt2uniq (sp<F>-<utt> <utt>); one factor per run.  The audio is resampled from
F x rate to rate (LinearResample, where the shell script runs `sox speed`), the VAD sees the perturbed audio, and the dither is keyed
by the written key, so the copies of an utterance get different noise.  The wav.scp of a directory that
perturb_data_dir_speed.sh made (or of train plus its copies combined) is read as it stands: a `sox -t wav PATH -t wav - speed F |` line
is resampled by its own factor and written under its own key, so one command writes the archive, vad.scp and utt2num_frames that
train_resnet.py --wav-scp on the same wav.scp is compared against; --speed does not combine with such lines.

Entries that are the recipe's wav-reverberate commands (feature_pre.sh:109-167: the reverb, noise, music and babble copies that
steps/data/reverberate_data_dir.py and steps/data/augment_data_dir.py write; the grammar: features.parse_wav_entry) are applied on
the GPU (features.augment) and quantised to 16 bits as the pipe would, before resampling and the fbank; the number of samples the
quantisation clipped is reported.  The dither is keyed by the written key.  --speed is refused with such entries.  --vad-scp FILE
(with --egs) takes the voiced frames from that file's 0/1 vectors under the written keys instead of computing the VAD: the
recipe copies the clean set's vad.scp to the augmented copies.

    python scripts/compute_fbank.py data/train/wav.scp out --fbank-config conf/fbank.conf --vad-config conf/vad.conf --egs
    python scripts/compute_fbank.py data/train/wav.scp out_sp0.9 --speed 0.9 --utt2spk data/train/utt2spk --fbank-config ...
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _compute_feats  # noqa: E402

if __name__ == "__main__":
    _compute_feats.main("fbank")
