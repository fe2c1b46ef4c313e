#!/bin/bash
# Scoring and report of the reference's test.sh (steps 12 and 13): cosine scores, optional adaptive S-norm, then the
# three-line report eer_<backend>[_adapt_snorm] (EER, minDCF at p-target 0.01 and 0.001).
# usage: ./test.sh <modeldir> <dir> <backend: cosine|snorm|plda> <stage> [trials]
#   <modeldir> holds mean.vec and test.iv (for plda also transform.mat and plda, from scripts/compute_lda.py and
#   scripts/compute_plda.py); <dir> receives the scores and the report and, for snorm, holds topk_mean_std.
#   SPK_SCORE_BACKEND=hip runs every step on the GPU (default host: the same files, byte for byte; plda: the same
#   scores to the rounding of its float32 stages).
#   SPK_CALIBRATION=<model> (scripts/calibrate.py train, one system): stage 12 also writes the calibrated scores <scores>_cal and
#   stage 13 the report <eer file>_cal: Cllr, minCllr and actDCF at p-target 0.01 and 0.001.
#   SPK_BOOTSTRAP=<R> (optionally SPK_BOOTSTRAP_UTT2SPK=<utt2spk>: resample speakers, not utterance ids): stage 13 also writes
#   <eer file>_ci, the report with a speaker-level bootstrap interval behind each number (scripts/bootstrap_ci.py).
set -e
here=$(cd "$(dirname "$0")" && pwd)

modeldir=$1
dir=$2
backend=$3
stage=$4
voxceleb1_trials=${5:-data/test/trials_e}
impl=${SPK_SCORE_BACKEND:-host}

if [ "$backend" == "plda" ]; then
  if [ ! -f "$modeldir/plda" ] || [ ! -f "$modeldir/transform.mat" ]; then
    echo "plda scoring needs $modeldir/transform.mat and $modeldir/plda: train them with scripts/compute_lda.py and" >&2
    echo "scripts/compute_plda.py (Kaldi's own binaries stay out of this project: see DESIGN.md section 7)" >&2
    exit 1
  fi
elif [ "$backend" != "cosine" ] && [ "$backend" != "snorm" ]; then
  echo "usage: $0 <modeldir> <dir> <cosine|snorm|plda> <stage> [trials]" >&2
  exit 1
fi

score_file=scores_$backend
eer_file=eer_$backend
mkdir -p $dir/log
if [ $stage -le 12 ] && [ $backend == 'plda' ]; then
  echo "plda scoring..."
  python $here/scripts/plda_score.py \
      --mean $modeldir/mean.vec \
      --transform $modeldir/transform.mat \
      --plda $modeldir/plda \
      --enroll $modeldir/test.iv \
      --test $modeldir/test.iv \
      --trials $voxceleb1_trials \
      --score-file $dir/$score_file --backend $impl > $dir/log/test_scoring.log
elif [ $stage -le 12 ]; then
  echo "cosine scoring..."
  python $here/scripts/cosine_score.py \
      --mean $modeldir/mean.vec \
      --enroll $modeldir/test.iv \
      --test $modeldir/test.iv \
      --trials $voxceleb1_trials \
      --score-file $dir/$score_file --backend $impl > $dir/log/test_scoring.log
  if [ $backend == 'snorm' ]; then
    echo "adptive S-norm..."
    python $here/scripts/adaptive_snorm.py \
        --enroll $dir/topk_mean_std \
        --test $dir/topk_mean_std \
        --score-in $dir/$score_file \
        --score-out $dir/${score_file}_adapt_snorm --backend $impl > $dir/log/adaptive_snorm.log
  fi
fi

if [ $backend == 'snorm' ]; then
  score_file=${score_file}_adapt_snorm
  eer_file=${eer_file}_adapt_snorm
fi

if [ -n "$SPK_CALIBRATION" ] && [ $stage -le 12 ]; then
  python $here/scripts/calibrate.py apply --model $SPK_CALIBRATION --scores $dir/$score_file \
      --score-out $dir/${score_file}_cal --backend $impl > $dir/log/calibrate.log
fi

if [ $stage -le 13 ]; then
  eer=`python $here/scripts/compute_eer.py --backend $impl $dir/$score_file $voxceleb1_trials 2> /dev/null`
  mindcf1=`python $here/scripts/compute_min_dcf.py --backend $impl --p-target 0.01 $dir/$score_file $voxceleb1_trials 2> /dev/null`
  mindcf2=`python $here/scripts/compute_min_dcf.py --backend $impl --p-target 0.001 $dir/$score_file $voxceleb1_trials 2> /dev/null`
  echo "EER: $eer%" > $dir/$eer_file
  echo "minDCF(p-target=0.01): $mindcf1" >> $dir/$eer_file
  echo "minDCF(p-target=0.001): $mindcf2" >> $dir/$eer_file
  echo "backend: $backend"
  cat $dir/$eer_file
  if [ -n "$SPK_CALIBRATION" ]; then
    python $here/scripts/compute_cllr.py --backend $impl $dir/${score_file}_cal $voxceleb1_trials > $dir/${eer_file}_cal 2> /dev/null
    cat $dir/${eer_file}_cal
  fi
  if [ -n "$SPK_BOOTSTRAP" ]; then
    python $here/scripts/bootstrap_ci.py --backend $impl --replicates $SPK_BOOTSTRAP \
        ${SPK_BOOTSTRAP_UTT2SPK:+--utt2spk $SPK_BOOTSTRAP_UTT2SPK} $dir/$score_file $voxceleb1_trials > $dir/${eer_file}_ci 2> /dev/null
    cat $dir/${eer_file}_ci
  fi
fi
