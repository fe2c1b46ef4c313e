"""Kaldi-compatible feature front end on the GPU: fbank (compute-fbank-feats), MFCC (compute-mfcc-feats), energy VAD (compute-vad),
centred sliding CMN (apply-cmvn-sliding --norm-vars=false --center=true) and voiced-frame selection (select-voiced-frames) - the Kaldi binaries of
stage 1 of the reference's feature_pre.sh:77-104 and of local/nnet3/xvector/prepare_feats_for_egs.sh:68-70.

The kernels are csrc/frontend.hip (include/spkhip.h: spk_fbank_fwd, spk_mfcc_fwd, spk_vad_count, spk_cmn_select) and csrc/resample.hip
(spk_resample_fwd: Kaldi's LinearResample, for audio at another sample rate and for speed perturbation) and csrc/augment.hip
(spk_augment_fwd: reverberation and additive noise, the wav-reverberate entries of the recipe's augmented wav.scp); this module parses Kaldi
config files, builds the window / twiddle / mel / resampling tables in fp64 and runs the launches.  Semantics and numerics: DESIGN.md "Feature front end".
Training from audio adds the span form of the two frame kernels (fbank_span / mfcc_span: the frames of a part of
an utterance, bit for bit the frames of the whole), pcm16_to_f32, AugmentPool (the device-resident form of WavAugmentation) and
ChunkFrontend, which ingest.WavTrainLoader runs on its copy stream.  Speed-perturbed entries (`sox ... speed F` lines of a wav.scp)
add the span form of the resampler (include/spkwav.h: resample_span, check_resample_spans - a span of the resampled signal from a
span of the file, bit for bit the samples of resample() on the whole file) and SpeedBatch, ChunkFrontend's per-batch speed plan.
Speech segments: SegmentOptions, vad_segments (spk_vad_segments: the VAD decisions of a batch -> speech segments, on
the device) and Frontend(..., segments=): all frames kept, the segments in frames of the recording - the front of the diarization chain.
The one deliberate difference from Kaldi: dither is a counter-based N(0,1) draw keyed by (seed, utt_id, frame, position), and the VAD
sees the same dithered frames as the fbank (Kaldi draws a second dither for its MFCC pass).
"""
import dataclasses
import fractions
import collections
import ctypes
import hashlib
import math
import re
import shlex

import numpy as np
import torch

from . import hip

FLT_EPSILON = 1.1920928955078125e-07
WINDOWS = ("hamming", "hanning", "povey", "rectangular", "blackman")


def _parse_bool(v):
    if v in ("true", "True", "1"):
        return True
    if v in ("false", "False", "0"):
        return False
    raise ValueError("not a boolean: %r" % v)


def parse_kaldi_config(path, fields):
    """'--name=value  # comment' lines of a Kaldi config file -> {field name: value} converted to the type of `fields`
    (a dict name -> default); unknown names are an error."""
    out = {}
    for n, line in enumerate(open(path), 1):
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        if not line.startswith("--") or "=" not in line:
            raise ValueError("%s:%d: expected --name=value, got %r" % (path, n, line))
        name, val = line[2:].split("=", 1)
        key = name.strip().replace("-", "_")
        if key not in fields:
            raise ValueError("%s:%d: unknown option --%s" % (path, n, name.strip()))
        d = fields[key]
        val = val.strip()
        out[key] = _parse_bool(val) if isinstance(d, bool) else type(d)(val)
    return out


class _KaldiOptions:
    @classmethod
    def from_kaldi_config(cls, path, **overrides):
        defaults = {f.name: f.default for f in dataclasses.fields(cls)}
        kw = parse_kaldi_config(path, defaults)
        kw.update(overrides)
        return cls(**kw)


def _check_frame_and_mel_options(name, o):
    """the refusals FbankOptions and MfccOptions share (`name` is the class in the messages)"""
    if o.window_type not in WINDOWS:
        raise ValueError("%s: window_type %r (one of %s)" % (name, o.window_type, ", ".join(WINDOWS)))
    if o.num_mel_bins <= 3:
        raise ValueError("%s: num_mel_bins must be > 3" % name)
    if o.frame_len < 2 or o.frame_sh < 1:
        raise ValueError("%s: frame length %d / shift %d samples" % (name, o.frame_len, o.frame_sh))
    if o.padded_len > 1024:
        raise ValueError("%s: padded window of %d samples > 1024 is not supported" % (name, o.padded_len))
    if not 0.0 <= o.preemphasis_coefficient <= 1.0 or o.dither < 0 or o.energy_floor < 0:
        raise ValueError("%s: preemphasis_coefficient in [0, 1], dither >= 0, energy_floor >= 0" % name)
    nyq = 0.5 * o.sample_frequency
    hf = o.high_freq + nyq if o.high_freq <= 0 else o.high_freq
    if not (0.0 <= o.low_freq < nyq and 0.0 < hf <= nyq and o.low_freq < hf):
        raise ValueError("%s: low_freq %g / high_freq %g vs. Nyquist %g" % (name, o.low_freq, o.high_freq, nyq))


@dataclasses.dataclass
class FbankOptions(_KaldiOptions):
    """compute-fbank-feats options (Kaldi names and defaults)."""
    sample_frequency: float = 16000.0
    frame_length: float = 25.0
    frame_shift: float = 10.0
    dither: float = 1.0
    preemphasis_coefficient: float = 0.97
    remove_dc_offset: bool = True
    window_type: str = "povey"
    round_to_power_of_two: bool = True
    blackman_coeff: float = 0.42
    snip_edges: bool = True
    num_mel_bins: int = 23
    low_freq: float = 20.0
    high_freq: float = 0.0
    vtln_low: float = 100.0
    vtln_high: float = -500.0
    vtln_warp: float = 1.0
    energy_floor: float = 0.0
    raw_energy: bool = True
    use_energy: bool = False
    htk_compat: bool = False
    use_log_fbank: bool = True
    use_power: bool = True
    subtract_mean: bool = False

    def __post_init__(self):
        refuse = [("vtln_warp", self.vtln_warp != 1.0), ("use_energy", self.use_energy), ("htk_compat", self.htk_compat),
                  ("subtract_mean", self.subtract_mean), ("use_power=false", not self.use_power),
                  ("use_log_fbank=false", not self.use_log_fbank), ("raw_energy=false", not self.raw_energy),
                  ("round_to_power_of_two=false", not self.round_to_power_of_two)]
        for name, bad in refuse:
            if bad:
                raise ValueError("FbankOptions: %s is not supported by the GPU front end" % name)
        _check_frame_and_mel_options("FbankOptions", self)

    @property
    def frame_len(self):
        return int(self.sample_frequency * self.frame_length * 0.001)

    @property
    def frame_sh(self):
        return int(self.sample_frequency * self.frame_shift * 0.001)

    @property
    def padded_len(self):
        L = self.frame_len
        return 1 if L <= 1 else 2 ** (L - 1).bit_length()

    def num_frames(self, nsamp):
        """frame count of an utterance of nsamp samples (nsamp >= frame length)"""
        L, S = self.frame_len, self.frame_sh
        return 1 + (nsamp - L) // S if self.snip_edges else (nsamp + S // 2) // S


@dataclasses.dataclass
class MfccOptions(_KaldiOptions):
    """compute-mfcc-feats options (Kaldi names and defaults): the frame and mel options of FbankOptions, and the cepstral ones.
    The mel banks do not depend on htk_compat."""
    sample_frequency: float = 16000.0
    frame_length: float = 25.0
    frame_shift: float = 10.0
    dither: float = 1.0
    preemphasis_coefficient: float = 0.97
    remove_dc_offset: bool = True
    window_type: str = "povey"
    round_to_power_of_two: bool = True
    blackman_coeff: float = 0.42
    snip_edges: bool = True
    num_mel_bins: int = 23
    low_freq: float = 20.0
    high_freq: float = 0.0
    vtln_low: float = 100.0
    vtln_high: float = -500.0
    vtln_warp: float = 1.0
    num_ceps: int = 13
    use_energy: bool = True
    energy_floor: float = 0.0
    raw_energy: bool = True
    cepstral_lifter: float = 22.0
    htk_compat: bool = False
    subtract_mean: bool = False

    def __post_init__(self):
        refuse = [("vtln_warp", self.vtln_warp != 1.0), ("subtract_mean", self.subtract_mean),
                  ("raw_energy=false", not self.raw_energy), ("round_to_power_of_two=false", not self.round_to_power_of_two)]
        for name, bad in refuse:
            if bad:
                raise ValueError("MfccOptions: %s is not supported by the GPU front end" % name)
        _check_frame_and_mel_options("MfccOptions", self)
        if self.num_ceps < 1 or self.num_ceps > self.num_mel_bins:
            raise ValueError("MfccOptions: num_ceps %d must be in [1, num_mel_bins %d]" % (self.num_ceps, self.num_mel_bins))
        if not self.cepstral_lifter >= 0:
            raise ValueError("MfccOptions: cepstral_lifter %r must be >= 0" % (self.cepstral_lifter,))
        if self.num_mel_bins > self.padded_len:
            raise ValueError("MfccOptions: num_mel_bins %d above the padded window of %d samples" % (self.num_mel_bins, self.padded_len))

    # the derived sizes are FbankOptions' own: Frontend, wav_scp_batches and the resampler take either options object
    frame_len = FbankOptions.frame_len
    frame_sh = FbankOptions.frame_sh
    padded_len = FbankOptions.padded_len
    num_frames = FbankOptions.num_frames


@dataclasses.dataclass
class VadOptions(_KaldiOptions):
    """compute-vad options (Kaldi names and defaults)."""
    vad_energy_threshold: float = 5.0
    vad_energy_mean_scale: float = 0.5
    vad_frames_context: int = 0
    vad_proportion_threshold: float = 0.6

    def __post_init__(self):
        if self.vad_frames_context < 0 or self.vad_energy_mean_scale < 0:
            raise ValueError("VadOptions: vad_frames_context >= 0 and vad_energy_mean_scale >= 0")
        if not 0.0 < self.vad_proportion_threshold < 1.0:
            raise ValueError("VadOptions: vad_proportion_threshold in (0, 1)")


@dataclasses.dataclass
class CmnOptions(_KaldiOptions):
    """apply-cmvn-sliding options; only --norm-vars=false --center=true is supported, so center defaults to true here (Kaldi's
    default is false, which is refused)."""
    cmn_window: int = 600
    min_cmn_window: int = 100
    center: bool = True
    norm_vars: bool = False

    def __post_init__(self):
        if self.norm_vars:
            raise ValueError("CmnOptions: norm_vars=true is not supported")
        if not self.center:
            raise ValueError("CmnOptions: only center=true is supported (pass center=True, as the recipe does)")
        if self.cmn_window < 1:
            raise ValueError("CmnOptions: cmn_window >= 1")


@dataclasses.dataclass
class SegmentOptions:
    """VAD decisions -> speech segments (the rule: include/spkhip.h, spk_vad_segments), in frames: every run
    of voiced frames is padded by `padding` on both sides, runs whose padded ends are at most `max_gap` apart are joined, and a
    segment shorter than `min_length` is dropped.  The defaults are the project's choice, not a measurement."""
    padding: int = 10
    max_gap: int = 30
    min_length: int = 50

    def __post_init__(self):
        if self.padding < 0 or self.max_gap < 0 or self.min_length < 1:
            raise ValueError("SegmentOptions: padding >= 0, max_gap >= 0 and min_length >= 1")


# ---- host tables (fp64, rounded to fp32 once) ----
def window_function(opts, dtype=np.float64):
    L = opts.frame_len
    n = np.arange(L, dtype=np.float64)
    a = 2 * math.pi / (L - 1)
    if opts.window_type == "hanning":
        w = 0.5 - 0.5 * np.cos(a * n)
    elif opts.window_type == "hamming":
        w = 0.54 - 0.46 * np.cos(a * n)
    elif opts.window_type == "povey":
        w = (0.5 - 0.5 * np.cos(a * n)) ** 0.85
    elif opts.window_type == "rectangular":
        w = np.ones(L)
    else:
        w = opts.blackman_coeff - 0.5 * np.cos(a * n) + (0.5 - opts.blackman_coeff) * np.cos(2 * a * n)
    return w.astype(dtype)


def mel_scale(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_banks(opts):
    """[F][P/2] triangular filters in Kaldi's mel scale over FFT bins 0 .. P/2-1 (fp64)"""
    F, P, fs = opts.num_mel_bins, opts.padded_len, opts.sample_frequency
    nyq = 0.5 * fs
    hf = opts.high_freq + nyq if opts.high_freq <= 0 else opts.high_freq
    lo_mel, hi_mel = mel_scale(opts.low_freq), mel_scale(hf)
    delta = (hi_mel - lo_mel) / (F + 1)
    b = np.arange(F, dtype=np.float64)[:, None]
    left, center, right = lo_mel + b * delta, lo_mel + (b + 1) * delta, lo_mel + (b + 2) * delta
    mel = mel_scale((fs / P) * np.arange(P // 2, dtype=np.float64))[None, :]
    up = (mel - left) / (center - left)
    down = (right - mel) / (right - center)
    return np.maximum(0.0, np.minimum(up, down))


def dct_matrix(opts):
    """[C][F] rows of Kaldi's DCT-II (ComputeDctMatrix): D[0][n] = sqrt(1 / F), D[k][n] = sqrt(2 / F) cos(pi / F (n + 0.5) k) (fp64)"""
    C, F = opts.num_ceps, opts.num_mel_bins
    k = np.arange(C, dtype=np.float64)[:, None]
    n = np.arange(F, dtype=np.float64)[None, :]
    d = math.sqrt(2.0 / F) * np.cos(math.pi / F * (n + 0.5) * k)
    d[0, :] = math.sqrt(1.0 / F)
    return d


def lifter_coeffs(opts):
    """[C] 1 + Q / 2 sin(pi k / Q) for cepstral_lifter Q != 0, else ones (fp64)"""
    Q = float(opts.cepstral_lifter)
    k = np.arange(opts.num_ceps, dtype=np.float64)
    return 1.0 + 0.5 * Q * np.sin(math.pi * k / Q) if Q != 0 else np.ones(opts.num_ceps)


class _Tables:
    def __init__(self, opts, device):
        P = opts.padded_len
        self.window = torch.from_numpy(window_function(opts).astype(np.float32)).to(device)
        k = np.arange(P // 2, dtype=np.float64)
        tw = np.stack([np.cos(-2 * math.pi * k / P), np.sin(-2 * math.pi * k / P)], 1)
        self.twiddle = torch.from_numpy(tw.astype(np.float32).reshape(-1)).to(device)
        banks = mel_banks(opts)
        lo, off, ws = [], [0], []
        for m in range(banks.shape[0]):
            nz = np.nonzero(banks[m] > 0)[0]
            a, b = (int(nz[0]), int(nz[-1]) + 1) if nz.size else (0, 0)
            lo.append(a)
            ws.append(banks[m, a:b])
            off.append(off[-1] + (b - a))
        self.mel_w = torch.from_numpy(np.concatenate(ws + [np.zeros(1)]).astype(np.float32)).to(device)
        self.mel_lo = torch.tensor(lo, dtype=torch.int32, device=device)
        self.mel_off = torch.tensor(off, dtype=torch.int32, device=device)
        if isinstance(opts, MfccOptions):
            self.dct = torch.from_numpy(dct_matrix(opts).astype(np.float32)).to(device)
            self.lifter = torch.from_numpy(lifter_coeffs(opts).astype(np.float32)).to(device)


_TABLES = {}


def _tables(opts, device):
    key = (type(opts).__name__, dataclasses.astuple(opts), str(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = _Tables(opts, device)
    return t


def utt_id(key):
    """stable int64 id of an utterance key (the dither stream of that utterance: independent of batch, row, padding and rank)"""
    return int.from_bytes(hashlib.blake2b(key.encode(), digest_size=8).digest(), "little", signed=True)


def _host_ints(v, dtype=np.int64):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy().astype(dtype).reshape(-1)
    return np.asarray(v, dtype=dtype).reshape(-1)


# ---- Kaldi's one-byte compressed matrices ('CM '; csrc/cm.hip) ----
def compress(feats, T):
    """Kaldi's CompressedMatrix (format 'CM ': one byte per value) of every row of a batch of features, on the GPU.
    feats: float32 cuda [B, F, Tcap], T: frames per row (host or device ints in [0, Tcap]); whatever lies past T[b] is ignored.
    Returns cuda tensors (minrange [B, 2] float32, hdr [B, F, 4] int32 - the 16-bit column headers -, codes [B, F, Tcap] uint8, zero
    past T[b]): codes[b, :, :T[b]] is the column-major payload of the [T[b], F] matrix, kaldi_io.write_cm writes a record from these
    parts.  A row with T[b] = 0 has nothing written (zeros).  A row with a non-finite value (or whose range overflows float32) is
    refused: ValueError naming the row."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 3 or feats.dtype != torch.float32 or not feats.is_cuda:
        raise ValueError("compress: feats must be a float32 cuda tensor [B, F, Tcap]")
    B, F, Tcap = feats.shape
    n = _host_ints(T, np.int32)
    if n.size != B:
        raise ValueError("compress: %d frame counts for %d rows" % (n.size, B))
    if B == 0 or F == 0:
        raise ValueError("compress: empty batch [%d, %d, %d]" % (B, F, Tcap))
    if (n < 0).any() or (n > Tcap).any():
        bad = int(np.nonzero((n < 0) | (n > Tcap))[0][0])
        raise ValueError("compress: row %d has %d frames, outside [0, Tcap %d]" % (bad, int(n[bad]), Tcap))
    dev = feats.device
    minrange = torch.zeros(B, 2, device=dev)
    hdr = torch.zeros(B, F, 4, dtype=torch.int32, device=dev)
    codes = torch.zeros(B, F, Tcap, dtype=torch.uint8, device=dev)
    if Tcap == 0:
        return minrange, hdr, codes
    feats = feats.contiguous()
    tdev = torch.from_numpy(n).to(dev)
    ws = torch.empty(B, F, 2, device=dev)
    hip.call("spk_cm_compress", hip.ptr(feats), hip.ptr(tdev), B, F, Tcap, hip.ptr(ws), hip.ptr(minrange), hip.ptr(hdr), hip.ptr(codes),
             hip.stream())
    ok = torch.isfinite(minrange).all(dim=1).cpu().numpy()
    if not ok.all():
        bad = int(np.nonzero(~ok)[0][0])
        raise ValueError("compress: row %d holds a non-finite value (or its range overflows float32)" % bad)
    return minrange, hdr, codes


def column_headers(minrange, hdr):
    """the float32 values of 16-bit column headers: min + (range * 1.52590218966964e-05f) * p, every operation rounded to float32
    on its own (on the host: numpy never fuses).  minrange [B, 2], hdr [B, F, 4] (tensors or arrays) -> float32 array [B, F, 4]"""
    mr = minrange.detach().cpu().numpy() if isinstance(minrange, torch.Tensor) else np.asarray(minrange)
    h = hdr.detach().cpu().numpy() if isinstance(hdr, torch.Tensor) else np.asarray(hdr)
    mr = mr.astype(np.float32).reshape(-1, 1, 2)
    scale = mr[:, :, 1:2] * np.float32(1.52590218966964e-05)
    return (mr[:, :, 0:1] + scale * h.astype(np.float32)).astype(np.float32)


def decompress(codes, colhdr, lengths=None, out=None):
    """The GPU decode of 'CM ' codes.  codes: uint8 cuda [B, F, T] (as ArkTable.read_crop_codes / read_padded_codes or compress
    give them), colhdr: float32 cuda [B, F, 4], the decoded column headers (column_headers), lengths: None or per-row frame counts
    (cuda int32 tensor, or host ints).  Returns float32 [B, F, T] (into `out` when given: contiguous, 4-byte aligned), zero for
    t >= lengths[b]; the same bits as kaldi_io.read_mat of the record."""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 3 or codes.dtype != torch.uint8 or not codes.is_cuda:
        raise ValueError("decompress: codes must be a uint8 cuda tensor [B, F, T]")
    B, F, T = codes.shape
    if B == 0 or F == 0 or T == 0:
        raise ValueError("decompress: empty batch [%d, %d, %d]" % (B, F, T))
    if not isinstance(colhdr, torch.Tensor) or colhdr.dtype != torch.float32 or tuple(colhdr.shape) != (B, F, 4) or not colhdr.is_cuda:
        raise ValueError("decompress: colhdr must be a float32 cuda tensor [%d, %d, 4]" % (B, F))
    dev = codes.device
    if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda and lengths.dtype == torch.int32):
        lengths = torch.from_numpy(_host_ints(lengths, np.int32)).to(dev)
    if lengths is not None and lengths.numel() != B:
        raise ValueError("decompress: %d lengths for %d rows" % (lengths.numel(), B))
    if out is None:
        out = torch.empty(B, F, T, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, F, T) or not out.is_cuda:
        raise ValueError("decompress: out must be a float32 cuda tensor [%d, %d, %d]" % (B, F, T))
    hip.call("spk_cm_decode", hip.ptr(codes.contiguous()), hip.ptr(colhdr.contiguous()), hip.ptr(lengths), B, F, T, hip.ptr(out),
             hip.stream())
    return out


# ---- resampling (Kaldi's LinearResample; csrc/resample.hip) ----
LOWPASS_FILTER_WIDTH = 6        # zero crossings of the windowed sinc (Kaldi's ResampleWaveform)


def _int_rate(v, what):
    r = int(round(float(v)))
    if r <= 0 or r != float(v):
        raise ValueError("%s: sample rate %r must be a positive whole number of Hz" % (what, v))
    return r


def num_resampled(n, fi, fo):
    """LinearResample::GetNumOutputSamples: the number of outputs j with j / fo < n / fi (n: an int or an integer array)"""
    fi, fo = _int_rate(fi, "num_resampled"), _int_rate(fo, "num_resampled")
    g = math.gcd(fi, fo)
    iu, ou = fi // g, fo // g
    if isinstance(n, (int, np.integer)):
        return max(-((-int(n) * ou) // iu), 0)
    n = np.maximum(np.asarray(n, dtype=np.int64), 0)
    return -((-n * ou) // iu)


def _resample_first(fi, fo):
    """(iu, ou, K, first [ou], window width ww, cutoff fc): the cheap part of the table (no [ou][K] array yet)"""
    g = math.gcd(fi, fo)
    iu, ou = fi // g, fo // g
    fc = 0.99 * 0.5 * min(fi, fo)
    ww = LOWPASS_FILTER_WIDTH / (2.0 * fc)
    t = np.arange(ou, dtype=np.float64) / fo
    first = np.ceil((t - ww) * fi)
    last = np.floor((t + ww) * fi)
    return iu, ou, int((last - first + 1).max()), first, ww, fc


def _resample_tables(fi, fo):
    iu, ou, K, first, ww, fc = _resample_first(fi, fo)
    t = np.arange(ou, dtype=np.float64) / fo
    dt = (first[:, None] + np.arange(K, dtype=np.float64)[None, :]) / fi - t[:, None]
    w = np.where(np.abs(dt) < ww, 0.5 * (1 + np.cos(2 * math.pi * fc / LOWPASS_FILTER_WIDTH * dt)), 0.0)
    zero = dt == 0.0
    w = w * np.where(zero, 2 * fc, np.sin(2 * math.pi * fc * dt) / (math.pi * np.where(zero, 1.0, dt)))
    return iu, ou, K, first.astype(np.int64), w / fi


class _ResampleTables:
    def __init__(self, fi, fo, device):
        self.iu, self.ou, self.K, self.first, self.w = _resample_tables(fi, fo)
        self.first_dev = self.wq_dev = None
        if device is not None:
            # the kernel reads the weights as pairs of consecutive taps, the phase running fastest ([ceil(K / 2)][ou][2], an odd
            # K padded with a zero tap): consecutive outputs, consecutive LDS banks
            K2 = (self.K + 1) // 2
            wp = np.zeros((self.ou, 2 * K2), dtype=np.float32)
            wp[:, :self.K] = self.w.astype(np.float32)
            self.first_dev = torch.from_numpy(self.first.astype(np.int32)).to(device)
            self.wq_dev = torch.from_numpy(np.ascontiguousarray(wp.reshape(self.ou, K2, 2).transpose(1, 0, 2))).to(device)


_RESAMPLE_TABLES = {}


def _resample_cached(fi, fo, device):
    key = (fi, fo, None if device is None else str(device))
    t = _RESAMPLE_TABLES.get(key)
    if t is None:
        t = _RESAMPLE_TABLES[key] = _ResampleTables(fi, fo, device)
    return t


def resample_tables(fi, fo, device=None):
    """(iu, ou, K, first [ou] int64, w [ou][K] fp64) of Kaldi's LinearResample from fi to fo Hz: output j of a signal x is
    sum_k w[j % ou][k] * x[first[j % ou] + (j // ou) * iu + k].  Cached per (fi, fo, device); with a device the fp32 copies the
    kernel reads are cached next to them."""
    fi, fo = _int_rate(fi, "resample_tables"), _int_rate(fo, "resample_tables")
    t = _resample_cached(fi, fo, device)
    return t.iu, t.ou, t.K, t.first, t.w


def speed_rates(speed, rate, input_rate=None):
    """Speed perturbation by `speed` (a decimal string such as "0.9", or a Fraction) of audio that the front end reads at `rate` Hz,
    recorded at input_rate (default: rate): the (fi, fo) of the one resampling that does it, fi = input_rate * speed -> fo = rate.
    Read at fo, the result is 1 / speed times as long.  speed == 1 and a fractional fi are refused."""
    if isinstance(speed, float):
        raise ValueError("speed: pass the factor as a decimal string or a Fraction, not the float %r" % speed)
    try:
        f = fractions.Fraction(speed)
    except (ValueError, TypeError, ZeroDivisionError):
        raise ValueError("speed: %r is not a decimal factor such as '0.9'" % (speed,))
    if f <= 0:
        raise ValueError("speed: factor %s must be positive" % f)
    if f == 1:
        raise ValueError("speed: factor 1 is no perturbation")
    fo = _int_rate(rate, "speed")
    fi = _int_rate(fo if input_rate is None else input_rate, "speed") * f
    if fi.denominator != 1:
        raise ValueError("speed: %s x %s Hz = %s is not a whole number of Hz" % (f, fo if input_rate is None else input_rate, fi))
    return int(fi), fo


def resample(wave, nsamp, fi, fo):
    """Kaldi's ResampleWaveform on the GPU.  wave: float32 cuda [B, Nmax] at int16 scale, nsamp: per-row sample counts (host or
    device ints, each in [1, Nmax]), fi -> fo: whole rates in Hz.  Returns (wave_out [B, max n_out] cuda, zeros past each row's
    count; nsamp_out int64 host array = num_resampled(nsamp, fi, fo)).  fi == fo returns (wave, nsamp) as they came."""
    fi, fo = _int_rate(fi, "resample"), _int_rate(fo, "resample")
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
        raise ValueError("resample: wave must be a float32 cuda tensor [B, Nmax]")
    B, Nmax = wave.shape
    n = _host_ints(nsamp)
    if n.size != B:
        raise ValueError("resample: %d sample counts for %d rows" % (n.size, B))
    if B == 0 or Nmax == 0:
        raise ValueError("resample: empty batch [%d, %d]" % (B, Nmax))
    if (n < 1).any() or (n > Nmax).any():
        bad = int(np.nonzero((n < 1) | (n > Nmax))[0][0])
        raise ValueError("resample: row %d has %d samples, outside [1, Nmax %d]" % (bad, int(n[bad]), Nmax))
    if fi == fo:
        return wave, nsamp
    iu, ou, K = _resample_first(fi, fo)[:3]
    if hip.lib().spk_resample_tile(iu, ou, K) == 0:      # before the table is built and before any launch
        raise ValueError("resample: %d -> %d Hz needs a filter table of %d phases x %d taps, beyond the LDS budget of the kernel "
                         "(rates with a larger common divisor have fewer phases)" % (fi, fo, ou, K))
    wave = wave.contiguous()
    dev = wave.device
    tab = _resample_cached(fi, fo, dev)
    n_out = num_resampled(n, fi, fo)
    Nout = int(n_out.max())
    ns = torch.from_numpy(n.astype(np.int32)).to(dev)
    out = torch.empty(B, Nout, device=dev)
    nd = torch.empty(B, dtype=torch.int32, device=dev)
    hip.call("spk_resample_fwd", hip.ptr(wave), hip.ptr(ns), B, Nmax, hip.ptr(tab.first_dev), hip.ptr(tab.wq_dev), fi, fo, tab.K,
             hip.ptr(out), hip.ptr(nd), Nout, hip.stream())
    return out, n_out


# ---- the span form of the resampler (include/spkwav.h; DESIGN.md sections 6e "Resampling" and 6k) ----
def check_speed_table(what, fi, fo):
    """refuse, before any launch, a resampling whose filter table exceeds the LDS budget of the kernel (`what` names the entry)"""
    iu, ou, K = _resample_first(fi, fo)[:3]
    if hip.lib().spk_resample_tile(iu, ou, K) == 0:
        raise ValueError("%s: resampling %d -> %d Hz needs a filter table of %d phases x %d taps, beyond the LDS budget of the kernel "
                         "(rates with a larger common divisor have fewer phases)" % (what, fi, fo, ou, K))


def check_resample_spans(what, fi, fo, icount, ifirst, itotal, ofirst, ocount, Nmax_in, Nmax_out, rows=None):
    """the refusals of resample_span, on host arrays, before any launch: every row (of `rows`: the others are not looked at) is a
    part of its utterance, its outputs exist, and the row holds every sample of the utterance that ingest.resample_input_span
    names for those outputs - the union of their windows with its margin.  Returns the five arrays as int64."""
    from . import ingest
    c, f, N, o, m = (_host_ints(v) for v in (icount, ifirst, itotal, ofirst, ocount))
    B = c.size
    if not (f.size == N.size == o.size == m.size == B):
        raise ValueError("%s: icount, ifirst, itotal, ofirst and ocount must have one entry per row (%d rows)" % (what, B))
    sel = np.arange(B) if rows is None else _host_ints(rows)
    if sel.size == 0 or (sel < 0).any() or (sel >= B).any() or np.unique(sel).size != sel.size:
        raise ValueError("%s: the row list must name distinct rows in [0, %d)" % (what, B))

    def bad(mask, msg):
        if mask[sel].any():
            b = int(sel[np.nonzero(mask[sel])[0][0]])
            raise ValueError("%s: row %d (samples %d .. +%d of an utterance of %d, outputs %d .. +%d): %s"
                             % (what, b, int(f[b]), int(c[b]), int(N[b]), int(o[b]), int(m[b]), msg))
    bad((N < 1) | (N >= 2 ** 30), "utterance length outside [1, 2^30)")
    n_out = num_resampled(np.where((N < 1) | (N >= 2 ** 30), 1, N), fi, fo)
    bad(n_out >= 2 ** 30, "the resampled utterance has 2^30 samples or more")
    bad((c < 1) | (c > Nmax_in), "sample count outside [1, Nmax_in %d]" % Nmax_in)
    bad((f < 0) | (f + c > N), "the row is not a part of the utterance")
    bad((m < 1) | (m > Nmax_out), "output count outside [1, Nmax_out %d]" % Nmax_out)
    bad((o < 0) | (o + m > n_out), "outputs outside the resampled utterance's")
    need_first, need_count = ingest.resample_input_span(np.where(o < 0, 0, o), np.maximum(m, 1), N, fi, fo)
    bad((need_first < f) | (need_first + need_count > f + c), "an output needs a sample of the utterance outside the row")
    return c, f, N, o, m


def _resample_span_launch(wave, ifirst, icount, itotal, ofirst, ocount, rows, fi, fo, out):
    """the span launch on device arguments alone (no check of their values, nothing read back): wave [B, Nmax_in] and out
    [B, Nmax_out] float32, ifirst / itotal / ofirst int64 [B], icount / ocount int32 [B], rows int32 [R] or None"""
    B, Nmax_in = wave.shape
    tab = _resample_cached(fi, fo, wave.device)
    hip.call("spkw_resample_span_fwd", hip.ptr(wave), hip.ptr(ifirst), hip.ptr(icount), hip.ptr(itotal), hip.ptr(ofirst),
             hip.ptr(ocount), hip.ptr(rows), B if rows is None else rows.numel(), B, Nmax_in, hip.ptr(tab.first_dev),
             hip.ptr(tab.wq_dev), fi, fo, tab.K, hip.ptr(out), out.shape[1], hip.stream())
    return out


def _copy_rows_launch(wave, count, rows, out):
    """rows of a batch that are not resampled: wave[b, :count[b]] into out[b], zeros behind (device arguments alone)"""
    B, Nmax_in = wave.shape
    hip.call("spkw_copy_rows_fwd", hip.ptr(wave), hip.ptr(count), hip.ptr(rows), B if rows is None else rows.numel(), B, Nmax_in,
             hip.ptr(out), out.shape[1], hip.stream())
    return out


def resample_span(wave, icount, ifirst, itotal, ofirst, ocount, fi, fo, rows=None, out=None):
    """A span of the resampled signal from a span of the utterance, equal bit for bit to the same samples of resample() on the
    whole utterance.  Row b of wave (float32 cuda [B, Nmax_in], contiguous or a view whose rows are) holds samples ifirst[b] ..
    ifirst[b] + icount[b] - 1 of an utterance of itotal[b] samples; written are outputs ofirst[b] .. ofirst[b] + ocount[b] - 1 of
    that utterance resampled from fi to fo Hz, zeros behind them.  All five are host integers per row.  rows: the rows to work on
    (host ints; the others are neither checked nor touched); out: float32 cuda [B, Nmax_out] to write into (default: a new
    tensor with Nmax_out = the largest ocount of the rows, zero in the other rows).  Refused before any launch
    (check_resample_spans): outputs that the resampled utterance does not have, a row that lacks a sample its outputs need
    (ingest.resample_input_span gives the samples an output range needs), lengths at or above 2^30, a table beyond the kernel's
    LDS budget."""
    fi, fo = _int_rate(fi, "resample_span"), _int_rate(fo, "resample_span")
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
        raise ValueError("resample_span: wave must be a float32 cuda tensor [B, Nmax_in]")
    if fi == fo:
        raise ValueError("resample_span: %d -> %d Hz is no resampling" % (fi, fo))
    B, Nmax_in = wave.shape
    if B == 0 or Nmax_in == 0:
        raise ValueError("resample_span: empty batch [%d, %d]" % (B, Nmax_in))
    check_speed_table("resample_span", fi, fo)
    sel = None if rows is None else _host_ints(rows)
    m = _host_ints(ocount)
    if out is None:
        Nmax_out = int(m.max() if sel is None else m[sel[(sel >= 0) & (sel < m.size)]].max()) if m.size else 0
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or not out.is_cuda \
            or not out.is_contiguous():
        raise ValueError("resample_span: out must be a contiguous float32 cuda tensor [%d, Nmax_out]" % B)
    else:
        Nmax_out = out.shape[1]
    c, f, N, o, m = check_resample_spans("resample_span", fi, fo, icount, ifirst, itotal, ofirst, ocount, Nmax_in, max(Nmax_out, 1), sel)
    if not wave.is_contiguous():
        wave = wave.contiguous()
    dev = wave.device

    def dv(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    if out is None:
        out = torch.zeros(B, Nmax_out, device=dev)
    return _resample_span_launch(wave, dv(f, np.int64), dv(c, np.int32), dv(N, np.int64), dv(o, np.int64), dv(m, np.int32),
                                 None if sel is None else dv(sel, np.int32), fi, fo, out)


# ---- augmentation (the recipe's wav-reverberate entries; csrc/augment.hip) ----
AUGMENT_FFT = 2048              # FFT size of the partitioned convolution (blocks of 1024 samples)
_AUG_TWIDDLE = {}


def _aug_twiddle(device):
    t = _AUG_TWIDDLE.get(str(device))
    if t is None:
        k = np.arange(AUGMENT_FFT // 2, dtype=np.float64)
        tw = np.stack([np.cos(-2 * math.pi * k / AUGMENT_FFT), np.sin(-2 * math.pi * k / AUGMENT_FFT)], 1)
        t = _AUG_TWIDDLE[str(device)] = torch.from_numpy(tw.astype(np.float32).reshape(-1)).to(device)
    return t


def early_window(h, sample_rate):
    """(s, e0, e1) of an impulse response h at sample_rate Hz: the peak s (the first maximum of the signed value) and the early
    part h[e0:e1] = h[max(0, s - int(0.001 fs)) : min(R, s + int(0.05 fs))] whose output power is the signal power of the SNRs"""
    s = int(np.argmax(h))
    return s, max(0, s - int(0.001 * sample_rate)), min(len(h), s + int(0.05 * sample_rate))


def _aug_samples(v, what):
    v = np.asarray(v)
    if v.ndim != 1 or v.dtype != np.float32:
        raise ValueError("augment: %s must be a one-dimensional float32 array, not %s%s" % (what, v.dtype, list(v.shape)))
    if v.size == 0:
        raise ValueError("augment: %s is empty" % what)
    return v


def augment(wave, nsamp, rir=None, noises=None, quantize=False, sample_rate=16000, names=None):
    """Reverberation and additive noise as Kaldi's `wav-reverberate --shift-output=true` applies them (the contract: DESIGN.md
    section 6f, restated in tests/augment_ref.py).  wave: float32 cuda [B, Nmax] at int16 scale, nsamp: per-row sample counts.
    rir: per row a float32 array (the impulse response, any scale) or None.  noises: per row a list of (samples float32 array,
    duration in seconds or None, start in seconds, snr in dB), added in order; a duration repeats or cuts the samples to
    int(sample_rate * duration).  quantize: truncate toward zero and clip to [-32768, 32767], what a 16-bit WAV pipe carries.
    Returns (wave_out [B, Nmax] cuda with zeros past each row's count, clipped int64 host array: the samples quantize clipped per
    row).  A row with neither an impulse response nor a noise comes back as it went in (quantised, if asked).  names: per row a
    label (the file) for the error messages.  Everything is refused here, before any launch."""
    if not isinstance(wave, torch.Tensor) or wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
        raise ValueError("augment: wave must be a float32 cuda tensor [B, Nmax]")
    B, Nmax = wave.shape
    n = _host_ints(nsamp)
    if n.size != B:
        raise ValueError("augment: %d sample counts for %d rows" % (n.size, B))
    if B == 0 or Nmax == 0:
        raise ValueError("augment: empty batch [%d, %d]" % (B, Nmax))
    if (n < 1).any() or (n > Nmax).any():
        bad = int(np.nonzero((n < 1) | (n > Nmax))[0][0])
        raise ValueError("augment: row %d has %d samples, outside [1, Nmax %d]" % (bad, int(n[bad]), Nmax))
    rir = [None] * B if rir is None else list(rir)
    noises = [[]] * B if noises is None else [list(v) if v is not None else [] for v in noises]
    if len(rir) != B or len(noises) != B:
        raise ValueError("augment: %d impulse responses and %d noise lists for %d rows" % (len(rir), len(noises), B))
    fs = float(sample_rate)
    if not (math.isfinite(fs) and fs > 0):
        raise ValueError("augment: sample_rate %r" % (sample_rate,))
    label = (lambda b: "row %d (%s)" % (b, names[b])) if names is not None else (lambda b: "row %d" % b)
    lib = hip.lib()
    max_rir, max_early = lib.spk_augment_max_rir(), lib.spk_augment_max_early()
    rir_off, rir_row, rir_parts, pos = np.zeros(B, dtype=np.int64), np.zeros((B, 4), dtype=np.int32), [], 0
    for b, h in enumerate(rir):
        if h is None:
            continue
        h = _aug_samples(h, "the impulse response of %s" % label(b))
        if h.size > max_rir:
            raise ValueError("augment: the impulse response of %s has %d samples, more than the %d the kernel is built for"
                             % (label(b), h.size, max_rir))
        s, e0, e1 = early_window(h, fs)
        if not 1 <= e1 - e0 <= max_early:
            raise ValueError("augment: the early part of the impulse response of %s has %d samples at %g Hz, outside [1, %d]"
                             % (label(b), e1 - e0, fs, max_early))
        rir_off[b], rir_row[b] = pos, (h.size, s, e0, e1 - e0)
        rir_parts.append(h)
        pos += h.size
    desc_ptr, d_off, d_len, d_snr, n_parts, npos, seen, nonzero = [0], [], [], [], [], 0, {}, {}
    for b, lst in enumerate(noises):
        for item in lst:
            if len(item) != 4:
                raise ValueError("augment: a noise of %s is not (samples, duration, start, snr)" % label(b))
            r, duration, start, snr = item
            r = _aug_samples(r, "a noise of %s" % label(b))
            if id(r) not in seen:
                seen[id(r)] = npos
                n_parts.append(r)
                npos += r.size
            if not (isinstance(snr, (int, float, np.integer, np.floating)) and math.isfinite(snr)):
                raise ValueError("augment: a noise of %s has the non-finite SNR %r" % (label(b), snr))
            if not (math.isfinite(start) and start >= 0):
                raise ValueError("augment: a noise of %s starts at %r s (negative or not finite)" % (label(b), start))
            fill = r.size if duration is None else int(fs * duration) if math.isfinite(duration) else 0
            if not 1 <= fill < 2 ** 30 or start * fs >= 2 ** 30:
                raise ValueError("augment: a noise of %s with duration %r s and start %r s gives %d samples from sample %d"
                                 % (label(b), duration, start, fill, int(min(start * fs, 2.0 ** 62))))
            if (id(r), min(fill, r.size)) not in nonzero:       # q_k is the power of what is added: the filled signal
                nonzero[(id(r), min(fill, r.size))] = bool(np.any(r[:fill]))
            if not nonzero[(id(r), min(fill, r.size))]:
                raise ValueError("augment: a noise of %s is all zero over the %d samples that are added (its power scales "
                                 "the SNR)" % (label(b), min(fill, r.size)))
            d_off.append(seen[id(r)])
            d_len.append((r.size, fill, int(start * fs)))
            d_snr.append(float(snr))
        desc_ptr.append(len(d_off))
    nd = len(d_off)
    if B + nd > 65535:
        raise ValueError("augment: %d rows with %d noises in one call (at most 65535 together)" % (B, nd))
    Rmax = int(rir_row[:, 0].max())
    Emax = int(rir_row[:, 3].max())
    Fmax = max([v[1] for v in d_len], default=0)
    sizes = (ctypes.c_longlong * 3)()
    hip.call("spk_augment_workspace", B, Nmax, Rmax, Emax, Fmax, nd, sizes)
    wave = wave.contiguous()
    dev = wave.device

    def dv(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    ns = dv(n, np.int32)
    rpool = dv(np.concatenate(rir_parts), np.float32) if rir_parts else None
    npool = dv(np.concatenate(n_parts), np.float32) if n_parts else None
    spectra = torch.empty(2 * sizes[0], device=dev) if sizes[0] else None
    y = torch.empty(max(sizes[1], 1), device=dev)
    work = torch.empty(max(sizes[2], 1), dtype=torch.float64, device=dev)
    out = torch.empty(B, Nmax, device=dev)
    clipped = torch.zeros(B, dtype=torch.int64, device=dev)
    t_off, t_row, t_ptr = dv(rir_off, np.int64), dv(rir_row, np.int32), dv(desc_ptr, np.int32)
    t_doff = dv(d_off, np.int64) if nd else None
    t_dlen = dv(np.asarray(d_len).reshape(-1), np.int32) if nd else None
    t_dsnr = dv(d_snr, np.float64) if nd else None
    hip.call("spk_augment_fwd", hip.ptr(wave), hip.ptr(ns), B, Nmax, hip.ptr(rpool), pos, hip.ptr(t_off), hip.ptr(t_row), Rmax, Emax,
             hip.ptr(npool), npos, hip.ptr(t_ptr), hip.ptr(t_doff), hip.ptr(t_dlen), hip.ptr(t_dsnr), nd, Fmax,
             hip.ptr(_aug_twiddle(dev)) if Rmax else None, hip.ptr(spectra), hip.ptr(y), hip.ptr(work), int(bool(quantize)),
             hip.ptr(out), hip.ptr(clipped), hip.stream())
    return out, clipped.cpu().numpy()


WavEntry = collections.namedtuple("WavEntry", "path rir_path noises augmented speed", defaults=(None,))
WavEntry.__doc__ = """one wav.scp entry: the speech file, the impulse-response file or None, the additive signals
[(path, duration or None, start seconds, snr dB)], whether any of these is applied at all, and the speed factor of a `sox ... speed F`
entry as the decimal string F (None: the file as it is; such an entry is never augmented)"""


def _pipe_error(text, why):
    return ValueError("wav.scp pipe entry not supported (%s): %r" % (why, text))


def _reverberate_options(tokens, text, top):
    """{name: value} of the --name=value tokens of one wav-reverberate command; `top`: the options of an entry, else of an item"""
    allowed = ("shift-output", "impulse-response", "additive-signals", "start-times", "snrs") if top else ("duration",)
    out = {}
    for t in tokens:
        if not t.startswith("--") or "=" not in t:
            raise _pipe_error(text, "expected --name=value, got %r" % t)
        name, val = t[2:].split("=", 1)
        if name not in allowed or name in out:
            raise _pipe_error(text, "option --%s" % name)
        out[name] = val
    return out


def _floats(val, what, text):
    try:
        return [float(v) for v in val.split(",")]
    except ValueError:
        raise _pipe_error(text, "%s %r" % (what, val))


def parse_wav_entry(text):
    """The value of a wav.scp line -> WavEntry.  Accepted are a plain path and exactly the commands the recipe's two scripts
    write (the reference's feature_pre.sh:109-167):
        cat PATH | wav-reverberate --shift-output=true [--impulse-response="RIR"] [--additive-signals= --start-times= --snrs=] - - |
                                      (steps/data/reverberate_data_dir.py:345,365; augment_data_dir.py:116 on such a `cat` entry)
        wav-reverberate --shift-output=true --additive-signals='ITEM,..' --start-times='..' --snrs='..' PATH - |
                                                                            (steps/data/augment_data_dir.py:112)
    with ITEM a plain path or `wav-reverberate --duration=D "PATH" - |` (augment_data_dir.py:87-88), and the speed-perturbed copy
        sox -t wav PATH -t wav - speed F |                 (local/perturb_data_dir_speed.sh:83,95 on a plain path)
    with F a decimal string, kept as a string in WavEntry.speed (a factor equal to 1 is the plain file).  Everything else - another
    command, another pipe in front, --shift-output=false, a top-level --duration, an impulse response inside an item, an unknown
    option, lists of unequal length - is a ValueError that says `pipe` and quotes the entry."""
    text = text.strip()
    if not text.endswith("|"):
        return WavEntry(text, None, [], False)
    try:
        tok = shlex.split(text)
    except ValueError as e:
        raise _pipe_error(text, str(e))
    if len(tok) >= 7 and tok[0] == "cat" and tok[2] == "|" and tok[3] == "wav-reverberate" and tok[-3:] == ["-", "-", "|"]:
        path, opts = tok[1], _reverberate_options(tok[4:-3], text, True)
        if "impulse-response" not in opts and "additive-signals" not in opts:
            raise _pipe_error(text, "neither --impulse-response nor --additive-signals")
    elif len(tok) >= 5 and tok[0] == "wav-reverberate" and tok[-2:] == ["-", "|"] and not tok[-3].startswith("-"):
        path, opts = tok[-3], _reverberate_options(tok[1:-3], text, True)
        if "impulse-response" in opts or "additive-signals" not in opts:
            raise _pipe_error(text, "expected --additive-signals and no --impulse-response")
    elif len(tok) == 10 and tok[:3] == ["sox", "-t", "wav"] and tok[4:8] == ["-t", "wav", "-", "speed"] and tok[9] == "|":
        path, factor = tok[3], tok[8]
        if "|" in path or not path or path.startswith("-"):
            raise _pipe_error(text, "speech file %r" % path)
        if not re.fullmatch(r"[0-9]+(\.[0-9]*)?|\.[0-9]+", factor) or fractions.Fraction(factor) <= 0:
            raise _pipe_error(text, "speed factor %r" % factor)
        return WavEntry(path, None, [], False, None if fractions.Fraction(factor) == 1 else factor)
    else:
        raise _pipe_error(text, "not one of the wav-reverberate forms of the recipe")
    if "|" in path or not path:
        raise _pipe_error(text, "speech file %r" % path)
    if opts.get("shift-output") != "true":
        raise _pipe_error(text, "--shift-output=%s" % opts.get("shift-output", "false (the default)"))
    noises = []
    if "additive-signals" in opts:
        if "start-times" not in opts or "snrs" not in opts:
            raise _pipe_error(text, "--additive-signals needs --start-times and --snrs")
        items = [v.strip() for v in opts["additive-signals"].split(",")]
        starts, snrs = _floats(opts["start-times"], "--start-times", text), _floats(opts["snrs"], "--snrs", text)
        if not len(items) == len(starts) == len(snrs):
            raise _pipe_error(text, "%d signals, %d start times, %d SNRs" % (len(items), len(starts), len(snrs)))
        for item, start, snr in zip(items, starts, snrs):
            duration = None
            if item.endswith("|"):
                try:
                    it = shlex.split(item)
                except ValueError as e:
                    raise _pipe_error(text, str(e))
                if len(it) != 5 or it[0] != "wav-reverberate" or it[3:] != ["-", "|"] or it[2].startswith("-"):
                    raise _pipe_error(text, "additive signal %r" % item)
                d = _floats(_reverberate_options(it[1:2], text, False).get("duration", ""), "--duration", text)
                duration, item = d[0], it[2]
            if not item or " " in item or "|" in item:
                raise _pipe_error(text, "additive signal %r" % item)
            noises.append((item, duration, start, snr))
    elif "start-times" in opts or "snrs" in opts:
        raise _pipe_error(text, "--start-times / --snrs without --additive-signals")
    return WavEntry(path, opts.get("impulse-response"), noises, True)


def read_wav_scp(wav_scp):
    """(keys, [WavEntry]) of a wav.scp"""
    tab = [l.rstrip().split(None, 1) for l in open(wav_scp) if l.strip()]
    return [k for k, _ in tab], [parse_wav_entry(p) for _, p in tab]


AUX_CACHE_BYTES = 2 << 30       # samples of impulse-response and noise files kept on the host between batches


class WavAugmentation:
    """What an augmented wav.scp adds to the table of its speech files: the parsed entries and ONE table of the distinct
    impulse-response and noise files (each header probed once per run), whose samples are read once and kept on the host (up to
    AUX_CACHE_BYTES).  Every such file must have its speech file's rate."""

    def __init__(self, table, entries):
        from . import ingest
        self.entries = entries
        paths = sorted({p for e in entries for p in self.files(e)})
        self.aux = ingest.WavTable(paths, 0)
        self.index = {p: i for i, p in enumerate(paths)}
        self.cache = collections.OrderedDict()
        self.reads = 0                  # files read so far (a file is read again only after the cache dropped it)
        for i, e in enumerate(entries):
            for p in self.files(e):
                r = int(self.aux.rate[self.index[p]])
                if r != int(table.rate[i]):
                    raise ValueError("%s: sample rate %d differs from the %d Hz of the speech file %s it is applied to"
                                     % (p, r, int(table.rate[i]), table.paths[i]))

    @staticmethod
    def files(e):
        return ([e.rir_path] if e.rir_path else []) + [v[0] for v in e.noises]

    def samples(self, path):
        v = self.cache.get(path)
        if v is None:
            i = self.index[path]
            nmax = int(self.aux.nsamp[i])
            if nmax < 1:
                raise ValueError("%s: no samples" % path)
            buf = torch.empty(1, nmax)
            self.aux.read_padded(np.asarray([i]), nmax, buf, 1)
            v = self.cache[path] = buf.numpy()[0]
            self.reads += 1
            while len(self.cache) > 1 and sum(a.nbytes for a in self.cache.values()) > AUX_CACHE_BYTES:
                self.cache.popitem(last=False)
        return v

    def inputs(self, idx):
        """(rir, noises, names) of the rows idx, as features.augment takes them"""
        rir, noises, names = [], [], []
        for i in idx:
            e = self.entries[i]
            rir.append(self.samples(e.rir_path) if e.rir_path else None)
            noises.append([(self.samples(p), d, st, snr) for p, d, st, snr in e.noises])
            names.append(e.path if not e.augmented else "%s with %s" % (e.path, ", ".join(self.files(e))))
        return rir, noises, names


def augment_inputs(table, idx):
    """(rir, noises, names) for features.augment of the rows idx of the table of an augmented wav.scp
    (wav_scp_batches(..., augment=True): table.augmentation is its WavAugmentation)"""
    return table.augmentation.inputs(idx)


AUX_POOL_BYTES = 2 << 30        # samples of impulse-response and noise files kept on the device by an AugmentPool


class _Arena:
    """a growing float32 device buffer; what is added keeps its offset until reset()"""

    def __init__(self, device):
        self.device, self.buf, self.used = device, None, 0

    def add(self, v):
        need = self.used + v.size
        if self.buf is None or need > self.buf.numel():
            new = torch.empty(max(need, 2 * (self.buf.numel() if self.buf is not None else 1 << 18)), device=self.device)
            if self.used:
                new[:self.used].copy_(self.buf[:self.used])
            self.buf = new
        self.buf[self.used:need].copy_(torch.from_numpy(v), non_blocking=True)
        off, self.used = self.used, need
        return off


class AugmentBatch:
    """the descriptors of one batch for AugmentPool.apply: host arrays in terms of the pool's file numbers (AugmentPool.plan)"""
    __slots__ = ("rows", "rir_file", "desc_ptr", "desc_file", "desc_len", "desc_snr", "files")


class AugmentPool:
    """The device-resident form of WavAugmentation, for a caller that augments batch after batch (training from audio): every
    distinct impulse-response or noise file is read and uploaded once, on first use, into one of two device buffers that are kept
    (up to cap_bytes together; beyond it the pool is emptied and refilled from the batch in hand).  plan(idx) builds the
    descriptors of a batch with numpy array operations over tables made once per wav.scp - on any thread, it touches no device -
    and apply(wave, nsamp, plan) uploads what the pool lacks and runs spk_augment_fwd, the launch of features.augment, on the
    current stream: no host synchronisation, and the counts of clipped samples stay on the device (self.clipped accumulates them
    per call: an int64 scalar tensor, None before the first call).  Everything features.augment refuses is refused here: the values of the entries when the pool
    is made, a file's content when it is first read."""

    def __init__(self, augmentation, device, sample_rate, cap_bytes=AUX_POOL_BYTES):
        self.aug, self.device, self.fs, self.cap = augmentation, torch.device(device), float(sample_rate), int(cap_bytes)
        aux, index, entries = augmentation.aux, augmentation.index, augmentation.entries
        n = len(entries)
        self.ent_rir = np.full(n, -1, dtype=np.int64)
        ptr, dfile, ddur, dstart, dsnr, dent = [0], [], [], [], [], []
        for i, e in enumerate(entries):           # once per wav.scp
            if e.rir_path:
                self.ent_rir[i] = index[e.rir_path]
            for p, d, st, snr in e.noises:
                dfile.append(index[p])
                ddur.append(np.nan if d is None else d)
                dstart.append(st)
                dsnr.append(snr)
                dent.append(i)
            ptr.append(len(dfile))
        self.ent_ptr = np.asarray(ptr, dtype=np.int64)
        self.d_file = np.asarray(dfile, dtype=np.int64)
        dur, start = np.asarray(ddur, dtype=np.float64), np.asarray(dstart, dtype=np.float64)
        self.d_snr = np.asarray(dsnr, dtype=np.float64)
        raw = aux.nsamp[self.d_file] if self.d_file.size else np.zeros(0, dtype=np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            fill = np.where(np.isnan(dur), raw.astype(np.float64), np.where(np.isfinite(dur), np.trunc(self.fs * dur), 0.0))
            bad = ~np.isfinite(self.d_snr) | ~np.isfinite(start) | (start < 0) | ~(fill >= 1) | ~(fill < 2 ** 30) | (start * self.fs >= 2 ** 30)
        if bad.any():
            d = int(np.nonzero(bad)[0][0])
            raise ValueError("augment: a noise of %s (%s) has SNR %r, duration %r s, start %r s: not finite, negative or too long"
                             % (entries[dent[d]].path, aux.paths[self.d_file[d]], self.d_snr[d], ddur[d], dstart[d]))
        self.d_len = np.stack([raw, fill.astype(np.int64), np.trunc(start * self.fs).astype(np.int64)], 1).astype(np.int32) \
            if self.d_file.size else np.zeros((0, 3), dtype=np.int32)
        # per file: the descriptors that add it (for the all-zero check at first read), its place in the pool, the early window
        self._by_file = np.argsort(self.d_file, kind="stable")
        self._file_lo = np.searchsorted(self.d_file[self._by_file], np.arange(len(aux.paths) + 1))
        self.off = np.full(len(aux.paths), -1, dtype=np.int64)
        self.rir_meta = np.zeros((len(aux.paths), 4), dtype=np.int32)
        self.is_rir = np.zeros(len(aux.paths), dtype=bool)
        self.is_rir[self.ent_rir[self.ent_rir >= 0]] = True
        self.is_noise = np.zeros(len(aux.paths), dtype=bool)
        self.is_noise[self.d_file] = True
        self.rirs, self.noises = _Arena(self.device), _Arena(self.device)
        self.noise_off = np.full(len(aux.paths), -1, dtype=np.int64)
        self.clipped = None             # made by the first apply(): nothing is launched here
        lib = hip.lib()
        self.max_rir, self.max_early = lib.spk_augment_max_rir(), lib.spk_augment_max_early()

    @property
    def reads(self):
        """files read so far (a file is read again only after the host cache dropped it and the pool was emptied)"""
        return self.aug.reads

    def plan(self, idx):
        """descriptors of the rows idx of the wav.scp (numpy only): None when no row is augmented"""
        idx = np.asarray(idx, dtype=np.int64)
        rir = self.ent_rir[idx]
        cnt = self.ent_ptr[idx + 1] - self.ent_ptr[idx]
        rows = np.nonzero((rir >= 0) | (cnt > 0))[0]
        if rows.size == 0:
            return None
        p = AugmentBatch()
        p.rows = rows
        p.rir_file = rir[rows]
        cnt = cnt[rows]
        p.desc_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        d = np.repeat(self.ent_ptr[idx[rows]] - p.desc_ptr[:-1], cnt) + np.arange(int(p.desc_ptr[-1]))
        p.desc_file, p.desc_len, p.desc_snr = self.d_file[d], self.d_len[d], self.d_snr[d]
        p.files = np.unique(np.concatenate([p.rir_file[p.rir_file >= 0], p.desc_file]))
        return p

    def _check_file(self, f, v):
        path = self.aug.aux.paths[f]
        if self.is_rir[f]:
            if v.size > self.max_rir:
                raise ValueError("augment: the impulse response %s has %d samples, more than the %d the kernel is built for"
                                 % (path, v.size, self.max_rir))
            s, e0, e1 = early_window(v, self.fs)
            if not 1 <= e1 - e0 <= self.max_early:
                raise ValueError("augment: the early part of the impulse response %s has %d samples at %g Hz, outside [1, %d]"
                                 % (path, e1 - e0, self.fs, self.max_early))
            self.rir_meta[f] = (v.size, s, e0, e1 - e0)
        ds = self._by_file[self._file_lo[f]:self._file_lo[f + 1]]
        for fill in np.unique(np.minimum(self.d_len[ds, 1], v.size)):
            if not np.any(v[:fill]):
                raise ValueError("augment: the noise %s is all zero over the %d samples that are added (its power scales the SNR)"
                                 % (path, int(fill)))

    def _resident(self, files):
        def missing():
            return [int(f) for f in files if (self.is_rir[f] and self.off[f] < 0) or (self.is_noise[f] and self.noise_off[f] < 0)]
        todo = missing()
        if not todo:
            return
        new = 4 * sum(int(self.aug.aux.nsamp[f]) * (int(self.is_rir[f]) + int(self.is_noise[f])) for f in todo)
        if 4 * (self.rirs.used + self.noises.used) + new > self.cap:
            self.off[:] = -1
            self.noise_off[:] = -1
            self.rirs.used = self.noises.used = 0
            todo = missing()
            new = 4 * sum(int(self.aug.aux.nsamp[f]) * (int(self.is_rir[f]) + int(self.is_noise[f])) for f in todo)
            if new > self.cap:
                raise ValueError("augment: one batch needs %d bytes of impulse responses and noises, above the pool's cap of %d"
                                 % (new, self.cap))
        for f in todo:
            v = self.aug.samples(self.aug.aux.paths[f])
            self._check_file(f, v)
            if self.is_rir[f] and self.off[f] < 0:
                self.off[f] = self.rirs.add(v)
            if self.is_noise[f] and self.noise_off[f] < 0:
                self.noise_off[f] = self.noises.add(v)

    def apply(self, wave, nsamp, plan, quantize=True):
        """wave: float32 cuda [B', Nmax], the rows plan.rows of the batch the plan was made for, nsamp: int32 cuda [B'] -> the
        augmented rows [B', Nmax], as features.augment(wave, nsamp, ..., quantize) gives them, bit for bit"""
        B, Nmax = wave.shape
        if B != plan.rows.size:
            raise ValueError("AugmentPool.apply: %d rows for a plan of %d" % (B, plan.rows.size))
        self._resident(plan.files)
        dev = self.device
        has = plan.rir_file >= 0
        rf = np.where(has, plan.rir_file, 0)
        rir_row = np.where(has[:, None], self.rir_meta[rf], 0).astype(np.int32)
        rir_off = np.where(has, self.off[rf], 0).astype(np.int64)
        nd = int(plan.desc_file.size)
        if B + nd > 65535:
            raise ValueError("augment: %d rows with %d noises in one call (at most 65535 together)" % (B, nd))
        Rmax, Emax = int(rir_row[:, 0].max()), int(rir_row[:, 3].max())
        Fmax = int(plan.desc_len[:, 1].max()) if nd else 0
        sizes = (ctypes.c_longlong * 3)()
        hip.call("spk_augment_workspace", B, Nmax, Rmax, Emax, Fmax, nd, sizes)

        def dv(a, dtype):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev, non_blocking=True)
        t_off, t_row, t_ptr = dv(rir_off, np.int64), dv(rir_row, np.int32), dv(plan.desc_ptr, np.int32)
        t_doff = dv(self.noise_off[plan.desc_file], np.int64) if nd else None
        t_dlen = dv(plan.desc_len.reshape(-1), np.int32) if nd else None
        t_dsnr = dv(plan.desc_snr, np.float64) if nd else None
        spectra = torch.empty(2 * sizes[0], device=dev) if sizes[0] else None
        y = torch.empty(max(sizes[1], 1), device=dev)
        work = torch.empty(max(sizes[2], 1), dtype=torch.float64, device=dev)
        out = torch.empty(B, Nmax, device=dev)
        clipped = torch.zeros(B, dtype=torch.int64, device=dev)
        hip.call("spk_augment_fwd", hip.ptr(wave.contiguous()), hip.ptr(nsamp), B, Nmax, hip.ptr(self.rirs.buf) if Rmax else None,
                 self.rirs.used, hip.ptr(t_off), hip.ptr(t_row), Rmax, Emax, hip.ptr(self.noises.buf) if nd else None,
                 self.noises.used, hip.ptr(t_ptr), hip.ptr(t_doff), hip.ptr(t_dlen), hip.ptr(t_dsnr), nd, Fmax,
                 hip.ptr(_aug_twiddle(dev)) if Rmax else None, hip.ptr(spectra), hip.ptr(y), hip.ptr(work), int(bool(quantize)),
                 hip.ptr(out), hip.ptr(clipped), hip.stream())
        self.clipped = clipped.sum() if self.clipped is None else self.clipped + clipped.sum()
        return out


class SpeedBatch:
    """what ChunkFrontend needs for a batch with speed-perturbed rows.  Device tensors made by the caller: ofirst, ototal int64 [B]
    and ocount int32 [B] - row b of the resampled buffer holds samples [ofirst, ofirst + ocount) of the perturbed utterance of
    ototal samples (a plain row: what was read) - and rows int32 [B], the batch's rows grouped by factor.  Host values: groups
    [(fi, fo, lo, hi)]: rows[lo:hi] are resampled from fi to fo Hz; plain (lo, hi): rows[lo:hi] are copied; Nmax_out: the width of
    the resampled buffer (>= every ocount)."""
    __slots__ = ("ofirst", "ototal", "ocount", "rows", "groups", "plain", "Nmax_out")

    def __init__(self, ofirst, ototal, ocount, rows, groups, plain, Nmax_out):
        self.ofirst, self.ototal, self.ocount, self.rows = ofirst, ototal, ocount, rows
        self.groups, self.plain, self.Nmax_out = groups, plain, int(Nmax_out)


class ChunkFrontend:
    """Audio of a batch of training chunks -> the chunks, on the current stream: spk_pcm16_to_f32, the augmentation of the rows
    that have one (AugmentPool), the span fbank / MFCC (fbank_opts: FbankOptions or MfccOptions) and spk_cmn_select with
    span-relative frame indices.  Every argument of a call is a device tensor made by the caller (ingest.WavTrainLoader plans the
    spans on the host and uploads the numbers with the audio): nothing is read back, no .cpu(), no synchronisation.
    ChunkFrontend(fbank_opts, cmn, seed=0, pool=None)(pcm, count, first, total, frame0, nframes, rel, T, utt_ids, plan) -> [B, F, T]
        pcm int16 [B, Nmax]: row b = samples first[b] .. + count[b] of an utterance of total[b] samples (int32 / int64 / int64 [B])
        frame0, nframes int32 [B]: the frames of the utterance that are computed; rel int32 [B, Tcap], Tcap >= max nframes: in its
        first T columns the T selected frames, counted from frame0; plan: AugmentPool.plan of the batch or None
    times: None, or a dict that gets (start, end) event pairs per stage ("convert", "augment", "resample", "frontend", "cmn").
    speed: None, or the SpeedBatch of a batch with speed-perturbed rows (`sox ... speed F` entries).  pcm, count, first and total
    then describe what was read from the FILE, and frame0 / nframes / rel count frames of the PERTURBED utterance: after the
    conversion (and the augmentation of the plain rows that have one) every group of rows of one factor goes through one
    spkw_resample_span_fwd launch and the plain rows through spkw_copy_rows_fwd, all into one [B, Nmax_out] buffer, which the
    span front end reads with first = speed.ofirst, total = speed.ototal and count = speed.ocount."""

    def __init__(self, fbank_opts, cmn=None, seed=0, pool=None):
        self.opts, self.cmn, self.seed, self.pool = fbank_opts, cmn, seed, pool
        self.mfcc = isinstance(fbank_opts, MfccOptions)
        self.dim = fbank_opts.num_ceps if self.mfcc else fbank_opts.num_mel_bins

    def __call__(self, pcm, count, first, total, frame0, nframes, rel, T, utt_ids=None, plan=None, times=None, speed=None):
        B, Nmax = pcm.shape
        Tcap = rel.shape[1]
        dev = pcm.device
        if self.opts.dither != 0 and utt_ids is None:
            raise ValueError("ChunkFrontend: dither != 0 needs utt_ids")
        if plan is not None and self.pool is None:
            raise ValueError("ChunkFrontend: augmented rows need an AugmentPool")

        def stage(name, fn):
            if times is None:
                return fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            times[name] = (e0, e1)
            return r
        wave = stage("convert", lambda: pcm16_to_f32(pcm, count))
        if plan is not None:
            def aug():
                if plan.rows.size == B:
                    return self.pool.apply(wave, count, plan)
                rows = torch.from_numpy(plan.rows).to(dev, non_blocking=True)
                wave.index_copy_(0, rows, self.pool.apply(wave.index_select(0, rows), count.index_select(0, rows), plan))
                return wave
            wave = stage("augment", aug)
        if speed is not None:
            def resample_rows():
                out = torch.empty(B, speed.Nmax_out, device=dev)
                for fi, fo, lo, hi in speed.groups:
                    _resample_span_launch(wave, first, count, total, speed.ofirst, speed.ocount, speed.rows[lo:hi], fi, fo, out)
                if speed.plain[1] > speed.plain[0]:
                    _copy_rows_launch(wave, count, speed.rows[speed.plain[0]:speed.plain[1]], out)
                return out
            wave = stage("resample", resample_rows)
            count, first, total = speed.ocount, speed.ofirst, speed.ototal
        feats, _ = stage("frontend", lambda: _launch(self.mfcc, self.opts, wave, count, utt_ids, self.seed, Tcap,
                                                     span=(first, total, frame0, nframes)))
        W = int(self.cmn.cmn_window) if self.cmn is not None else 0
        F = feats.shape[1]

        def cmn():
            pre = torch.empty(B * F * (Tcap + 1), dtype=torch.float64, device=dev) if W > 0 else None
            out = torch.empty(B, F, T, device=dev)
            cnt = torch.full((B,), T, dtype=torch.int32, device=dev)
            hip.call("spk_cmn_select", hip.ptr(feats), hip.ptr(nframes), hip.ptr(rel), hip.ptr(cnt), hip.ptr(pre), hip.ptr(out), B, F,
                     Tcap, T, W, hip.stream())
            return out
        return stage("cmn", cmn)


# ---- functional API ----
def _launch(mfcc, opts, wave, ns, ids, seed, Tcap, out=None, span=None):
    """the one front-end launch, on device arguments alone (no check of their values, nothing read back).  mfcc: spk_mfcc_* with
    the cepstral options of an MfccOptions, else spk_fbank_*; span: None for the whole-utterance kernels, or the device tensors
    (first, total, frame0, nframes) of the span kernels.  Returns (feats [B, R, Tcap] - `out` when given -, log_energy [B, Tcap])"""
    B, Nmax = wave.shape
    dev = wave.device
    tab = _tables(opts, dev)
    feats = torch.empty(B, opts.num_ceps if mfcc else opts.num_mel_bins, Tcap, device=dev) if out is None else out
    loge = torch.empty(B, Tcap, device=dev)
    tdev = torch.empty(B, dtype=torch.int32, device=dev)
    name = (("spk_fbank_fwd", "spk_fbank_span_fwd"), ("spk_mfcc_fwd", "spk_mfcc_span_fwd"))[bool(mfcc)][span is not None]
    p = hip.ptr
    # the arguments that only the MFCC exports take, in their three places of the parameter list
    tables, ceps, order = ((), (), ()) if not mfcc else ((p(tab.dct), p(tab.lifter)), (opts.num_ceps,),
                                                         (int(opts.use_energy), int(opts.htk_compat)))
    hip.call(name, p(wave), p(ns), *(p(t) for t in span or ()), p(ids), B, Nmax, p(tab.window), p(tab.twiddle), p(tab.mel_w),
             p(tab.mel_lo), p(tab.mel_off), *tables, opts.frame_len, opts.frame_sh, opts.padded_len, opts.num_mel_bins, *ceps,
             int(opts.snip_edges), float(opts.dither), float(opts.preemphasis_coefficient), int(opts.remove_dc_offset),
             float(opts.energy_floor), *order, int(seed) & (2 ** 64 - 1), p(feats), p(loge), p(tdev), Tcap, hip.stream())
    return feats, loge


def _checked(what, mfcc, wave, opts, utt_ids, Tcap, out, rows, min_cap):
    """the argument checks that the whole-utterance and the span forms share, in front of any device work (`what` names the
    caller in the messages).  rows(B, Nmax): the form's own checks of its per-row host integers -> (frames per row, [(array,
    dtype), ..] the integer arguments of the launch); min_cap: the least Tcap the form picks by itself.
    Returns (wave contiguous, frames per row, Tcap, the integer arguments on the device, utt_ids on the device or None)"""
    if not getattr(wave, "is_cuda", False) or wave.dim() != 2 or wave.dtype != torch.float32:
        raise ValueError("%s: wave must be a float32 cuda tensor [B, Nmax]" % what)
    wave = wave.contiguous()
    B, Nmax = wave.shape
    T, ints = rows(B, Nmax)
    longest = max(int(T.max()), min_cap)
    Tcap = longest if Tcap is None else int(Tcap)
    if Tcap < longest:
        raise ValueError("%s: Tcap %d < longest row, %d frames" % (what, Tcap, longest))
    if opts.dither != 0 and utt_ids is None:
        raise ValueError("%s: dither != 0 needs utt_ids (the key of each row's noise)" % what)
    R = opts.num_ceps if mfcc else opts.num_mel_bins
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (B, R, Tcap)
                            or not out.is_cuda or not out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous float32 cuda tensor [%d, %d, %d]" % (what, B, R, Tcap))
    dev = wave.device

    def dv(a, dtype):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)
    return wave, T, Tcap, [dv(a, dtype) for a, dtype in ints], dv(_host_ints(utt_ids), np.int64) if utt_ids is not None else None


def _whole(what, mfcc, wave, nsamp, opts, utt_ids, seed, Tcap, out=None):
    """fbank and mfcc: every row is a whole utterance of at least one frame"""
    def rows(B, Nmax):
        n = _host_ints(nsamp)
        if n.size != B:
            raise ValueError("%s: %d sample counts for %d rows" % (what, n.size, B))
        L = opts.frame_len
        if (n < L).any() or (n > Nmax).any():
            bad = int(np.nonzero((n < L) | (n > Nmax))[0][0])
            raise ValueError("%s: row %d has %d samples, outside [frame length %d, Nmax %d]" % (what, bad, int(n[bad]), L, Nmax))
        return np.asarray([opts.num_frames(int(v)) for v in n], dtype=np.int64), [(n, np.int32)]
    wave, T, Tcap, (ns,), ids = _checked(what, mfcc, wave, opts, utt_ids, Tcap, out, rows, 0)
    feats, loge = _launch(mfcc, opts, wave, ns, ids, seed, Tcap, out)
    return feats, T, loge


def fbank(wave, nsamp, opts, utt_ids=None, seed=0, Tcap=None):
    """wave: float32 cuda [B, Nmax] at int16 scale, nsamp: per-row sample counts (host or device ints, each >= frame length).
    Returns (feats [B, F, Tcap] cuda (zeros past T[b]), T int64 host array, log_energy [B, Tcap] cuda (raw log energy))."""
    return _whole("fbank", False, wave, nsamp, opts, utt_ids, seed, Tcap)


def mfcc(wave, nsamp, opts, utt_ids=None, seed=0, Tcap=None, out=None):
    """compute-mfcc-feats (opts: MfccOptions).  wave, nsamp, utt_ids, seed, Tcap as for fbank; the frames, the dither draws and the
    raw log energy are the fbank's for the same framing options.  Returns (feats [B, C, Tcap] cuda, C = num_ceps (zeros past T[b]),
    T int64 host array, log_energy [B, Tcap] cuda - the raw log energy, floored by log(energy_floor), whatever use_energy says:
    the VAD's input).  out: a preallocated contiguous float32 cuda tensor [B, C, Tcap] to write the features into."""
    if not isinstance(opts, MfccOptions):
        raise ValueError("mfcc: opts must be an MfccOptions")
    return _whole("mfcc", True, wave, nsamp, opts, utt_ids, seed, Tcap, out)


# ---- the span form: frames of a part of an utterance, equal to the frames of the whole ----
def span_samples(opts, frame_lo, frame_hi, total):
    """(first, last): the samples [first, last) of utterances of `total` samples that their frames [frame_lo, frame_hi) read, the
    snip_edges=false reflection about 0 and `total` included (integer arrays, numpy only; frame_hi > frame_lo)"""
    L, S = opts.frame_len, opts.frame_sh
    lo, hi, N = (np.asarray(v, dtype=np.int64) for v in (frame_lo, frame_hi, total))
    off = 0 if opts.snip_edges else L // 2 - S // 2
    a, b = lo * S - off, (hi - 1) * S - off + L
    first, last = np.maximum(a, 0), np.minimum(b, N)
    last = np.where(a < 0, np.maximum(last, np.minimum(-a, N)), last)          # s < 0 reads -s - 1
    first = np.where(b > N, np.minimum(first, np.maximum(2 * N - b, 0)), first)  # s >= N reads 2N - 1 - s
    return first, last


def pcm16_to_f32(pcm, count, out=None):
    """16-bit samples as they lie in a WAV file -> float32 at int16 scale on the GPU.  pcm: int16 cuda [B, Nmax], count: int32 cuda
    [B] (samples per row); zeros past the count.  Nothing is read back."""
    if not isinstance(pcm, torch.Tensor) or pcm.dim() != 2 or pcm.dtype != torch.int16 or not pcm.is_cuda:
        raise ValueError("pcm16_to_f32: pcm must be an int16 cuda tensor [B, Nmax]")
    B, Nmax = pcm.shape
    if B == 0 or Nmax == 0:
        raise ValueError("pcm16_to_f32: empty batch [%d, %d]" % (B, Nmax))
    if not (isinstance(count, torch.Tensor) and count.is_cuda and count.dtype == torch.int32 and count.numel() == B):
        raise ValueError("pcm16_to_f32: count must be an int32 cuda tensor of %d rows" % B)
    if out is None:
        out = torch.empty(B, Nmax, device=pcm.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, Nmax) or not out.is_cuda or not out.is_contiguous():
        raise ValueError("pcm16_to_f32: out must be a contiguous float32 cuda tensor [%d, %d]" % (B, Nmax))
    hip.call("spk_pcm16_to_f32", hip.ptr(pcm.contiguous()), hip.ptr(count), B, Nmax, hip.ptr(out), hip.stream())
    return out


def check_spans(what, opts, nsamp, first, total, frame0, nframes, Nmax):
    """the refusals of the span form, on host arrays, before any launch: every computed frame exists in the utterance and, after
    reflection, touches only samples that the row holds.  Returns the arrays as int64."""
    n, f, N, f0, nf = (_host_ints(v) for v in (nsamp, first, total, frame0, nframes))
    B = n.size
    if not (f.size == N.size == f0.size == nf.size == B):
        raise ValueError("%s: nsamp, first, total, frame0 and nframes must have one entry per row (%d rows)" % (what, B))
    L = opts.frame_len

    def bad(mask, msg):
        if mask.any():
            b = int(np.nonzero(mask)[0][0])
            raise ValueError("%s: row %d (first %d, %d samples, utterance of %d samples, frames %d .. +%d): %s"
                             % (what, b, int(f[b]), int(n[b]), int(N[b]), int(f0[b]), int(nf[b]), msg))
    bad((n < 1) | (n > Nmax), "sample count outside [1, Nmax %d]" % Nmax)
    bad(N < L, "the utterance is shorter than one frame (%d samples)" % L)
    bad((f < 0) | (f + n > N), "the row is not a part of the utterance")
    Tu = np.asarray([opts.num_frames(int(v)) for v in N], dtype=np.int64)
    bad((f0 < 0) | (nf < 0) | (f0 + nf > Tu), "frames outside the utterance's")
    need_first, need_last = span_samples(opts, f0, np.maximum(f0 + nf, f0 + 1), N)
    bad((nf > 0) & ((need_first < f) | (need_last > f + n)), "a frame touches a sample outside the row")
    return n, f, N, f0, nf


def _span(what, mfcc, wave, nsamp, first, total, frame0, nframes, opts, utt_ids, seed, Tcap, out=None):
    """fbank_span and mfcc_span: check_spans on the rows; a row may have no frame, Tcap is at least 1"""
    def rows(B, Nmax):
        n, f, N, f0, nf = check_spans(what, opts, nsamp, first, total, frame0, nframes, Nmax)
        if n.size != B:
            raise ValueError("%s: %d sample counts for %d rows" % (what, n.size, B))
        return nf, [(n, np.int32), (f, np.int64), (N, np.int64), (f0, np.int32), (nf, np.int32)]
    wave, nf, Tcap, (ns, *span), ids = _checked(what, mfcc, wave, opts, utt_ids, Tcap, out, rows, 1)
    feats, loge = _launch(mfcc, opts, wave, ns, ids, seed, Tcap, out, span)
    return feats, nf, loge


def fbank_span(wave, nsamp, first, total, frame0, nframes, opts, utt_ids=None, seed=0, Tcap=None):
    """The frames of a span of each utterance, equal bit for bit to the same frames of fbank() on the whole utterance.  Row b of
    wave (float32 cuda [B, Nmax], int16 scale) holds samples first[b] .. first[b] + nsamp[b] - 1 of an utterance of total[b]
    samples; computed are frames frame0[b] .. frame0[b] + nframes[b] - 1 of that utterance: the reflection of snip_edges=false is
    about 0 and total[b], the dither draw is keyed by the frame's index in the utterance.  All five are host integers per row.
    Returns (feats [B, F, Tcap] cuda, column j = frame frame0[b] + j, zeros from nframes[b]; nframes int64 host array; log_energy
    [B, Tcap]).  Refused before any launch: a frame outside the utterance, a frame that after reflection touches a sample outside
    its row (span_samples gives the samples a frame range needs)."""
    if isinstance(opts, MfccOptions):
        raise ValueError("fbank_span: opts must be a FbankOptions (mfcc_span takes MfccOptions)")
    return _span("fbank_span", False, wave, nsamp, first, total, frame0, nframes, opts, utt_ids, seed, Tcap)


def mfcc_span(wave, nsamp, first, total, frame0, nframes, opts, utt_ids=None, seed=0, Tcap=None, out=None):
    """fbank_span for compute-mfcc-feats (opts: MfccOptions): feats [B, num_ceps, Tcap], equal bit for bit to mfcc() on the whole
    utterance.  out: as for mfcc, [B, num_ceps, Tcap]"""
    if not isinstance(opts, MfccOptions):
        raise ValueError("mfcc_span: opts must be an MfccOptions")
    return _span("mfcc_span", True, wave, nsamp, first, total, frame0, nframes, opts, utt_ids, seed, Tcap, out)


def dither_noise(utt, seed, frame0, nframes, L, device="cuda"):
    """[nframes, L] the N(0,1) noise spk_fbank_fwd / spk_mfcc_fwd adds (times dither) to frames frame0 .. of the utterance with id `utt`"""
    out = torch.empty(nframes, L, device=device)
    hip.call("spk_fbank_dither_noise", hip.ptr(out), int(utt), int(seed) & (2 ** 64 - 1), int(frame0), int(nframes), int(L),
             hip.stream())
    return out


def vad(log_energy, T, opts):
    """compute-vad on raw log energies [B, Tcap] (cuda) of T[b] frames -> (vad [B, Tcap] int32 cuda, idx [B, Tcap] int32 cuda: the
    voiced frames of row b in idx[b, :count[b]], count int64 host array)"""
    B, Tcap = log_energy.shape
    dev = log_energy.device
    tdev = torch.as_tensor(_host_ints(T, np.int32)).to(dev)
    v = torch.empty(B, Tcap, dtype=torch.int32, device=dev)
    idx = torch.empty(B, Tcap, dtype=torch.int32, device=dev)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    hip.call("spk_vad_count", hip.ptr(log_energy.contiguous()), hip.ptr(tdev), B, Tcap, float(opts.vad_energy_threshold),
             float(opts.vad_energy_mean_scale), int(opts.vad_frames_context), float(opts.vad_proportion_threshold), hip.ptr(v),
             hip.ptr(idx), hip.ptr(cnt), hip.stream())
    return v, idx, cnt.cpu().numpy().astype(np.int64)


SEGMENT_CAP = 1024      # segments per row the first launch of vad_segments has room for


def vad_segments(vad, T, opts):
    """spk_vad_segments: the VAD decisions vad [B, Tcap] (int32 cuda; voiced iff != 0) of T[b] frames -> the speech segments under
    SegmentOptions `opts`, as (row, start, end): flat int64 host arrays in row and then time order - what ingest.segments_from_vad
    gives for the same input.  One launch with room for SEGMENT_CAP segments per row, one more with room for the largest count
    when a row has more; only the counts and the written pairs are downloaded, never the VAD tensor."""
    if vad.dim() != 2 or vad.dtype != torch.int32 or not vad.is_cuda:
        raise ValueError("vad_segments: vad must be a [B, Tcap] int32 cuda tensor")
    B, Tcap = vad.shape
    dev = vad.device
    vad = vad.contiguous()
    tdev = torch.as_tensor(_host_ints(T, np.int32)).to(dev)
    if tdev.numel() != B:
        raise ValueError("vad_segments: T has %d entries for %d rows" % (tdev.numel(), B))
    nseg = torch.empty(B, dtype=torch.int32, device=dev)
    cap = SEGMENT_CAP
    while True:
        seg = torch.empty(B, cap, 2, dtype=torch.int32, device=dev)
        hip.call("spk_vad_segments", hip.ptr(vad), hip.ptr(tdev), B, Tcap, int(opts.padding), int(opts.max_gap), int(opts.min_length),
                 hip.ptr(seg), cap, hip.ptr(nseg), hip.stream())
        n = nseg.cpu().numpy().astype(np.int64)
        if n.size == 0 or int(n.max()) <= cap:
            break
        cap = int(n.max())
    written = torch.arange(cap, device=dev)[None, :] < nseg[:, None]
    pairs = seg[written].cpu().numpy().astype(np.int64)        # [sum n, 2], row-major: by row, then in order
    return np.repeat(np.arange(B, dtype=np.int64), n), np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def _cmn_select(x, T, idx, count, cmn, Tout):
    B, F, Tcap = x.shape
    dev = x.device
    x = x.contiguous()
    tdev = torch.as_tensor(_host_ints(T, np.int32)).to(dev)
    W = int(cmn.cmn_window) if cmn is not None else 0
    pre = torch.empty(B * F * (Tcap + 1), dtype=torch.float64, device=dev) if W > 0 else None
    cdev = torch.as_tensor(_host_ints(count, np.int32)).to(dev) if count is not None else None
    out = torch.empty(B, F, max(Tout, 1), device=dev)
    hip.call("spk_cmn_select", hip.ptr(x), hip.ptr(tdev), hip.ptr(idx), hip.ptr(cdev), hip.ptr(pre), hip.ptr(out), B, F, Tcap,
             max(Tout, 1), W, hip.stream())
    return out[:, :, :Tout]


def sliding_cmn(x, T, opts):
    """apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=W over every frame of x [B, F, Tcap] (cuda, T[b] frames):
    [B, F, Tcap], zeros past T[b]"""
    return _cmn_select(x, T, None, None, opts, x.shape[2])


def select_voiced(x, T, idx, count, cmn=None):
    """select-voiced-frames (after the optional sliding CMN over all frames): the frames idx[b, :count[b]] of x [B, F, Tcap]
    compacted into [B, F, max(count)] with zero tails; returns (feats, lengths = count)"""
    count = _host_ints(count)
    return _cmn_select(x, T, idx, count, cmn, int(count.max()) if count.size else 0), count


class Frontend:
    """wav -> model input: (optional) resampling, fbank (MFCC when fbank_opts is an MfccOptions), then (optional) sliding CMN over all frames and voiced-frame selection, as the
    recipe's prepare_feats_for_egs.sh.  Frontend(fbank_opts, vad=None, cmn=None, input_rate=None, speed=None)(wave [B, Nmax] cuda,
    nsamp, utt_ids, seed, input_rate=None) -> (feats [B, F, T] cuda, lengths int64 host array): the input predict(x, lengths=...)
    takes.  A row without voiced frames has length 0 (its column block is all zero): the caller reports and skips it.

    input_rate: the rate of the samples handed in (one rate per batch; the call's input_rate overrides the constructor's), resampled
    to fbank_opts.sample_frequency first.  speed: a decimal string or Fraction ("0.9"): the audio is played `speed` times as fast,
    i.e. resampled from input_rate * speed to sample_frequency - one resampling for both.  Every row must still hold a frame after it.

    segments: a SegmentOptions (needs `vad`).  The call then returns (feats, T, (row, start, end)): the
    features of ALL frames - the sliding CMN over all frames, no voiced-frame selection, lengths = the frame counts T - and the
    speech segments that vad_segments makes of the VAD decisions, in frames of the recording."""

    def __init__(self, fbank_opts, vad=None, cmn=None, input_rate=None, speed=None, segments=None):
        if segments is not None and vad is None:
            raise ValueError("Frontend: segments needs vad (the segments are made of the VAD decisions)")
        self.fbank_opts, self.vad_opts, self.cmn_opts, self.segment_opts = fbank_opts, vad, cmn, segments
        self.input_rate = None if input_rate is None else _int_rate(input_rate, "Frontend")
        self.speed = speed
        self.rates(self.input_rate)     # refuse a bad speed / rate pair here, not at the first batch

    def rates(self, input_rate=None):
        """(fi, fo) of the resampling in front of the fbank for samples at input_rate (None: the constructor's, else the fbank's)"""
        fo = _int_rate(self.fbank_opts.sample_frequency, "Frontend") if (input_rate or self.input_rate or self.speed) else None
        fi = input_rate or self.input_rate or fo
        if self.speed is not None:
            return speed_rates(self.speed, fo, fi)
        return (None, None) if fo is None else (_int_rate(fi, "Frontend"), fo)

    def __call__(self, wave, nsamp, utt_ids=None, seed=0, input_rate=None):
        fi, fo = self.rates(input_rate)
        if fi != fo:
            wave, nsamp = resample(wave, nsamp, fi, fo)
        feats, T, loge = (mfcc if isinstance(self.fbank_opts, MfccOptions) else fbank)(wave, nsamp, self.fbank_opts, utt_ids, seed)
        if self.vad_opts is None:
            if self.cmn_opts is not None:
                feats = sliding_cmn(feats, T, self.cmn_opts)
            return feats, T
        v, idx, cnt = vad(loge, T, self.vad_opts)
        if self.segment_opts is not None:
            if self.cmn_opts is not None:
                feats = sliding_cmn(feats, T, self.cmn_opts)
            return feats, T, vad_segments(v, T, self.segment_opts)
        return select_voiced(feats, T, idx, cnt, self.cmn_opts)


# ---- wav.scp helpers of scripts/compute_fbank.py, scripts/compute_mfcc.py and scripts/decode.py --wav-scp ----
def options_from_configs(fbank_config=None, vad_config=None, cmn_window=0, mfcc_config=None):
    """(FbankOptions, VadOptions or None, CmnOptions or None) from Kaldi config files and an apply-cmvn-sliding window (0: no CMN);
    mfcc_config (instead of fbank_config; "" for compute-mfcc-feats' defaults): MfccOptions in place of the FbankOptions"""
    if mfcc_config is not None and fbank_config:
        raise ValueError("options_from_configs: fbank_config and mfcc_config are mutually exclusive")
    if mfcc_config is not None:
        fb = MfccOptions.from_kaldi_config(mfcc_config) if mfcc_config else MfccOptions()
    else:
        fb = FbankOptions.from_kaldi_config(fbank_config) if fbank_config else FbankOptions()
    vad_opts = VadOptions.from_kaldi_config(vad_config) if vad_config else None
    cmn = CmnOptions(cmn_window=cmn_window) if cmn_window and cmn_window > 0 else None
    return fb, vad_opts, cmn


def wav_scp_batches(wav_scp, fb, batch_size, allow_downsample=False, allow_upsample=False, speed=None, augment=False,
                    speed_entries=False):
    """(keys, ingest.WavTable, batches [(indices, Nmax)], indices shorter than one frame) of a wav.scp ('key path' lines; pipe
    entries are refused, except - with augment=True, for a caller that applies them - the wav-reverberate entries that
    parse_wav_entry accepts): length-sorted by the speech file's sample count, at most 10 % padded samples per batch.  With such
    entries the table is the speech files' and table.augmentation a WavAugmentation (augment_inputs(table, idx) gives what
    features.augment takes); wav_scp may also be what read_wav_scp returned, (keys, entries), so that a caller parses the file once;
    without any, nothing differs from a call without `augment`.

    A file whose header rate is above / below fb.sample_frequency is refused, naming it, unless allow_downsample / allow_upsample
    is set (compute-fbank-feats' flags).  With them every batch holds files of ONE rate, table.rate[indices[0]]: files are grouped
    by rate, then sorted and padded within a rate.  `short` is judged on the length after resampling (and after `speed`).

    speed_entries=True, for a caller that applies them: the `sox ... speed F` entries of a speed-perturbed data directory are
    taken (without it they are refused like any other pipe).  table.speed[i] is then entry i's factor (the decimal string, or None)
    and no batch mixes (file rate, factor): batch b is resampled from speed_rates(table.speed[i], fo, table.rate[i])[0] to fo
    for i = indices[0].  Such entries do not combine with the `speed` argument, and a factor whose filter table exceeds the LDS
    budget of the resampler is refused here, naming the key."""
    from . import ingest
    keys, entries = read_wav_scp(wav_scp) if isinstance(wav_scp, str) else wav_scp
    augmented = any(e.augmented for e in entries)
    if augmented and not augment:
        raise ValueError("wav.scp pipe entries are not applied here: %r" % [e for e in entries if e.augmented][0].path)
    perturbed = [i for i, e in enumerate(entries) if e.speed is not None]
    if perturbed and not speed_entries:
        raise ValueError("wav.scp pipe entries are not applied here: %r (a `sox ... speed` entry)" % entries[perturbed[0]].path)
    if perturbed and speed is not None:
        raise ValueError("speed %s does not combine with the `sox ... speed` entries of the wav.scp (%s)" % (speed, keys[perturbed[0]]))
    table = ingest.WavTable([e.path for e in entries], 0)
    if augmented:
        table.augmentation = WavAugmentation(table, entries)
    table.speed = [e.speed for e in entries]
    fo = _int_rate(fb.sample_frequency, "wav_scp_batches")
    for i in np.nonzero(table.rate != fo)[0]:
        r = int(table.rate[i])
        if r > fo and not allow_downsample:
            raise ValueError("%s: sample rate %d is above sample_frequency %d (--allow-downsample resamples it)" % (table.paths[i], r, fo))
        if r < fo and not allow_upsample:
            raise ValueError("%s: sample rate %d is below sample_frequency %d (--allow-upsample resamples it)" % (table.paths[i], r, fo))
    n_eff = np.zeros(len(keys), dtype=np.int64)
    # the factor of every entry as a group number: 0 = none, then the distinct factors in order of their value
    factors = sorted({e.speed for e in entries if e.speed is not None}, key=fractions.Fraction)
    group = np.asarray([0 if e.speed is None else 1 + factors.index(e.speed) for e in entries], dtype=np.int64)
    for r in np.unique(table.rate):
        for g in np.unique(group[table.rate == r]):
            sel = (table.rate == r) & (group == g)
            f = speed if g == 0 else factors[g - 1]
            fi = speed_rates(f, fo, int(r))[0] if f is not None else int(r)
            if g:
                check_speed_table("%s (speed %s)" % (keys[int(np.nonzero(sel)[0][0])], f), fi, fo)
            n_eff[sel] = num_resampled(table.nsamp[sel], fi, fo)
    good = n_eff >= fb.frame_len
    short = np.nonzero(~good)[0]
    batches = []
    for r in np.unique(table.rate[good]):
        for g in np.unique(group[good & (table.rate == r)]):
            ok = np.nonzero(good & (table.rate == r) & (group == g))[0]
            batches += [(ok[b], int(n)) for b, n in ingest.pad_batches(table.nsamp[ok], batch_size, quantum=1)]
    return keys, table, batches, short


def speed_key(speed, name):
    """sp<F>-<name>: the key / speaker prefix of local/perturb_data_dir_speed.sh"""
    return "sp%s-%s" % (speed, name)


def speed_side_files(speed, keys, utt2spk=None):
    """the text of the utt2spk and utt2uniq files perturb_data_dir_speed.sh makes for the copies sp<F>-<utt> of `keys` (original
    keys, in order): (utt2spk text or None without a speaker map, utt2uniq text).  utt2spk: {utt: spk}; a key without a speaker
    is an error."""
    u2s = None
    if utt2spk is not None:
        missing = [k for k in keys if k not in utt2spk]
        if missing:
            raise ValueError("utt2spk has no speaker for %s" % missing[0])
        u2s = "".join("%s %s\n" % (speed_key(speed, k), speed_key(speed, utt2spk[k])) for k in keys)
    return u2s, "".join("%s %s\n" % (speed_key(speed, k), k) for k in keys)
