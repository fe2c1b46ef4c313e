"""Kaldi-compatible feature front end on the GPU: fbank (compute-fbank-feats), energy VAD (compute-vad), centred sliding CMN
(apply-cmvn-sliding --norm-vars=false --center=true) and voiced-frame selection (select-voiced-frames) - the Kaldi binaries of
stage 1 of the reference's feature_pre.sh:77-104 and of local/nnet3/xvector/prepare_feats_for_egs.sh:68-70.

The kernels are csrc/frontend.hip (include/spkhip.h: spk_fbank_fwd, spk_vad_count, spk_cmn_select); this module parses Kaldi config
files, builds the window / twiddle / mel tables in fp64 and runs the launches.  Semantics and numerics: DESIGN.md "Feature front end".
The one deliberate difference from Kaldi: dither is a counter-based N(0,1) draw keyed by (seed, utt_id, frame, position), and the VAD
sees the same dithered frames as the fbank (Kaldi draws a second dither for its MFCC pass).
"""
import dataclasses
import hashlib
import math

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
        if self.window_type not in WINDOWS:
            raise ValueError("FbankOptions: window_type %r (one of %s)" % (self.window_type, ", ".join(WINDOWS)))
        if self.num_mel_bins <= 3:
            raise ValueError("FbankOptions: num_mel_bins must be > 3")
        if self.frame_len < 2 or self.frame_sh < 1:
            raise ValueError("FbankOptions: frame length %d / shift %d samples" % (self.frame_len, self.frame_sh))
        if self.padded_len > 1024:
            raise ValueError("FbankOptions: padded window of %d samples > 1024 is not supported" % self.padded_len)
        if not 0.0 <= self.preemphasis_coefficient <= 1.0 or self.dither < 0 or self.energy_floor < 0:
            raise ValueError("FbankOptions: preemphasis_coefficient in [0, 1], dither >= 0, energy_floor >= 0")
        nyq = 0.5 * self.sample_frequency
        hf = self.high_freq + nyq if self.high_freq <= 0 else self.high_freq
        if not (0.0 <= self.low_freq < nyq and 0.0 < hf <= nyq and self.low_freq < hf):
            raise ValueError("FbankOptions: low_freq %g / high_freq %g vs. Nyquist %g" % (self.low_freq, self.high_freq, nyq))

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


_TABLES = {}


def _tables(opts, device):
    key = (dataclasses.astuple(opts), str(device))
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


# ---- functional API ----
def fbank(wave, nsamp, opts, utt_ids=None, seed=0, Tcap=None):
    """wave: float32 cuda [B, Nmax] at int16 scale, nsamp: per-row sample counts (host or device ints, each >= frame length).
    Returns (feats [B, F, Tcap] cuda (zeros past T[b]), T int64 host array, log_energy [B, Tcap] cuda (raw log energy))."""
    if wave.dim() != 2 or wave.dtype != torch.float32 or not wave.is_cuda:
        raise ValueError("fbank: wave must be a float32 cuda tensor [B, Nmax]")
    wave = wave.contiguous()
    B, Nmax = wave.shape
    n = _host_ints(nsamp)
    if n.size != B:
        raise ValueError("fbank: %d sample counts for %d rows" % (n.size, B))
    L = opts.frame_len
    if (n < L).any() or (n > Nmax).any():
        bad = int(np.nonzero((n < L) | (n > Nmax))[0][0])
        raise ValueError("fbank: row %d has %d samples, outside [frame length %d, Nmax %d]" % (bad, int(n[bad]), L, Nmax))
    T = np.asarray([opts.num_frames(int(v)) for v in n], dtype=np.int64)
    Tcap = int(T.max()) if Tcap is None else int(Tcap)
    if Tcap < T.max():
        raise ValueError("fbank: Tcap %d < longest utterance %d frames" % (Tcap, int(T.max())))
    if opts.dither != 0 and utt_ids is None:
        raise ValueError("fbank: dither != 0 needs utt_ids (the key of each row's noise)")
    dev = wave.device
    tab = _tables(opts, dev)
    ns = torch.from_numpy(n.astype(np.int32)).to(dev)
    ids = torch.as_tensor(_host_ints(utt_ids), dtype=torch.int64).to(dev) if utt_ids is not None else None
    feats = torch.empty(B, opts.num_mel_bins, Tcap, device=dev)
    loge = torch.empty(B, Tcap, device=dev)
    tdev = torch.empty(B, dtype=torch.int32, device=dev)
    hip.call("spk_fbank_fwd", hip.ptr(wave), hip.ptr(ns), hip.ptr(ids), B, Nmax, hip.ptr(tab.window), hip.ptr(tab.twiddle),
             hip.ptr(tab.mel_w), hip.ptr(tab.mel_lo), hip.ptr(tab.mel_off), L, opts.frame_sh, opts.padded_len, opts.num_mel_bins,
             int(opts.snip_edges), float(opts.dither), float(opts.preemphasis_coefficient), int(opts.remove_dc_offset),
             float(opts.energy_floor), int(seed) & (2 ** 64 - 1), hip.ptr(feats), hip.ptr(loge), hip.ptr(tdev), Tcap, hip.stream())
    return feats, T, loge


def dither_noise(utt, seed, frame0, nframes, L, device="cuda"):
    """[nframes, L] the N(0,1) noise spk_fbank_fwd adds (times dither) to frames frame0 .. of the utterance with id `utt`"""
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
    """wav -> model input: fbank, then (optional) sliding CMN over all frames and voiced-frame selection, as the recipe's
    prepare_feats_for_egs.sh.  Frontend(fbank_opts, vad=None, cmn=None)(wave [B, Nmax] cuda, nsamp, utt_ids, seed) ->
    (feats [B, F, T] cuda, lengths int64 host array): the input predict(x, lengths=...) takes.  A row without voiced frames has
    length 0 (its column block is all zero): the caller reports and skips it."""

    def __init__(self, fbank_opts, vad=None, cmn=None):
        self.fbank_opts, self.vad_opts, self.cmn_opts = fbank_opts, vad, cmn

    def __call__(self, wave, nsamp, utt_ids=None, seed=0):
        feats, T, loge = fbank(wave, nsamp, self.fbank_opts, utt_ids, seed)
        if self.vad_opts is None:
            if self.cmn_opts is not None:
                feats = sliding_cmn(feats, T, self.cmn_opts)
            return feats, T
        _, idx, cnt = vad(loge, T, self.vad_opts)
        return select_voiced(feats, T, idx, cnt, self.cmn_opts)


# ---- wav.scp helpers of scripts/compute_fbank.py and scripts/decode.py --wav-scp ----
def options_from_configs(fbank_config=None, vad_config=None, cmn_window=0):
    """(FbankOptions, VadOptions or None, CmnOptions or None) from Kaldi config files and an apply-cmvn-sliding window (0: no CMN)"""
    fb = FbankOptions.from_kaldi_config(fbank_config) if fbank_config else FbankOptions()
    vad_opts = VadOptions.from_kaldi_config(vad_config) if vad_config else None
    cmn = CmnOptions(cmn_window=cmn_window) if cmn_window and cmn_window > 0 else None
    return fb, vad_opts, cmn


def wav_scp_batches(wav_scp, fb, batch_size):
    """(keys, ingest.WavTable, batches [(indices, Nmax)], indices shorter than one frame) of a wav.scp ('key path' lines; pipe
    entries are refused): length-sorted by sample count, at most 10 % padded samples per batch"""
    from . import ingest
    tab = [l.rstrip().split(None, 1) for l in open(wav_scp) if l.strip()]
    keys = [k for k, _ in tab]
    table = ingest.WavTable([p for _, p in tab], int(fb.sample_frequency))
    ok = np.nonzero(table.nsamp >= fb.frame_len)[0]
    short = np.nonzero(table.nsamp < fb.frame_len)[0]
    batches = [(ok[b], int(n)) for b, n in ingest.pad_batches(table.nsamp[ok], batch_size, quantum=1)] if ok.size else []
    return keys, table, batches, short
