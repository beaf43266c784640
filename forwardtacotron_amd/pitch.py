"""Raw pitch on the MI355X: pYIN for a ragged batch of wavs.

Reference: pitch_extraction/pitch_extractor.py:24-78 (LibrosaPitchExtractor, new_pitch_extractor_from_config) and
preprocess.py:90, where `self.pitch_extractor(y)` follows `wav_to_mel(y)` and its result is saved as raw_pitch/{id}.npy.

    ext = new_pitch_extractor_from_config(config)        # 'librosa' -> LibrosaPitchExtractor
    pitch = ext(y)                                       # [1 + len(y) // hop]; numpy in -> numpy out, device in -> device out
    out = dsp.preprocess_batch(wavs)
    res = ext.extract_batch(out['wav'], out['wav_len'])  # {'pitch' [B, Tmax], 'pitch_len' [B], 'voiced_prob' [B, Tmax]}
    write_raw_pitch(res, item_ids, paths.raw_pitch)      # the files pitch_energy.extract_pitch_energy reads

HIP device only: without a device the constructor raises FtError.  extract_batch is three launches -- ft_pyin_cmnd,
ft_pyin_observe, ft_pyin_viterbi (csrc/ft_pitch.hip) -- behind the intake of the ragged batch (ragged.py, which states
the contract; here a device-side length is clamped silently, so lengths on the device or on the host never
synchronise).  The algorithm is probabilistic YIN (Mauch & Dixon 2014) with librosa.pyin's documented defaults:
n_thresholds=100, beta_parameters=(2, 18), boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92,
switch_prob=0.01, no_trough_prob=0.01, win_length = frame_length // 2, center=True with zero padding.  Semantics are
in include/fwdtaco_hip.h and DESIGN.md section 7; the float64 and fp32 restatements the tests compare against are
tests/pyin_cpu.py.  pyin_tables (the host tables and the derived sizes) needs no device.

PARITY UNPINNED against the reference, as for the rest of the audio front end: librosa is not installed here.  What is
pinned is the written definition, and it differs from librosa.pyin on purpose in three places: the difference function
is formed directly as squared differences in fp32 (librosa's FFT route computes energy - 2 acf, which cancels, and
patches that with 1e-6 cut-offs); a candidate beyond the top pitch bin is dropped (librosa clips it into the top bin);
the floors are fp32's FLT_MIN (librosa: float64's tiny).

Not provided: 'pyworld' (DIO is a chain of heuristics without a closed published definition) raises FtError, as DSP does
for trim_long_silences.
"""
import math
import os
from fractions import Fraction
from typing import Any, Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from . import hip as H
from . import ragged

Wav = Union[np.ndarray, torch.Tensor]

N_THRESHOLDS = 100
BETA = (2, 18)
BOLTZMANN = 2.0
BINS_PER_SEMITONE = 10                      # resolution = 0.1
MAX_TRANSITION_RATE = 35.92
SWITCH_PROB = 0.01
NO_TROUGH_PROB = 0.01
FLT_MIN = float(np.finfo(np.float32).tiny)
# what the kernels hold (include/fwdtaco_hip.h)
MAX_PERIODS = 1024
MAX_BINS = 1024                             # 2N <= 2048 states
MAX_HALF = 2048
CMND_LDS_BYTES = 65536
VITERBI_LDS_BYTES = 65536
_CMND_FRAMES = 4


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of this module is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)


def _beta_2_18_steps(n: int):
    """(bp [n], bpc [n + 1]) of the Beta(2, 18) cdf F(x) = 1 - (1 - x)^19 - 19 x (1 - x)^18 on the grid k / n: bp[k] =
    F((k + 1) / n) - F(k / n) and its prefix sums bpc[m] = F(m / n).  With x = k / n, 1 - F = (n - k)^18 (n + 18 k) /
    n^19 is a ratio of integers, so every entry is the exact value rounded once (in floating point 1 - x loses half an
    ulp, which the 19th power multiplies by 19)."""
    den = n ** 19
    surv = [(n - k) ** 18 * (n + 18 * k) for k in range(n + 1)]
    bp = np.array([float(Fraction(surv[k] - surv[k + 1], den)) for k in range(n)], dtype=np.float64)
    bpc = np.array([float(Fraction(den - surv[m], den)) for m in range(n + 1)], dtype=np.float64)
    return bp, bpc


def cmnd_lds_bytes(frame_length: int, hop_length: int, pmax: int) -> int:
    """LDS of ft_pyin_cmnd: the samples of four consecutive frames and their difference functions"""
    span = (frame_length + (_CMND_FRAMES - 1) * hop_length + 8 + 3) & ~3
    return 4 * (span + _CMND_FRAMES * ((pmax + 4) & ~3))


def viterbi_lds_rows(N: int, half: int) -> int:
    """the back-pointer rows ft_pyin_viterbi's LDS plan holds beside its arrays (ft_pyin_viterbi_rows): (4N + 6 half + 33)
    floats, 2N flag bytes, then rows of 2N 16-bit entries, at most 32, within 65536 bytes; 0: the plan does not fit"""
    rows_off = (4 * (4 * N + 6 * half + 33) + 2 * N + 3) & ~3
    return max(0, min(32, (VITERBI_LDS_BYTES - rows_off) // (4 * N))) if rows_off < VITERBI_LDS_BYTES else 0


def pyin_tables(sr, fmin, fmax, frame_length, hop_length) -> Dict[str, Any]:
    """The derived sizes and host tables of pYIN for one configuration; no device needed.

    Sizes: W, pmin, pmax, P, N, half, band (= 2 half + 1), nE.  Tables as float32 (float64 rounded once): thr, bp [100],
    bpc [101], E, C [nE], tri, logtri [band], norm, lognorm, freqs [N]; scalars ls, lw, LZ, lN (Python floats holding
    the fp32 values).  't64' holds the same tables before the rounding.  FtError for a configuration the definition or
    the kernels do not hold."""
    for name, v in (('sample_rate', sr), ('frame_length', frame_length), ('hop_length', hop_length)):
        if isinstance(v, (bool, float)) or not hasattr(v, '__index__') or int(v) <= 0:
            raise _lib.FtError(f'pyin: {name} must be a positive integer, got {v!r}')
    sr, fl, hop = int(sr), int(frame_length), int(hop_length)
    fmin, fmax = float(fmin), float(fmax)
    if fl < 4 or fl % 2:
        raise _lib.FtError(f'pyin: frame_length must be even and at least 4, got {fl}')
    if not fmin > 0:
        raise _lib.FtError(f'pyin: fmin must be positive, got {fmin}')
    if not (fmax > fmin and math.isfinite(fmax)):
        raise _lib.FtError(f'pyin: fmax ({fmax}) must be above fmin ({fmin})')
    W = fl // 2
    pmin = max(int(math.floor(sr / fmax)), 1)
    pmax = min(int(math.ceil(sr / fmin)), fl - W - 1)
    if pmax < pmin + 2:
        raise _lib.FtError(f'pyin: periods {pmin}..{pmax}: frame_length {fl} holds fewer than three periods between '
                           f'sr / fmax and sr / fmin')
    P = pmax - pmin + 1
    N = int(math.floor(12 * BINS_PER_SEMITONE * math.log2(fmax / fmin))) + 1
    half = BINS_PER_SEMITONE * int(round(MAX_TRANSITION_RATE * 12 * hop / sr)) // 2
    if N > MAX_BINS:
        raise _lib.FtError(f'pyin: fmin {fmin} .. fmax {fmax} gives 2N = {2 * N} HMM states; the Viterbi kernel holds at '
                           f'most {2 * MAX_BINS}')
    if half > MAX_HALF:
        raise _lib.FtError(f'pyin: hop_length {hop} at {sr} Hz gives a transition band of {2 * half + 1} bins; at most '
                           f'{2 * MAX_HALF + 1}')
    if viterbi_lds_rows(N, half) < 1:
        raise _lib.FtError(f'pyin: 2N = {2 * N} states with a transition band of {2 * half + 1} bins do not fit the Viterbi '
                           f"kernel's LDS plan ({VITERBI_LDS_BYTES} bytes)")
    if P > MAX_PERIODS:
        raise _lib.FtError(f'pyin: {P} periods per frame; the observation kernel holds at most {MAX_PERIODS}')
    if cmnd_lds_bytes(fl, hop, pmax) > CMND_LDS_BYTES:
        raise _lib.FtError(f'pyin: frame_length {fl} with hop_length {hop} needs {cmnd_lds_bytes(fl, hop, pmax)} bytes of '
                           f'LDS in the difference kernel; at most {CMND_LDS_BYTES}')
    nE = (P + 1) // 2 + 1
    edges = np.arange(N_THRESHOLDS + 1, dtype=np.float64) / N_THRESHOLDS
    t64: Dict[str, np.ndarray] = {}
    t64['thr'] = edges[1:].copy()
    t64['bp'], t64['bpc'] = _beta_2_18_steps(N_THRESHOLDS)
    n = np.arange(nE, dtype=np.float64)
    t64['E'] = np.exp(-BOLTZMANN * n)
    with np.errstate(divide='ignore'):
        t64['C'] = np.where(n > 0, (1.0 - math.exp(-BOLTZMANN)) / (1.0 - np.exp(-BOLTZMANN * np.maximum(n, 1))), 0.0)
    j = np.arange(2 * half + 1, dtype=np.float64)
    t64['tri'] = 1.0 - np.abs(j - half) / (half + 1)         # scipy.signal.get_window('triangle', 2 half + 1, False)
    k = np.arange(N)
    lo, hi = np.maximum(k - half, 0), np.minimum(k + half, N - 1)           # the targets inside [0, N)
    tc = np.concatenate([[0.0], np.cumsum(t64['tri'])])
    t64['norm'] = tc[hi - k + half + 1] - tc[lo - k + half]
    t64['logtri'] = np.log(t64['tri'])
    t64['lognorm'] = np.log(t64['norm'])
    t64['freqs'] = fmin * 2.0 ** (k / (12.0 * BINS_PER_SEMITONE))
    out: Dict[str, Any] = dict(sr=sr, fmin=fmin, fmax=fmax, frame_length=fl, hop_length=hop, W=W, pmin=pmin, pmax=pmax,
                               P=P, N=N, half=half, band=2 * half + 1, nE=nE, t64=t64)
    for name, v in t64.items():
        out[name] = np.ascontiguousarray(v, dtype=np.float32)
    for name, v in (('ls', math.log(1.0 - SWITCH_PROB)), ('lw', math.log(SWITCH_PROB)), ('LZ', math.log(FLT_MIN)),
                    ('lN', -math.log(N))):
        out[name] = float(np.float32(v))
    return out


_DEVICE_TABLES = ('thr', 'bp', 'bpc', 'E', 'C', 'logtri', 'lognorm', 'freqs')


class LibrosaPitchExtractor:
    """LibrosaPitchExtractor of the reference (its constructor arguments, its __call__) on HIP kernels, plus
    extract_batch for a ragged batch."""

    def __init__(self, fmin: float, fmax: float, sample_rate: int, frame_length: int, hop_length: int,
                 device: Union[str, torch.device] = 'cuda') -> None:
        self.tables = pyin_tables(sample_rate, fmin, fmax, frame_length, hop_length)
        self.fmin, self.fmax, self.sample_rate = fmin, fmax, sample_rate
        self.frame_length, self.hop_length = frame_length, hop_length
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise _lib.FtError('LibrosaPitchExtractor runs on an MI355X (HIP) device only; there is no CPU fallback')
        self._dev = {k: torch.from_numpy(self.tables[k]).to(self.device) for k in _DEVICE_TABLES}

    # ------------------------------------------------------------------------------------------------
    def _gather(self, wavs: Sequence[Wav]):
        """ragged.gather_wavs with this extractor's parameters (the stage tests and tools/bench_pitch.py start here)"""
        return ragged.gather_wavs(wavs, self.device, 'extract_batch', alloc=_alloc)

    def _input(self, wav, wav_len):
        """the intake of ragged.py (a device-side wav_len gets no flag: the kernels clamp it silently), with a one-column
        buffer for a padded batch of L == 0"""
        wav, lens, L, _ = ragged.intake(wav, wav_len, self.device, 'extract_batch', flag=False, alloc=_alloc)
        if wav.shape[1] == 0 or not wav.is_contiguous():
            buf = _alloc(len(wav), max(1, L), device=self.device)    # columns >= L are never read: every len <= L
            if L:
                buf.copy_(wav)
            wav = buf
        return wav, lens, L

    def stages(self, wav: torch.Tensor, lens: torch.Tensor, Lmax: int, debug: bool = False) -> Dict[str, torch.Tensor]:
        """the three launches on a gathered batch; returns every intermediate (dn, frames, lo_v, lo_u, vp, state, score,
        pitch, and with debug the observation kernel's prob and info)"""
        tb = self.tables
        Tmax = 1 + Lmax // tb['hop_length']
        dn, frames = H.pyin_cmnd(wav, lens, Lmax, tb['frame_length'], tb['hop_length'], tb['pmin'], tb['pmax'], Tmax,
                                 alloc=_alloc)
        out = {'dn': dn, 'frames': frames}
        out.update(H.pyin_observe(dn, frames, tb, self._dev, debug=debug, alloc=_alloc))
        out.update(H.pyin_viterbi(out['lo_v'], out['lo_u'], frames, tb, self._dev, alloc=_alloc))
        return out

    def extract_batch(self, wav, wav_len: Optional[Wav] = None) -> Dict[str, torch.Tensor]:
        """pYIN of a ragged batch.  wav: a padded float32 [B, L] tensor with wav_len int64 [B] on the host or the device
        -- preprocess_batch's 'wav' and 'wav_len' as they are -- or a list of 1-D numpy arrays or tensors.
        -> {'pitch': float32 [B, Tmax] in Hz, 0 on unvoiced frames and at t >= pitch_len[b]; 'pitch_len': int64 [B] =
        1 + wav_len // hop_length (wav_to_mel's mel_len); 'voiced_prob': float32 [B, Tmax], 0 at t >= pitch_len[b]}, on
        the device, Tmax = 1 + L // hop_length.

        Exact: an item's pitch and voiced_prob are bit-identical alone and inside any batch at any position, whatever
        sits beyond the lengths (NaN, Inf) or in other items.  A wav_len on the device is clamped into [0, L] inside the
        kernels; one on the host is checked here.  An item that holds NaN or Inf finishes like any other (every loop is
        bounded by host values); what it returns on the frames such a sample reaches means nothing -- finite pitches or
        0, a NaN lag of the difference function being no trough -- and its other frames are what they are without it."""
        wav, lens, Lmax = self._input(wav, wav_len)
        st = self.stages(wav, lens, Lmax)
        return {'pitch': st['pitch'], 'pitch_len': st['frames'], 'voiced_prob': st['vp']}

    def __call__(self, wav: Wav) -> Wav:
        """one 1-D wav -> its pitch track [1 + len(wav) // hop_length]; numpy in -> numpy float32 out, device tensor in ->
        device tensor out"""
        if getattr(wav, 'ndim', None) != 1:
            raise _lib.FtError('LibrosaPitchExtractor: expected a 1-D wav')
        n = 1 + int(wav.shape[0]) // self.hop_length
        pitch = self.extract_batch([wav])['pitch'][0, :n]
        return pitch.cpu().numpy() if isinstance(wav, np.ndarray) else pitch


def new_pitch_extractor_from_config(config: Dict[str, Any], device: Union[str, torch.device] = 'cuda'):
    preproc_config = config['preprocessing']
    pitch_extractor_type = preproc_config['pitch_extractor']
    if pitch_extractor_type == 'librosa':
        return LibrosaPitchExtractor(fmin=preproc_config['pitch_min_freq'], fmax=preproc_config['pitch_max_freq'],
                                     frame_length=preproc_config['pitch_frame_length'],
                                     sample_rate=config['dsp']['sample_rate'], hop_length=config['dsp']['hop_length'],
                                     device=device)
    if pitch_extractor_type == 'pyworld':
        raise _lib.FtError("pitch_extractor 'pyworld' (DIO) is not provided; use pitch_extractor: librosa")
    raise ValueError(f'Invalid pitch extractor type: {pitch_extractor_type}, choices: [librosa, pyworld].')


def write_raw_pitch(result: Dict[str, torch.Tensor], item_ids: Sequence, raw_pitch_dir: Union[str, os.PathLike]) -> List[str]:
    """extract_batch's result -> raw_pitch/{id}.npy per item: float32 [pitch_len], the file pitch_energy's loaders read
    (preprocess.py:95).  Copies to the host: this is the synchronisation point.  Returns the paths."""
    pitch, plen = result['pitch'].cpu().numpy(), result['pitch_len'].cpu().numpy()
    if len(item_ids) != pitch.shape[0]:
        raise _lib.FtError(f'write_raw_pitch: {len(item_ids)} item ids for {pitch.shape[0]} items')
    os.makedirs(raw_pitch_dir, exist_ok=True)
    paths = []
    for b, item_id in enumerate(item_ids):
        path = os.path.join(raw_pitch_dir, f'{item_id}.npy')
        np.save(path, np.ascontiguousarray(pitch[b, :int(plen[b])], dtype=np.float32), allow_pickle=False)
        paths.append(path)
    return paths


__all__ = ['LibrosaPitchExtractor', 'new_pitch_extractor_from_config', 'pyin_tables', 'write_raw_pitch']
