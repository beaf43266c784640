"""Audio front end on the MI355X: wav -> (trim, peak-normalise) -> log-mel.

Reference: utils/dsp.py:11-104 `DSP` (wav_to_mel, normalize, denormalize, trim_silence, griffinlim) and the audio half
of preprocess.py:78-89 `Preprocessor._convert_file` (trim_silence, peak normalisation, wav_to_mel).

    dsp = DSP.from_config(config)                    # config['dsp'] of configs/singlespeaker.yaml, unchanged
    mel = dsp.wav_to_mel(y)                          # [n_mels, 1 + len(y) // hop]; numpy in -> numpy out, device in -> device out
    out = dsp.preprocess_batch([y0, y1, ...])        # ragged batch, one pass, no host synchronisation inside
    items = split_items(out)                         # per-item numpy arrays for np.save (this is the one sync)
    out = dsp.preprocess_batch(wavs48k, source_sr=48000)     # load_wav's resampling first, then the same five launches
    rs = dsp.resample_batch(wavs, 48000)             # {'wav' [B, ld], 'wav_len' [B]} at dsp.sample_rate; one launch
    wav = dsp.griffinlim(mel)                        # vocoder.GriffinLim, which shares the bases
    wavs = split_wavs(dsp.griffinlim_batch(mel, mel_len))    # a ragged batch of mels (generate_batch's) -> wavs

HIP device only, like vocoder.GriffinLim: without a device the constructor raises FtError.  The wavs are first gathered
into one zero-padded [B, ld] device buffer and lengths are taken from the host or the device: the intake of a ragged
batch and its contract are ragged.py's.  After that one call is five launches: ft_wav_trim_peak (two), ft_wav_pack, the
DFT of every frame of every item as ONE GEMM over the packed buffer read with a row stride of hop (hip.linear_fwd_as,
whose kernel -- and with it the rounding -- does not depend on the batch: an item alone gives the bits it gives inside
a batch), and ft_mel_project.  Semantics are in include/fwdtaco_hip.h; the float64 restatement the tests compare
against is tests/mel_cpu.py.

PARITY UNPINNED against the reference, as for the vocoder: librosa is not installed here.  What is restated is
librosa's published algorithm: stft(center=True) with ZERO padding of n_fft // 2 (librosa >= 0.10; `pad_mode='reflect'`
gives the older default), periodic Hann window, magnitude, Slaney area-normalised mel basis; effects.trim(top_db,
frame_length=2048, hop_length=512) with ref = the maximum frame power.

Resampling (the reference's load_wav is librosa.load(path, sr=sample_rate), which resamples every file on the way in)
is provided for audio that is already in memory: resample / resample_batch, and the `source_sr` argument of preprocess /
preprocess_batch.  One launch, ft_resample_poly_ragged (csrc/ft_resample.hip), for a ragged batch: the polyphase design
of scipy.signal.resample_poly -- a Kaiser(5.0)-windowed sinc of 20 max(up, down) + 1 taps, zero phase, zero padding --
which is librosa's res_type='polyphase'.  The filter (resample_filter), the ratio and the output length are host
functions of this module, importable without a device; the float64 restatement the tests compare against is
tests/resample_cpu.py, itself held to scipy.  PARITY UNPINNED here too: librosa.load defaults to res_type='soxr_hq', and
neither librosa nor soxr is installed here; what is pinned is the published Kaiser polyphase design, to scipy.

Not provided: trim_long_silences (webrtcvad; the reference's own code for it fails on current numpy) raises FtError at
construction; the file I/O of load_wav / save_wav (reading and writing wav files is out of scope).  normalize /
denormalize are the two element-wise conveniences of the reference's interface; the hot path has them fused into
ft_mel_project / ft_exp_transpose.
"""
import math
import operator
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from . import hip as H
from . import ragged
from .vocoder import GriffinLim, slaney_mel_basis

MEL_PAD_VALUE = -11.5129          # datapath.MEL_PAD_VALUE: what the collators pad mels with

Wav = Union[np.ndarray, torch.Tensor]


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of this module is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


# ----------------------------------------------------------------------------------------------------
# sample-rate conversion: host side (no device needed)
# ----------------------------------------------------------------------------------------------------
RESAMPLE_MAX_RATE = 1024          # max(up, down) after the gcd: every pair of standard rates is far below; table < 100 KB


def _rate(sr, what: str) -> int:
    if isinstance(sr, (bool, float)) or not hasattr(sr, '__index__'):
        raise _lib.FtError(f'resample: {what} must be a positive integer, got {sr!r}')
    sr = operator.index(sr)
    if sr <= 0:
        raise _lib.FtError(f'resample: {what} must be a positive integer, got {sr!r}')
    return sr


def resample_ratio(source_sr: int, target_sr: int) -> Tuple[int, int]:
    """(up, down) = (target_sr, source_sr) / gcd; FtError for rates that are no positive integers or a ratio with
    max(up, down) > 1024"""
    source_sr, target_sr = _rate(source_sr, 'source_sr'), _rate(target_sr, 'target_sr')
    g = math.gcd(source_sr, target_sr)
    up, down = target_sr // g, source_sr // g
    if max(up, down) > RESAMPLE_MAX_RATE:
        raise _lib.FtError(f'resample: {source_sr} -> {target_sr} Hz reduces to {up}/{down}; max(up, down) must be <= '
                           f'{RESAMPLE_MAX_RATE}')
    return up, down


def resample_len(n: int, source_sr: int, target_sr: int) -> int:
    """the number of samples n samples at source_sr become: ceil(n * up / down)"""
    up, down = resample_ratio(source_sr, target_sr)
    n = operator.index(n)
    if n < 0:
        raise _lib.FtError(f'resample: a negative length ({n})')
    return -((-n * up) // down)


def resample_filter(source_sr: int, target_sr: int) -> Tuple[np.ndarray, int]:
    """(h float64 [2 half + 1], half): scipy.signal.resample_poly's default filter -- firwin(2 half + 1, 1 / R, window=
    ('kaiser', 5.0)) * up with R = max(up, down), half = 10 R -- whose centre tap h[half] sits on output n's position
    n * down / up"""
    up, down = resample_ratio(source_sr, target_sr)
    R = max(up, down)
    half = 10 * R
    i = np.arange(2 * half + 1, dtype=np.float64)
    h = (1.0 / R) * np.sinc((i - half) / R) * np.kaiser(2 * half + 1, 5.0)
    h /= h.sum()
    h *= up
    return h, half


def resample_table(h: np.ndarray, half: int, up: int) -> np.ndarray:
    """h -> the kernel's phase-major table, fp32 [up, Tp]: tab[p, t] = h[p + t * up], zero past the last tap; T =
    ceil((2 half + 1) / up) taps per phase, row stride Tp = T | 1 (include/fwdtaco_hip.h: ft_resample_poly_ragged)"""
    T = (2 * half + up) // up
    Tp = T | 1
    idx = np.arange(up)[:, None] + np.arange(T)[None, :] * up
    tab = np.zeros((up, Tp), dtype=np.float32)
    tab[:, :T] = np.where(idx <= 2 * half, np.asarray(h, dtype=np.float64)[np.minimum(idx, 2 * half)], 0.0)
    return tab


def resample_device_table(cache: Dict[Tuple[int, int], Any], up: int, down: int, device):
    """-> (the phase-major coefficient table on the device, half), built once per (up, down) and kept in `cache` (the
    caller's: DSP and speaker.VoiceEncoder each own one)"""
    ent = cache.get((up, down))
    if ent is None:
        h, half = resample_filter(down, up)                      # (up, down) is in lowest terms already
        host = torch.zeros(_lib.query('ft_resample_table_floats', up, down, half), dtype=torch.float32).pin_memory()
        flat = torch.from_numpy(resample_table(h, half, up).reshape(-1))
        host[:flat.numel()] = flat
        tab = _alloc(host.numel(), device=device)
        tab.copy_(host, non_blocking=True)
        ent = cache[(up, down)] = (tab, half, host)              # the pinned source stays alive with the copy
    return ent[0], ent[1]


def resample_intake(wavs, wav_len, device, what: str):
    """-> (wav [B, ld] on the device with 16-byte aligned rows, lens [B] int64 on the device, Lmax, error flag or
    None): the intake of ragged.py, then the rows of a padded batch re-laid where they are not aligned"""
    wav, lens, L, err = ragged.intake(wavs, wav_len, device, what, row_multiple=4, allow_all_empty=False, alloc=_alloc)
    if wav.shape[1] % 4 or not wav.is_contiguous() or wav.data_ptr() % 16:
        buf = _alloc(len(wav), (L + 3) // 4 * 4, device=device)      # columns >= L are never read: every len <= L
        buf[:, :L].copy_(wav)
        wav = buf
    return wav, lens, L, err


def resample_ragged(cache: Dict[Tuple[int, int], Any], wav: torch.Tensor, lens: torch.Tensor, Lmax: int, up: int,
                    down: int, err: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
    """the one launch (ft_resample_poly_ragged) on a batch resample_intake laid out -> {'wav' [B, ldy], 'wav_len' [B]}"""
    ldy = max(4, (-((-Lmax * up) // down) + 3) // 4 * 4)         # from the host's bound: no sync to allocate
    tab, half = (None, 0) if up == down else resample_device_table(cache, up, down, wav.device)
    y, out_len = H.resample_poly_ragged(wav, lens, Lmax, tab, up, down, half, ldy, err, alloc=_alloc)
    return {'wav': y, 'wav_len': out_len}


class DSP:
    def __init__(self, num_mels: int, sample_rate: int, hop_length: int, win_length: int, n_fft: int, fmin: float,
                 fmax: float, peak_norm: bool = False, trim_start_end_silence: bool = True,
                 trim_silence_top_db: float = 60, trim_long_silences: bool = False, vad_sample_rate: int = 16000,
                 vad_window_length: float = 30, vad_moving_average_width: float = 8, vad_max_silence_length: int = 12,
                 device: Union[str, torch.device] = 'cuda', pad_mode: str = 'constant', **kwargs) -> None:
        if trim_long_silences:
            raise _lib.FtError('DSP: trim_long_silences (webrtcvad) is not provided')
        if pad_mode not in ('constant', 'reflect'):
            raise _lib.FtError(f"DSP: pad_mode must be 'constant' or 'reflect', got {pad_mode!r}")
        self.device = torch.device(device)
        if self.device.type != 'cuda' or not torch.cuda.is_available():
            raise _lib.FtError('DSP runs on an MI355X (HIP) device only; there is no CPU fallback')
        if n_fft % 8:
            raise _lib.FtError('DSP: n_fft must be a multiple of 8')
        self.n_mels, self.sample_rate, self.hop_length, self.win_length, self.n_fft = (num_mels, sample_rate, hop_length,
                                                                                       win_length, n_fft)
        self.fmin, self.fmax = fmin, fmax
        self.should_peak_norm = bool(peak_norm)
        self.should_trim_start_end_silence = bool(trim_start_end_silence)
        self.should_trim_long_silences = False
        self.trim_silence_top_db = trim_silence_top_db
        self.vad_sample_rate, self.vad_window_length = vad_sample_rate, vad_window_length
        self.vad_moving_average_width, self.vad_max_silence_length = vad_moving_average_width, vad_max_silence_length
        self.pad_mode = pad_mode
        self.gl = GriffinLim(num_mels, sample_rate, hop_length, win_length, n_fft, fmin, fmax, device=self.device)
        self.Fp = self.gl.Fp
        w, meta = sparse_mel_basis(slaney_mel_basis(sample_rate, n_fft, num_mels, fmin, fmax))
        self.mel_w = torch.from_numpy(w).to(self.device)
        self.mel_meta = torch.from_numpy(meta).to(self.device)
        self._rs_tabs: Dict[Tuple[int, int], Any] = {}          # resampling coefficient tables per (up, down)
        self._len_flag = ragged.LenFlag()                       # the pinned word a device-side length check reports through

    @classmethod
    def from_config(cls, config: Dict[str, Any], **kw) -> 'DSP':
        return cls(**config['dsp'], **kw)

    # ------------------------------------------------------------------------------------------------
    def _wavs(self, wavs: Sequence[Wav], up: int = 1, down: int = 1):
        """the wavs of an STFT: ragged.gather_wavs with rows of a multiple of 4 floats, an all-empty batch refused; under
        pad_mode='reflect' the shortest wav, after a resampling by up / down, must be longer than the padding"""
        out = ragged.gather_wavs(wavs, self.device, 'DSP', row_multiple=4, allow_all_empty=False, alloc=_alloc)
        if self.pad_mode == 'reflect' and -((-min(int(y.shape[0]) for y in wavs) * up) // down) <= self.n_fft // 2:
            raise _lib.FtError(f"DSP: pad_mode='reflect' needs more than n_fft // 2 = {self.n_fft // 2} samples per wav")
        return out

    def _run(self, wav: torch.Tensor, lens: torch.Tensor, Lmax: int, do_trim: bool, peak_mode: int, log_clip: bool,
             pad_value: float) -> Dict[str, torch.Tensor]:
        B, ld = wav.shape
        hop, n_fft, Fp = self.hop_length, self.n_fft, self.Fp
        Tmax = 1 + Lmax // hop                                  # sized from the untrimmed lengths: no sync to allocate
        Tcap = (ld + n_fft + hop - 1) // hop                    # rows per item; its padded signal fits in Tcap * hop
        tp = H.wav_trim_peak(wav, lens, Lmax, do_trim, self.trim_silence_top_db, peak_mode, hop, alloc=_alloc)
        packed, wav_out = H.wav_pack(wav, tp, Tcap * hop, n_fft, self.pad_mode == 'reflect', alloc=_alloc)
        spec = H.linear_fwd_as(packed, hop, self.gl.w_fwd, B * Tcap, n_fft, alloc=_alloc)     # frames read in place
        mel = H.mel_project(spec, Fp, Tcap, tp['mel_len'], self.mel_w, self.mel_meta, self.n_mels, B, Tmax, log_clip,
                            pad_value, alloc=_alloc)
        return {'mel': mel, 'mel_len': tp['mel_len'], 'trim_start': tp['trim_start'], 'trim_end': tp['trim_end'],
                'peak': tp['peak'], 'wav': wav_out[:, :Lmax], 'wav_len': tp['wav_len']}

    # ------------------------------------------------------------------------------------------------
    # ---- sample-rate conversion ----------------------------------------------------------------------
    def _rs_table(self, up: int, down: int):
        """-> (the phase-major coefficient table on the device, half), built once per (up, down)"""
        return resample_device_table(self._rs_tabs, up, down, self.device)

    def _rs_input(self, wavs, wav_len):
        """resample_intake under this object's name and device"""
        return resample_intake(wavs, wav_len, self.device, 'resample_batch')

    def _resample(self, wav: torch.Tensor, lens: torch.Tensor, Lmax: int, up: int, down: int,
                  err: Optional[torch.Tensor]) -> Dict[str, torch.Tensor]:
        return resample_ragged(self._rs_tabs, wav, lens, Lmax, up, down, err)

    def resample_batch(self, wavs, source_sr: int, target_sr: Optional[int] = None,
                       wav_len: Optional[Wav] = None) -> Dict[str, torch.Tensor]:
        """The resampling of DSP.load_wav (librosa.load(path, sr=...)) for a ragged batch, in one launch: source_sr ->
        target_sr (default: self.sample_rate) by scipy.signal.resample_poly's Kaiser polyphase filter (resample_filter).

        wavs: a list of 1-D numpy arrays or tensors of different lengths (gathered as preprocess_batch does), or a padded
        float32 tensor [B, L] with wav_len int64 [B] on the host or the device -- griffinlim_batch's 'wav' and 'wav_len'.
        -> {'wav': float32 [B, ld] on the device, zero at j >= wav_len[b]; 'wav_len': int64 [B] = ceil(len * up / down)},
        ld = ceil(L * up / down) rounded up to a multiple of 4.

        Exact: item b's samples are bit-identical whether it is passed alone or inside any batch, at any position, and
        whatever sits beyond the lengths (NaN, Inf) or in other items.  source_sr == target_sr returns the input bits.

        The lengths follow the contract of ragged.py: a host-side wav_len is checked up front and nothing synchronises;
        a device-side one is clamped inside the kernel and its FtError is raised at the end of the call, after one
        synchronisation, through ONE pinned host word kept on this object -- so one DSP must not run resample_batch
        with a device-side wav_len from two threads or on two streams at once."""
        up, down = resample_ratio(source_sr, self.sample_rate if target_sr is None else target_sr)
        wav, lens, Lmax, err = self._rs_input(wavs, wav_len)
        out = self._resample(wav, lens, Lmax, up, down, err)
        self._len_flag.check(err, ragged.range_message('resample_batch', 'wav_len', 0, Lmax, 'L'))
        return out

    def resample(self, y: Wav, source_sr: int, target_sr: Optional[int] = None) -> Wav:
        """one 1-D wav at source_sr -> ceil(len(y) * up / down) samples at target_sr (default: self.sample_rate); numpy
        in -> numpy out, device tensor in -> device tensor out"""
        if getattr(y, 'ndim', None) != 1:
            raise _lib.FtError('DSP: every wav must be a 1-D array or tensor')
        target_sr = self.sample_rate if target_sr is None else target_sr
        n = resample_len(int(y.shape[0]), source_sr, target_sr)
        if n == 0:
            return np.zeros(0, dtype=np.float32) if isinstance(y, np.ndarray) else \
                torch.zeros(0, dtype=torch.float32, device=self.device)
        wav = self.resample_batch([y], source_sr, target_sr)['wav'][0, :n]
        return wav.cpu().numpy() if isinstance(y, np.ndarray) else wav

    # ------------------------------------------------------------------------------------------------
    def preprocess_batch(self, wavs: Sequence[Wav], source_sr: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """The audio part of Preprocessor._convert_file for a list of wavs of different lengths, in one pass.  Returns
        device tensors: mel [B, n_mels, Tmax] (-11.5129 at frames >= mel_len[b]), mel_len, trim_start, trim_end (int64
        sample indices into the input), peak (max |y| of the trimmed wav), wav [B, Lmax] (trimmed, scaled, zero-padded:
        what a pitch extractor is handed) and wav_len.  As in the reference, an all-zero item under peak_norm=True is
        divided by its peak of 0: its wav and mel are NaN.

        source_sr: the rate of `wavs` if it is not self.sample_rate.  The wavs are then resampled first (the reference's
        load_wav, then _convert_file: one more launch, resample_batch's, and no synchronisation), everything above is
        computed from the resampled signals, and trim_start / trim_end are sample indices into the RESAMPLED signal,
        not into the input.  With source_sr None or equal to self.sample_rate the call issues exactly the launches, and
        returns exactly the bits, of the call without it."""
        trim, peak = self.should_trim_start_end_silence, 1 if self.should_peak_norm else 0
        if source_sr is None or _rate(source_sr, 'source_sr') == self.sample_rate:
            wav, lens, Lmax = self._wavs(wavs)
            return self._run(wav, lens, Lmax, trim, peak, True, MEL_PAD_VALUE)
        up, down = resample_ratio(source_sr, self.sample_rate)
        wav, lens, Lmax = self._wavs(wavs, up, down)
        rs = self._resample(wav, lens, Lmax, up, down, None)
        return self._run(rs['wav'], rs['wav_len'], -((-Lmax * up) // down), trim, peak, True, MEL_PAD_VALUE)

    def preprocess(self, wav: Wav, source_sr: Optional[int] = None) -> Dict[str, torch.Tensor]:
        return self.preprocess_batch([wav], source_sr)

    def wav_to_mel(self, y: Wav, normalize: bool = True) -> Wav:
        """DSP.wav_to_mel: 1-D wav -> [n_mels, 1 + len(y) // hop] (log-mel, or the linear mel with normalize=False)"""
        wav, lens, Lmax = self._wavs([y])
        mel = self._run(wav, lens, Lmax, False, -1, bool(normalize), MEL_PAD_VALUE if normalize else 0.0)['mel'][0]
        return mel.cpu().numpy() if isinstance(y, np.ndarray) else mel

    def trim_silence(self, wav: Wav) -> Wav:
        """librosa.effects.trim(wav, top_db, frame_length=2048, hop_length=512)[0]"""
        dev, lens, Lmax = self._wavs([wav])
        tp = H.wav_trim_peak(dev, lens, Lmax, True, self.trim_silence_top_db, -1, self.hop_length, alloc=_alloc)
        s, e = int(tp['trim_start'][0]), int(tp['trim_end'][0])
        return wav[s:e]

    def normalize(self, mel: Wav) -> Wav:
        if isinstance(mel, np.ndarray):
            return np.log(np.clip(mel, a_min=1.e-5, a_max=None))
        return torch.log(torch.clamp(mel, min=1.e-5))

    def denormalize(self, mel: Wav) -> Wav:
        return np.exp(mel) if isinstance(mel, np.ndarray) else torch.exp(mel)

    def griffinlim(self, mel: Wav, n_iter: int = 32, **kw) -> Wav:
        wav = self.gl.griffinlim(mel, n_iter, **kw)
        return wav.cpu().numpy() if isinstance(mel, np.ndarray) else wav

    def griffinlim_batch(self, mel: Wav, mel_len: Wav, n_iter: int = 32, **kw) -> Dict[str, Wav]:
        """vocoder.GriffinLim.griffinlim_batch: mel [B, n_mels, Tmax], mel_len [B] -> {'wav' [B, hop * (Tmax - 1)],
        'wav_len' [B]}; numpy in -> numpy out (one copy each way), device tensors in -> device tensors out"""
        if not isinstance(mel, np.ndarray):
            return self.gl.griffinlim_batch(mel, mel_len, n_iter, **kw)
        dev = torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)).to(self.device)
        out = self.gl.griffinlim_batch(dev, torch.from_numpy(np.ascontiguousarray(mel_len, dtype=np.int64)), n_iter, **kw)
        return {k: v.cpu().numpy() for k, v in out.items()}


def sparse_mel_basis(basis: np.ndarray):
    """dense [n_mels, F] triangular basis -> (weights [nnz] fp32, meta [n_mels, 3] int32 = first bin, bin count, offset):
    every filter is one run of bins (zeros inside a run are kept), 2 F weights in all instead of n_mels * F"""
    ws, meta, off = [], [], 0
    for row in np.asarray(basis, dtype=np.float64):
        nz = np.flatnonzero(row)
        k0, cnt = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if nz.size else (0, 0)
        ws.append(row[k0:k0 + cnt])
        meta.append((k0, cnt, off))
        off += cnt
    w = np.concatenate(ws).astype(np.float32) if off else np.zeros(0, np.float32)
    if w.size == 0:
        w = np.zeros(1, np.float32)             # an all-zero basis still needs one weight to point at
    return np.ascontiguousarray(w), np.asarray(meta, dtype=np.int32).reshape(-1, 3)


def split_items(out: Dict[str, torch.Tensor]) -> List[Dict[str, Any]]:
    """preprocess_batch's result -> per-item numpy arrays sliced to their lengths (what np.save is handed): mel
    [n_mels, mel_len], wav [wav_len], and the scalars.  Copies to the host: this is the synchronisation point."""
    host = {k: v.cpu().numpy() for k, v in out.items()}
    items = []
    for b in range(host['mel'].shape[0]):
        ml, wl = int(host['mel_len'][b]), int(host['wav_len'][b])
        items.append({'mel': np.ascontiguousarray(host['mel'][b, :, :ml]), 'mel_len': ml,
                      'wav': np.ascontiguousarray(host['wav'][b, :wl]), 'wav_len': wl,
                      'trim_start': int(host['trim_start'][b]), 'trim_end': int(host['trim_end'][b]),
                      'peak': float(host['peak'][b])})
    return items


def split_wavs(out: Dict[str, Wav]) -> List[np.ndarray]:
    """griffinlim_batch's result -> the per-item wavs as numpy arrays cut to wav_len[b].  Copies to the host: this is the
    synchronisation point."""
    wav, wav_len = (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (out['wav'], out['wav_len']))
    return [np.ascontiguousarray(wav[b, :int(wav_len[b])]) for b in range(wav.shape[0])]


__all__ = ['DSP', 'MEL_PAD_VALUE', 'resample_device_table', 'resample_filter', 'resample_intake', 'resample_len',
           'resample_ragged', 'resample_ratio', 'resample_table', 'sparse_mel_basis', 'split_items', 'split_wavs']
