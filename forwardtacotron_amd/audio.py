"""Audio front end on the MI355X: wav -> (trim, peak-normalise) -> log-mel.

Reference: utils/dsp.py:11-104 `DSP` (wav_to_mel, normalize, denormalize, trim_silence, griffinlim) and the audio half
of preprocess.py:78-89 `Preprocessor._convert_file` (trim_silence, peak normalisation, wav_to_mel).

    dsp = DSP.from_config(config)                    # config['dsp'] of configs/singlespeaker.yaml, unchanged
    mel = dsp.wav_to_mel(y)                          # [n_mels, 1 + len(y) // hop]; numpy in -> numpy out, device in -> device out
    out = dsp.preprocess_batch([y0, y1, ...])        # ragged batch, one pass, no host synchronisation inside
    items = split_items(out)                         # per-item numpy arrays for np.save (this is the one sync)
    wav = dsp.griffinlim(mel)                        # vocoder.GriffinLim, which shares the bases
    wavs = split_wavs(dsp.griffinlim_batch(mel, mel_len))    # a ragged batch of mels (generate_batch's) -> wavs

HIP device only, like vocoder.GriffinLim: without a device the constructor raises FtError.  The wavs are first gathered
into one zero-padded [B, ld] device buffer (numpy inputs: one host-to-device copy; device tensors: a fill and one copy
per item, B + 1 small launches, still without a host synchronisation).  After that one call is five launches:
ft_wav_trim_peak (two), ft_wav_pack, the DFT of every frame of every item as ONE GEMM over the packed buffer read with
a row stride of hop (ft_linear_multi_fwd_as with a fixed `as_rows`, so the GEMM kernel -- and with it the rounding --
does not depend on the batch: an item alone gives the bits it gives inside a batch), and ft_mel_project.  Semantics are
in include/fwdtaco_hip.h; the float64 restatement the tests compare against is tests/mel_cpu.py.

PARITY UNPINNED against the reference, as for the vocoder: librosa is not installed here.  What is restated is
librosa's published algorithm: stft(center=True) with ZERO padding of n_fft // 2 (librosa >= 0.10; `pad_mode='reflect'`
gives the older default), periodic Hann window, magnitude, Slaney area-normalised mel basis; effects.trim(top_db,
frame_length=2048, hop_length=512) with ref = the maximum frame power.

Not provided: trim_long_silences (webrtcvad; the reference's own code for it fails on current numpy) raises FtError at
construction; load_wav / save_wav (wav I/O is out of scope).  normalize / denormalize are the two element-wise
conveniences of the reference's interface; the hot path has them fused into ft_mel_project / ft_exp_transpose.
"""
import ctypes
from typing import Any, Dict, List, Sequence, Union

import numpy as np
import torch

from . import _lib
from . import hip as H
from .vocoder import GriffinLim, slaney_mel_basis

MEL_PAD_VALUE = -11.5129          # datapath.MEL_PAD_VALUE: what the collators pad mels with
# the DFT GEMM is always rounded like a launch over this many rows (the 128 x 128 tile), whatever the batch holds
_AS_ROWS = 1 << 20

Wav = Union[np.ndarray, torch.Tensor]


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of this module is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


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
        self._w_ptr = H._ptr_array([self.gl.w_fwd])
        self._col0 = (ctypes.c_int * 1)(0)
        self._outf = (ctypes.c_int * 1)(2 * self.Fp)

    @classmethod
    def from_config(cls, config: Dict[str, Any], **kw) -> 'DSP':
        return cls(**config['dsp'], **kw)

    # ------------------------------------------------------------------------------------------------
    def _gather(self, wavs: Sequence[Wav]):
        """list of 1-D wavs -> (wav [B, ld] zero-padded device tensor, lens [B] int64 device tensor, Lmax)"""
        if len(wavs) == 0:
            raise _lib.FtError('DSP: an empty batch')
        lens = []
        for y in wavs:
            if getattr(y, 'ndim', None) != 1:
                raise _lib.FtError('DSP: every wav must be a 1-D array or tensor')
            lens.append(int(y.shape[0]))
        Lmax = max(lens)
        if Lmax == 0:
            raise _lib.FtError('DSP: every wav of the batch is empty')
        if self.pad_mode == 'reflect' and min(lens) <= self.n_fft // 2:
            raise _lib.FtError(f"DSP: pad_mode='reflect' needs more than n_fft // 2 = {self.n_fft // 2} samples per wav")
        ld = (Lmax + 3) // 4 * 4
        if all(isinstance(y, np.ndarray) for y in wavs):
            host = np.zeros((len(wavs), ld), dtype=np.float32)
            for b, y in enumerate(wavs):
                host[b, :lens[b]] = y
            wav = torch.from_numpy(host).to(self.device)
        else:
            wav = torch.zeros(len(wavs), ld, dtype=torch.float32, device=self.device)
            for b, y in enumerate(wavs):
                wav[b, :lens[b]] = torch.as_tensor(y).to(self.device, torch.float32)
        return wav, torch.tensor(lens, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True), Lmax

    def _run(self, wav: torch.Tensor, lens: torch.Tensor, Lmax: int, do_trim: bool, peak_mode: int, log_clip: bool,
             pad_value: float) -> Dict[str, torch.Tensor]:
        B, ld = wav.shape
        hop, n_fft, Fp = self.hop_length, self.n_fft, self.Fp
        Tmax = 1 + Lmax // hop                                  # sized from the untrimmed lengths: no sync to allocate
        Tcap = (ld + n_fft + hop - 1) // hop                    # rows per item; its padded signal fits in Tcap * hop
        tp = H.wav_trim_peak(wav, lens, Lmax, do_trim, self.trim_silence_top_db, peak_mode, hop, alloc=_alloc)
        packed, wav_out = H.wav_pack(wav, tp, Tcap * hop, n_fft, self.pad_mode == 'reflect', alloc=_alloc)
        rows = B * Tcap
        spec = _alloc(rows, 2 * Fp, device=self.device)
        c_void_p = ctypes.c_void_p
        _lib.call('ft_linear_multi_fwd_as', packed.data_ptr(), hop, 1, ctypes.cast(self._w_ptr, c_void_p), None,
                  spec.data_ptr(), 2 * Fp, ctypes.cast(self._col0, c_void_p), ctypes.cast(self._outf, c_void_p), rows,
                  n_fft, _AS_ROWS, H._stream())
        mel = H.mel_project(spec, Fp, Tcap, tp['mel_len'], self.mel_w, self.mel_meta, self.n_mels, B, Tmax, log_clip,
                            pad_value, alloc=_alloc)
        return {'mel': mel, 'mel_len': tp['mel_len'], 'trim_start': tp['trim_start'], 'trim_end': tp['trim_end'],
                'peak': tp['peak'], 'wav': wav_out[:, :Lmax], 'wav_len': tp['wav_len']}

    # ------------------------------------------------------------------------------------------------
    def preprocess_batch(self, wavs: Sequence[Wav]) -> Dict[str, torch.Tensor]:
        """The audio part of Preprocessor._convert_file for a list of wavs of different lengths, in one pass.  Returns
        device tensors: mel [B, n_mels, Tmax] (-11.5129 at frames >= mel_len[b]), mel_len, trim_start, trim_end (int64
        sample indices into the input), peak (max |y| of the trimmed wav), wav [B, Lmax] (trimmed, scaled, zero-padded:
        what a pitch extractor is handed) and wav_len.  As in the reference, an all-zero item under peak_norm=True is
        divided by its peak of 0: its wav and mel are NaN."""
        wav, lens, Lmax = self._gather(wavs)
        return self._run(wav, lens, Lmax, self.should_trim_start_end_silence, 1 if self.should_peak_norm else 0, True,
                         MEL_PAD_VALUE)

    def preprocess(self, wav: Wav) -> Dict[str, torch.Tensor]:
        return self.preprocess_batch([wav])

    def wav_to_mel(self, y: Wav, normalize: bool = True) -> Wav:
        """DSP.wav_to_mel: 1-D wav -> [n_mels, 1 + len(y) // hop] (log-mel, or the linear mel with normalize=False)"""
        wav, lens, Lmax = self._gather([y])
        mel = self._run(wav, lens, Lmax, False, -1, bool(normalize), MEL_PAD_VALUE if normalize else 0.0)['mel'][0]
        return mel.cpu().numpy() if isinstance(y, np.ndarray) else mel

    def trim_silence(self, wav: Wav) -> Wav:
        """librosa.effects.trim(wav, top_db, frame_length=2048, hop_length=512)[0]"""
        dev, lens, Lmax = self._gather([wav])
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


__all__ = ['DSP', 'MEL_PAD_VALUE', 'sparse_mel_basis', 'split_items', 'split_wavs']
