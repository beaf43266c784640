"""Mel inversion + Griffin-Lim on the MI355X (BASELINE configs[0]'s vocoder leg).

Reference: utils/dsp.py:80-94 `DSP.griffinlim(mel, n_iter=32)` -- exp, librosa `mel_to_stft(power=1)`, librosa
`griffinlim(n_iter, hop_length, win_length)` -- called from gen_forward.py:109-116 on `gen['mel_post']`.

    gl = GriffinLim.from_config(config)             # config['dsp'] as in configs/singlespeaker.yaml:8-26
    wav = gl.griffinlim(gen['mel_post'][0])         # log-mel [n_mels, T] (device tensor or numpy) -> wav [hop*(T-1)]

MI355X-first: both transforms are GEMMs on the package's MFMA kernels.  The forward DFT of all frames is ONE
`ft_linear_fwd` whose A operand is the zero-padded signal itself read with a row stride of `hop` samples (the frames
overlap in memory, nothing is gathered), against a [2F, n_fft] basis that has the Hann window folded in; the inverse is
one GEMM against the [n_fft, 2F] inverse basis (window folded in again) followed by an ordered overlap-add gather.  The
phase update and the mel pseudo-inverse steps are small element-wise kernels (csrc/ft_dsp.hip).  32 iterations on a
~800-frame utterance are 64 GEMMs of 1.7 GFLOP.

A RAGGED BATCH goes through `griffinlim_batch(mel, mel_len)` (generate_batch's 'mel_post' and 'mel_len'): every item
sits at a fixed stride of Tcap rows in one packed buffer (`gl_batch_geometry`), so each transform of every iteration is
ONE GEMM for the whole batch and each element-wise step ONE launch (the *_ragged kernels of csrc/ft_dsp.hip, lengths
read on the device).  Every GEMM of that path is `hip.linear_fwd_as`, whose kernel -- and the rounding -- never depends
on the batch: an item's samples are bit-identical alone and inside any batch.  How mel_len is taken from the host or
the device is the contract of ragged.py.

PARITY UNPINNED against the reference: librosa is not installed in this image and the reference ships no audio
fixture.  The oracle is oracle/gl_oracle.py (numpy, FFT-based -- an independent route to the same published algorithm);
tests/test_gpu_vocoder.py compares step by step.  Differences from librosa that are ours, not the reference's:
  * mel inversion: librosa runs scipy's L-BFGS-B NNLS from the clipped least-squares solution; here the same start is
    followed by `nnls_iter` projected-gradient steps (GEMMs), see the oracle's header;
  * the random initial phases come from numpy's default_rng(seed) on the host (librosa: default_rng(random_state)).
"""
import os
from typing import Any, Dict, Optional, Union

import numpy as np
import torch

from . import _lib
from . import hip as H
from . import ragged


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    lin = f / f_sp
    return np.where(f >= 1000.0, 1000.0 / f_sp + np.log(np.maximum(f, 1e-10) / 1000.0) / (np.log(6.4) / 27.0), lin)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    return np.where(m >= 1000.0 / f_sp, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 1000.0 / f_sp)), f_sp * m)


def slaney_mel_basis(sr: int, n_fft: int, n_mels: int, fmin: float, fmax: float) -> np.ndarray:
    """Slaney-scale triangular filters with area normalisation (what librosa.filters.mel builds by default)"""
    freqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    pts = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    up = (freqs[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
    down = (pts[2:, None] - freqs[None, :]) / (pts[2:] - pts[1:-1])[:, None]
    w = np.clip(np.minimum(up, down), 0, None)
    return w * (2.0 / (pts[2:] - pts[:-2]))[:, None]


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of the batched path is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


def gl_batch_geometry(B: int, Tmax: int, n_fft: int, hop: int) -> Dict[str, int]:
    """Layout of a ragged batch of B items of at most Tmax frames (pure host arithmetic).  Item b owns rows
    [b * Tcap, (b + 1) * Tcap) of every frame-major buffer and samples [b * stride, (b + 1) * stride) of the packed
    signal, stride = Tcap * hop >= n_fft + hop * (Tmax - 1) = its longest padded signal; the packed signal has an n_fft
    zero tail so that the last row of the one STFT GEMM (ldx = hop) reads inside the buffer."""
    if B < 1 or Tmax < 1 or hop < 1 or n_fft < hop:
        raise _lib.FtError(f'gl_batch_geometry: bad sizes (B {B}, Tmax {Tmax}, n_fft {n_fft}, hop {hop})')
    Tcap = Tmax - 1 + -(-n_fft // hop)
    rows = B * Tcap
    return {'Tcap': Tcap, 'rows': rows, 'stride': Tcap * hop, 'packed': rows * hop + n_fft,
            'last_read_end': (rows - 1) * hop + n_fft, 'wav_ld': hop * (Tmax - 1)}


def window_sumsquare_f32(w2: np.ndarray, N: int, n_fft: int, hop: int) -> np.ndarray:
    """What ft_overlap_add_ragged divides an N-frame item by, restated on the host: for every sample t of the padded
    signal, the fp32 sum of w2[t - n * hop] over the frames n < N that cover t, in ascending n (w2 = the squared window
    rounded to fp32).  Head, periodic middle and tail -- and their overlap for N < n_fft / hop -- all come out of the one
    rule.  At most ceil(n_fft / hop) positive terms: within (1 + ceil(n_fft / hop)) * 2^-24 relative of the exact sum."""
    w2 = np.asarray(w2, dtype=np.float32)
    out = np.zeros(n_fft + hop * (N - 1), dtype=np.float32)
    for n in range(N):                         # ascending n: every sample adds its frames in the kernel's order
        out[n * hop:n * hop + n_fft] += w2
    return out


class GriffinLim:
    def __init__(self, num_mels: int, sample_rate: int, hop_length: int, win_length: int, n_fft: int, fmin: float,
                 fmax: float, device: Union[str, torch.device] = 'cuda', nnls_iter: int = 64, momentum: float = 0.99,
                 **_unused) -> None:
        self.n_mels, self.sr, self.hop, self.win_length, self.n_fft = num_mels, sample_rate, hop_length, win_length, n_fft
        self.fmin, self.fmax, self.nnls_iter, self.momentum = fmin, fmax, nnls_iter, momentum
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.FtError('GriffinLim runs on an MI355X (HIP) device only; there is no CPU fallback')
        if n_fft % 4 or hop_length % 4 or not 0 < hop_length <= n_fft or win_length > n_fft:
            raise _lib.FtError('GriffinLim: n_fft and hop_length must be multiples of 4, hop <= n_fft, win <= n_fft')
        F = n_fft // 2 + 1
        self.F, self.Fp = F, (F + 3) // 4 * 4
        n = np.arange(win_length)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * n / win_length)                 # periodic Hann, centred in n_fft
        lpad = (n_fft - win_length) // 2
        self.window = np.pad(win, (lpad, n_fft - win_length - lpad))
        k = np.arange(n_fft)
        ang = 2 * np.pi * np.outer(np.arange(F), k) / n_fft                 # [F, n_fft]
        fwd = np.zeros((2 * self.Fp, n_fft))
        fwd[:F] = np.cos(ang) * self.window                                 # Re X_m =  sum_k w_k x_k cos
        fwd[self.Fp:self.Fp + F] = -np.sin(ang) * self.window               # Im X_m = -sum_k w_k x_k sin
        c = np.full(F, 2.0)
        c[0] = 1.0
        if n_fft % 2 == 0:
            c[-1] = 1.0
        inv = np.zeros((n_fft, 2 * self.Fp))
        inv[:, :F] = (np.cos(ang) * c[:, None]).T * self.window[:, None] / n_fft
        inv[:, self.Fp:self.Fp + F] = (-np.sin(ang) * c[:, None]).T * self.window[:, None] / n_fft
        B = slaney_mel_basis(sample_rate, n_fft, num_mels, fmin, fmax)      # [n_mels, F]
        Bp = np.zeros((num_mels, self.Fp))
        Bp[:, :F] = B
        pinv = np.zeros((self.Fp, num_mels))
        pinv[:F] = np.linalg.pinv(B)
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)
        self.w_fwd, self.w_inv = f32(fwd), f32(inv)
        self.w2 = f32(self.window ** 2)                                     # the batched overlap-add's fp32 squared window
        self.mel_basis, self.mel_basis_t, self.mel_pinv = f32(Bp), f32(Bp.T), f32(pinv)
        self.inv_lip = float(1.0 / np.linalg.norm(B, 2) ** 2)
        self._inv_wss: Dict[int, torch.Tensor] = {}
        self._len_flag = ragged.LenFlag()                   # the pinned word a device-side mel_len check reports through

    @classmethod
    def from_config(cls, config: Dict[str, Any], **kw) -> 'GriffinLim':
        return cls(**config['dsp'], **kw)

    # ------------------------------------------------------------------------------------------------
    def _wss(self, N: int) -> torch.Tensor:
        t = self._inv_wss.get(N)
        if t is None:
            wss = np.zeros(self.n_fft + self.hop * (N - 1))
            w2 = self.window ** 2
            for n in range(N):
                wss[n * self.hop:n * self.hop + self.n_fft] += w2
            inv = np.where(wss > np.finfo(np.float32).tiny, 1.0 / np.maximum(wss, 1e-300), 1.0)
            t = torch.from_numpy(inv.astype(np.float32)).to(self.device)
            self._inv_wss[N] = t
        return t

    def mel_to_stft(self, mel_log: torch.Tensor) -> torch.Tensor:
        """log-mel [n_mels, N] (device) -> magnitudes [N, Fp] (frames-major, columns >= F are zero)"""
        H._chk(mel_log, 'mel')
        C, N = mel_log.shape
        if C != self.n_mels:
            raise _lib.FtError(f'mel_to_stft: expected {self.n_mels} mel channels, got {C}')
        st = H._stream()
        M = torch.empty(N, C, device=self.device)
        _lib.call('ft_exp_transpose', mel_log.data_ptr(), M.data_ptr(), C, N, st)
        X = H.linear_fwd(M, self.mel_pinv, relu=True)                     # clipped least squares [N, Fp]
        for _ in range(self.nnls_iter):
            R = H.linear_fwd(X, self.mel_basis)                           # [N, n_mels]
            _lib.call('ft_sub', R.data_ptr(), M.data_ptr(), R.data_ptr(), R.numel(), st)
            G = H.linear_fwd(R, self.mel_basis_t)                         # [N, Fp]
            _lib.call('ft_nnls_step', X.data_ptr(), G.data_ptr(), self.inv_lip, X.numel(), st)
        return X

    def istft_padded(self, proj: torch.Tensor) -> torch.Tensor:
        """split spectrum [N, 2Fp] -> zero-padded signal [n_fft + hop*(N-1)] (the signal starts at n_fft // 2)"""
        N = proj.shape[0]
        frames = H.linear_fwd(proj, self.w_inv)                            # [N, n_fft], window folded in
        ypad = torch.empty(self.n_fft + self.hop * (N - 1), device=self.device)
        _lib.call('ft_overlap_add', frames.data_ptr(), self._wss(N).data_ptr(), ypad.data_ptr(), N, self.n_fft, self.hop,
                  H._stream())
        return ypad

    def stft_of_padded(self, ypad: torch.Tensor, N: int) -> torch.Tensor:
        """zero-padded signal -> split spectrum [N, 2Fp]: one GEMM over the overlapping frames (row stride = hop)"""
        out = torch.empty(N, 2 * self.Fp, device=self.device)
        _lib.call('ft_linear_fwd', ypad.data_ptr(), self.hop, self.w_fwd.data_ptr(), None, out.data_ptr(), 2 * self.Fp, N,
                  self.n_fft, 2 * self.Fp, 0, 0, 0, 0, H._stream())
        return out

    def stft(self, y: torch.Tensor) -> torch.Tensor:
        """y [L] -> split spectrum [1 + L // hop, 2Fp]"""
        H._chk(y, 'y')
        pad = self.n_fft // 2
        ypad = torch.zeros(y.numel() + 2 * pad, device=self.device)
        ypad[pad:pad + y.numel()] = y
        return self.stft_of_padded(ypad, 1 + y.numel() // self.hop)

    def griffinlim_from_stft(self, S: torch.Tensor, n_iter: int = 32, init_u: Optional[torch.Tensor] = None,
                             seed: Optional[int] = None) -> torch.Tensor:
        """S [N, Fp] magnitudes -> wav [hop*(N-1)].  init_u [N, Fp] in [0,1): the initial phases / (2 pi)."""
        H._chk(S, 'S')
        N, Fp = S.shape
        if Fp != self.Fp:
            raise _lib.FtError(f'griffinlim: expected {self.Fp} (padded) frequency columns, got {Fp}')
        if init_u is None:
            u = np.zeros((N, Fp), dtype=np.float32)
            u[:, :self.F] = np.random.default_rng(seed).random((self.F, N)).T       # drawn [F, N] like the reference
            init_u = torch.from_numpy(u).to(self.device)
        H._chk(init_u, 'init_u')
        st = H._stream()
        proj = torch.empty(N, 2 * Fp, device=self.device)
        tprev = torch.empty(N, 2 * Fp, device=self.device)
        _lib.call('ft_gl_init', init_u.data_ptr(), S.data_ptr(), proj.data_ptr(), N, Fp, st)
        alpha = self.momentum / (1.0 + self.momentum)
        for it in range(n_iter):
            ypad = self.istft_padded(proj)
            rebuilt = self.stft_of_padded(ypad, N)
            _lib.call('ft_gl_phase', rebuilt.data_ptr(), tprev.data_ptr(), S.data_ptr(), proj.data_ptr(), N, Fp, alpha,
                      int(it > 0), st)
        ypad = self.istft_padded(proj)
        pad = self.n_fft // 2
        return ypad[pad:ypad.numel() - pad].clone()

    def griffinlim(self, mel: Union[torch.Tensor, np.ndarray], n_iter: int = 32, seed: Optional[int] = None,
                   init_u: Optional[torch.Tensor] = None) -> torch.Tensor:
        """DSP.griffinlim (utils/dsp.py:80-94): log-mel [n_mels, T] -> wav (device tensor, hop*(T-1) samples)"""
        if isinstance(mel, np.ndarray):
            mel = torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32))
        mel = mel.to(self.device, torch.float32).contiguous()
        if mel.dim() == 3 and mel.shape[0] == 1:
            mel = mel[0]
        return self.griffinlim_from_stft(self.mel_to_stft(mel), n_iter, init_u, seed)

    # ---- ragged batch --------------------------------------------------------------------------------
    def _batch_lens(self, what: str, mel_len: torch.Tensor, B: int, Tmax: int):
        """-> (mel_len on the device, error flag or None, the message of a raised flag): ragged.device_lens for
        1 <= mel_len[b] <= Tmax"""
        if self.n_fft % 8:
            raise _lib.FtError('griffinlim_batch: n_fft must be a multiple of 8')
        if not isinstance(mel_len, torch.Tensor):
            raise _lib.FtError(f'{what}: mel_len must be an int64 tensor')
        if B < 1 or Tmax < 1:
            raise _lib.FtError(f'{what}: an empty batch')
        return ragged.device_lens(mel_len, B, 1, Tmax, what, 'mel_len', 'Tmax', self.device) \
            + (ragged.range_message(what, 'mel_len', 1, Tmax, 'Tmax'),)

    def _mel_to_stft_batch(self, mel: torch.Tensor, ml: torch.Tensor, err: Optional[torch.Tensor]) -> torch.Tensor:
        B, C, Tmax = mel.shape
        g = gl_batch_geometry(B, Tmax, self.n_fft, self.hop)
        rows, st = g['rows'], H._stream()
        M = H.gl_exp_transpose_ragged(mel, ml, g['Tcap'], err, alloc=_alloc)          # [rows, C], zero rows at n >= N_b
        X = H.gl_relu(H.linear_fwd_as(M, C, self.mel_pinv, rows, C, _alloc))         # clipped least squares [rows, Fp]
        for _ in range(self.nnls_iter):                                              # row-local: zero rows stay zero
            R = H.linear_fwd_as(X, self.Fp, self.mel_basis, rows, self.Fp, _alloc)        # [rows, n_mels]
            _lib.call('ft_sub', R.data_ptr(), M.data_ptr(), R.data_ptr(), R.numel(), st)
            G = H.linear_fwd_as(R, C, self.mel_basis_t, rows, C, _alloc)                  # [rows, Fp]
            _lib.call('ft_nnls_step', X.data_ptr(), G.data_ptr(), self.inv_lip, X.numel(), st)
        return X

    def _check_mel_batch(self, what: str, mel: torch.Tensor) -> torch.Tensor:
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3:
            raise _lib.FtError(f'{what}: mel must be a [B, n_mels, Tmax] tensor')
        if mel.dtype != torch.float32:
            raise _lib.FtError(f'{what}: mel must be float32, got {mel.dtype}')
        if mel.shape[1] != self.n_mels:
            raise _lib.FtError(f'{what}: expected {self.n_mels} mel channels, got {mel.shape[1]}')
        return mel.to(self.device).contiguous()

    def mel_to_stft_batch(self, mel: torch.Tensor, mel_len: torch.Tensor) -> torch.Tensor:
        """log-mel [B, n_mels, Tmax], mel_len int64 [B] -> magnitudes packed [B * Tcap, Fp] (item b's frame n at row
        b * Tcap + n, Tcap from gl_batch_geometry); the rows n >= mel_len[b] of an item are all zero"""
        mel = self._check_mel_batch('mel_to_stft_batch', mel)
        ml, err, msg = self._batch_lens('mel_to_stft_batch', mel_len, mel.shape[0], mel.shape[2])
        X = self._mel_to_stft_batch(mel, ml, err)
        self._len_flag.check(err, msg)
        return X

    def _gl_from_stft_batch(self, S, ml, B, Tmax, n_iter, init_u, seed, err) -> Dict[str, torch.Tensor]:
        g = gl_batch_geometry(B, Tmax, self.n_fft, self.hop)
        Tcap, rows, Fp = g['Tcap'], g['rows'], self.Fp
        H._chk(S, 'S')
        if tuple(S.shape) != (rows, Fp):
            raise _lib.FtError(f'griffinlim_from_stft_batch: expected S [B * Tcap = {rows}, Fp = {Fp}], got {tuple(S.shape)}')
        if init_u is None and seed is None:
            seed = int.from_bytes(os.urandom(8), 'little')
        proj = H.gl_init_ragged(S, ml, B, Tcap, Tmax, u=init_u, seed=seed or 0, err=err, alloc=_alloc)
        tprev = _alloc(rows, 2 * Fp, device=self.device)
        alpha = self.momentum / (1.0 + self.momentum)
        ola = lambda fr, as_wav: H.overlap_add_ragged(fr, self.w2, ml, B, Tcap, Tmax, self.n_fft, self.hop, as_wav, alloc=_alloc)
        for it in range(n_iter):
            frames = H.linear_fwd_as(proj, 2 * Fp, self.w_inv, rows, 2 * Fp, _alloc)        # inverse STFT of every item
            ypad = ola(frames, False)
            rebuilt = H.linear_fwd_as(ypad, self.hop, self.w_fwd, rows, self.n_fft, _alloc)     # in place, ldx = hop
            H.gl_phase_ragged(rebuilt, tprev, S, ml, proj, B, Tcap, Tmax, alpha, it > 0)
        wav = ola(H.linear_fwd_as(proj, 2 * Fp, self.w_inv, rows, 2 * Fp, _alloc), True)
        return {'wav': wav, 'wav_len': (ml - 1) * self.hop}

    def griffinlim_from_stft_batch(self, S: torch.Tensor, mel_len: torch.Tensor, Tmax: int, n_iter: int = 32,
                                   init_u: Optional[torch.Tensor] = None, seed: Optional[int] = None
                                   ) -> Dict[str, torch.Tensor]:
        """S packed [B * Tcap, Fp] (mel_to_stft_batch's layout for this Tmax) -> {'wav' [B, hop * (Tmax - 1)], zero at
        j >= wav_len[b]; 'wav_len' int64 [B] = hop * (mel_len - 1)}.  init_u [B * Tcap, Fp] in [0, 1): the initial phases
        / (2 pi) in the same layout (rows n >= mel_len[b] are ignored); without it they are drawn on the device from
        (seed, frame, bin) -- see griffinlim_batch."""
        B = int(mel_len.numel()) if isinstance(mel_len, torch.Tensor) else 0
        ml, err, msg = self._batch_lens('griffinlim_from_stft_batch', mel_len, B, int(Tmax))
        out = self._gl_from_stft_batch(S, ml, B, int(Tmax), n_iter, init_u, seed, err)
        self._len_flag.check(err, msg)
        return out

    def griffinlim_batch(self, mel: torch.Tensor, mel_len: torch.Tensor, n_iter: int = 32, seed: Optional[int] = None,
                         init_u: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """griffinlim() of a RAGGED batch of mels (generate_batch's 'mel_post' and 'mel_len'): item b of the result is
        what griffinlim gives mel[b, :, :mel_len[b]] alone, to fp32 rounding, given the same initial phases.

        mel: float32 [B, n_mels, Tmax] on the device; entries at t >= mel_len[b] are ignored, whatever they hold
        (padding_value, NaN, Inf).  mel_len: int64 [B], on the host or the device, 1 <= mel_len[b] <= Tmax.
        -> {'wav': float32 [B, hop * (Tmax - 1)], zero at j >= wav_len[b]; 'wav_len': int64 [B] = hop * (mel_len - 1)}.

        Two guarantees are exact.  (1) With the same `seed` or `init_u`, an item's wav_len[b] samples are bit-identical
        whether it is passed alone (B = 1, Tmax = its own length) or inside any batch, at any position: every GEMM runs
        on one fixed kernel and every other step is per frame, bin or sample.  (2) A NaN or Inf item, or NaN in the
        padding of mel, changes no other item's bits.  The phases of `seed` are drawn on the device by a counter-based
        generator keyed on (seed, frame, bin) (include/fwdtaco_hip.h: ft_gl_init_ragged); they deliberately differ from
        the numpy draw of griffinlim(seed=...).  seed=None takes a fresh seed from the operating system.  Seeds whose
        draws are meant to be independent must differ in the high 32-bit word, and not only in its top ten bits: two
        seeds with equal high words -- seed=1 and seed=2 -- give the same phases permuted by an XOR of the index
        (csrc/ft_common.h: the seed contract of ft_hash32).

        The lengths follow the contract of ragged.py: a host-side mel_len is checked up front and nothing synchronises;
        a device-side one is clamped inside the kernels and its FtError is raised at the end of the call, after one
        synchronisation, through ONE pinned host word kept on this object -- so one GriffinLim must not run the batched
        calls with a device-side mel_len from two threads or on two streams at once."""
        mel = self._check_mel_batch('griffinlim_batch', mel)
        B, _, Tmax = mel.shape
        ml, err, msg = self._batch_lens('griffinlim_batch', mel_len, B, Tmax)
        S = self._mel_to_stft_batch(mel, ml, err)
        out = self._gl_from_stft_batch(S, ml, B, Tmax, n_iter, init_u, seed, err)
        self._len_flag.check(err, msg)
        return out


def spectral_convergence(gl: GriffinLim, wav: torch.Tensor, S: torch.Tensor) -> float:
    """|| |STFT(wav)| - S ||_F / ||S||_F on the device (diagnostic)"""
    X = gl.stft(wav)
    N = min(X.shape[0], S.shape[0])
    mag = torch.sqrt(X[:N, :gl.Fp] ** 2 + X[:N, gl.Fp:] ** 2)
    return float(torch.linalg.norm(mag - S[:N]) / torch.linalg.norm(S[:N]).clamp_min(1e-30))


__all__ = ['GriffinLim', 'gl_batch_geometry', 'slaney_mel_basis', 'spectral_convergence', 'window_sumsquare_f32']
