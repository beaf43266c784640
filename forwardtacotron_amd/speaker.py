"""Speaker embeddings on the MI355X: VoiceEncoder.embed_batch for a ragged batch of wavs.

Reference: preprocess.py:80 (`self.voice_encoder = VoiceEncoder()`), :173-182 (speaker_emb/{id}.npy per file) and :218-227
(mean_speaker_emb/{speaker}.npy per speaker), which use resemblyzer's VoiceEncoder.

    enc = VoiceEncoder.from_checkpoint('pretrained.pt').to('cuda')          # or VoiceEncoder().to('cuda')
    emb = enc.embed_utterance(y)                                            # [256]; numpy in -> numpy out, device in -> device out
    res = enc.embed_batch(wavs, source_sr=48000)                            # {'embed' [B, 256], 'n_partials' [B]}
    write_speaker_embs(res, item_ids, paths.speaker_emb)
    names, means = enc.mean_speaker_embs(res['embed'], speakers)            # ({speaker: row}, [S, 256])
    write_mean_speaker_embs(names, means, paths.mean_speaker_emb)

The algorithm is resemblyzer's published one, written out as a definition in DESIGN.md section 7 ("Speaker embedding"):
increase-only volume normalisation to -30 dBFS, partial utterances of 160 frames every 77, a 40-channel POWER mel (25 ms
periodic Hann window, 10 ms hop, centred with zero padding, Slaney basis, no log), nn.LSTM(40, 256, 3) from zero states,
relu(linear(h_last)), 2-norm per partial, mean of the partials, 2-norm.  The module is constructible anywhere; the embed_*
methods run on a HIP device only and raise FtError for CPU parameters or CPU tensors (numpy arrays are host data and are
copied in, as everywhere in the audio path).

One call is ft_spk_gain, ft_spk_pack, the DFT of every frame of every item as ONE GEMM over the packed buffer read with
a row stride of hop (hip.linear_fwd_as, whose rounding does not depend on the batch), ft_spk_mel_power, then per chunk of
at most PARTIAL_CHUNK partials: ft_spk_gather_partials, three times (input-projection GEMM, ft_lstm_fwd_uni at H = 256),
the embedding GEMM with its ReLU; and at the end one ft_spk_segment_mean_norm.  With `source_sr` the package's polyphase
resampler runs first (audio.resample_ragged: one more launch).  Semantics of the kernels: include/fwdtaco_hip.h; the
float64 restatement the tests compare against: tests/voice_encoder_cpu.py.

Lengths follow ragged.py's contract.  With lengths on the host (a list of wavs, or wav_len as a host array) the table of
partials is computed exactly on the host, an item of length 0 raises up front, and nothing synchronises.  With wav_len on
the device nothing is sized from it: EVERY item gets the slot count of the padded length L, the kernels derive each
item's own count from its length on the device, unused slots carry zero input and are skipped by the reduction -- so a
device-side wav_len costs recurrence rows (B * slots(L) instead of the sum of the items' own counts) -- and a length
outside [1, L] is reported after ONE synchronisation at the end of the call through ONE pinned host word kept on this
object (so one VoiceEncoder must not run embed_batch with a device-side wav_len from two threads or two streams at once).

PARITY UNPINNED against the reference: resemblyzer, webrtcvad and librosa are not installed here and there is no
pretrained.pt.  What is pinned is the written definition, in float64.  Loading the published checkpoint is untested:
from_checkpoint is tested against a synthetic file of the same layout ({'model_state': {lstm.*, linear.*,
similarity_weight, similarity_bias}}).  Deliberate differences: an all-zero wav gets gain 1 (resemblyzer divides by zero
and returns NaN); the STFT's padding is zeros (librosa >= 0.10's default; older versions reflect).

Not provided: trim_long_silences (webrtcvad), exactly as in audio.DSP: embed_batch(..., trim_long_silences=True) raises
FtError.  Training the encoder (the GE2E loss, the similarity parameters) is out of scope.
"""
import os
from fractions import Fraction
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from . import hip as H
from . import ragged
from .audio import resample_intake, resample_len, resample_ragged, resample_ratio, sparse_mel_basis
from .vocoder import slaney_mel_basis

Wav = Union[np.ndarray, torch.Tensor]

# partials per pass through the LSTM stack: the time-major projection buffer is partials_n_frames * 4 H * 4 bytes = 655 KB
# per partial, 168 MB at 256 -- the bound is one of memory
PARTIAL_CHUNK = 256
COVERAGE_MAX_DEN = 1 << 20                  # min_coverage is compared in integers as the nearest fraction below this


def _empty(*shape, dtype=torch.float32, device=None) -> torch.Tensor:
    """every device buffer of this module is allocated here (tests replace it with a poison-filling allocator)"""
    return torch.empty(*shape, dtype=dtype, device=device)


def _alloc(*shape, **kw) -> torch.Tensor:
    return _empty(*shape, **kw)               # looked up at call time, so a replaced _empty takes effect


def coverage_fraction(min_coverage: float) -> Tuple[int, int]:
    """min_coverage as the integers (num, den) the comparison uses, den <= 2^20 (0.75 -> (3, 4))"""
    if not 0 <= min_coverage <= 1:
        raise _lib.FtError(f'VoiceEncoder: min_coverage must be in [0, 1], got {min_coverage!r}')
    f = Fraction(min_coverage).limit_denominator(COVERAGE_MAX_DEN)
    return f.numerator, f.denominator


def frame_step_of(sampling_rate: int, hop: int, rate: float) -> int:
    """int(round((sampling_rate / rate) / hop)): 77 at 16 kHz, 10 ms, 1.3 partials per second"""
    if not rate > 0:
        raise _lib.FtError(f'VoiceEncoder: rate must be positive, got {rate!r}')
    step = int(round((sampling_rate / rate) / hop))
    if step < 1:
        raise _lib.FtError(f'VoiceEncoder: rate {rate!r} gives a frame step of {step}')
    return step


def partial_count(n: int, hop: int, partials_n_frames: int, frame_step: int, cov: Tuple[int, int]) -> int:
    """the number of partials of an n-sample wav: one slice [i, i + partials_n_frames) per i in range(0, steps,
    frame_step), steps = max(1, ceil((n + 1) / hop) - partials_n_frames + frame_step + 1); the last is dropped if it is
    not the only one and covers less than min_coverage of its span (in integers).  Pure host arithmetic."""
    n_frames = (n + hop) // hop
    steps = max(1, n_frames - partials_n_frames + frame_step + 1)
    k = -(-steps // frame_step)
    start = (k - 1) * frame_step * hop
    if k > 1 and (n - start) * cov[1] < cov[0] * partials_n_frames * hop:
        k -= 1
    return k


def compute_partial_slices(n_samples: int, rate: float = 1.3, min_coverage: float = 0.75, sampling_rate: int = 16000,
                           hop: int = 160, partials_n_frames: int = 160) -> Tuple[List[slice], List[slice]]:
    """resemblyzer's VoiceEncoder.compute_partial_slices: (wav slices, mel slices) of an n_samples wav"""
    step = frame_step_of(sampling_rate, hop, rate)
    k = partial_count(int(n_samples), hop, partials_n_frames, step, coverage_fraction(min_coverage))
    mel = [slice(i * step, i * step + partials_n_frames) for i in range(k)]
    return [slice(s.start * hop, s.stop * hop) for s in mel], mel


class VoiceEncoder(nn.Module):
    """resemblyzer's VoiceEncoder (its state_dict layout: lstm.weight_ih_l0 .. lstm.bias_hh_l2, linear.weight,
    linear.bias) with embed_utterance on HIP kernels, plus embed_batch for a ragged batch.  `lstm` is a parameter
    container: its forward is never called."""

    def __init__(self, sampling_rate: int = 16000, mel_window_length: int = 25, mel_window_step: int = 10,
                 mel_n_channels: int = 40, partials_n_frames: int = 160, audio_norm_target_dBFS: float = -30,
                 model_hidden_size: int = 256, model_embedding_size: int = 256, model_num_layers: int = 3) -> None:
        super().__init__()
        self.sampling_rate = int(sampling_rate)
        self.n_fft = self.sampling_rate * mel_window_length // 1000
        self.hop = self.sampling_rate * mel_window_step // 1000
        self.n_mels, self.partials_n_frames = int(mel_n_channels), int(partials_n_frames)
        self.target_dBFS = float(audio_norm_target_dBFS)
        self.hidden, self.embedding, self.num_layers = int(model_hidden_size), int(model_embedding_size), int(model_num_layers)
        if self.n_fft < 8 or self.n_fft % 8 or self.hop < 4 or self.hop % 4 or self.hop > self.n_fft:
            raise _lib.FtError(f'VoiceEncoder: the window ({self.n_fft} samples) must be a multiple of 8 and the hop '
                               f'({self.hop}) a multiple of 4 that is no longer')
        if self.hidden % 16 or not 1 <= self.embedding <= 1024 or self.num_layers < 1 or self.partials_n_frames < 2:
            raise _lib.FtError('VoiceEncoder: model_hidden_size must be a multiple of 16, model_embedding_size in 1..1024, '
                               'partials_n_frames at least 2')
        self.lstm = nn.LSTM(self.n_mels, self.hidden, self.num_layers, batch_first=True)
        self.linear = nn.Linear(self.hidden, self.embedding)
        self._tabs: Dict[Any, Any] = {}                        # per device: DFT matrix and sparse mel basis
        self._rs_tabs: Dict[Tuple[int, int], Any] = {}         # resampling coefficient tables per (up, down)
        self._len_flag = ragged.LenFlag()                      # the pinned word a device-side length check reports through

    # ------------------------------------------------------------------------------------------------
    @classmethod
    def from_checkpoint(cls, path: Union[str, os.PathLike], **kw) -> 'VoiceEncoder':
        """resemblyzer's pretrained.pt: torch.load(path)['model_state'] (which also carries similarity_weight and
        similarity_bias, the GE2E loss's: ignored) or a bare state dict.  Every lstm.* / linear.* entry must be there."""
        ck = torch.load(path, map_location='cpu')
        state = ck['model_state'] if isinstance(ck, dict) and 'model_state' in ck else ck
        enc = cls(**kw)
        missing, _ = enc.load_state_dict(state, strict=False)
        if missing:
            raise _lib.FtError(f'VoiceEncoder.from_checkpoint: {path} lacks {sorted(missing)}')
        return enc

    def forward(self, *a, **kw):
        raise _lib.FtError('VoiceEncoder: use embed_utterance / embed_batch (training the encoder is not provided)')

    # ------------------------------------------------------------------------------------------------
    def dft_matrix(self) -> np.ndarray:
        """float64 [2 Fp, n_fft]: rows 0 .. F-1 = window * cos, rows Fp .. Fp+F-1 = -window * sin (periodic Hann)"""
        n_fft, F = self.n_fft, self.n_fft // 2 + 1
        Fp = (F + 3) // 4 * 4
        k = np.arange(n_fft)
        win = 0.5 - 0.5 * np.cos(2 * np.pi * k / n_fft)
        ang = 2 * np.pi * np.outer(np.arange(F), k) / n_fft
        fwd = np.zeros((2 * Fp, n_fft))
        fwd[:F] = np.cos(ang) * win
        fwd[Fp:Fp + F] = -np.sin(ang) * win
        return fwd

    def mel_basis(self) -> np.ndarray:
        return slaney_mel_basis(self.sampling_rate, self.n_fft, self.n_mels, 0, self.sampling_rate / 2)

    def _device(self) -> torch.device:
        dev = self.linear.weight.device
        if dev.type != 'cuda' or any(p.device != dev or p.dtype != torch.float32 for p in self.parameters()):
            raise _lib.FtError('VoiceEncoder runs on an MI355X (HIP) device only, in float32; there is no CPU fallback: '
                               "move it with .to('cuda')")
        return dev

    def _tables(self, dev: torch.device):
        ent = self._tabs.get(dev)
        if ent is None:
            w, meta = sparse_mel_basis(self.mel_basis())
            f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
            ent = self._tabs[dev] = (f32(self.dft_matrix()), f32(w), torch.from_numpy(meta).to(dev))
        return ent

    def _intake(self, wavs, wav_len, source_sr, rate: float, min_coverage: float, trim_long_silences: bool):
        """every check, then the intake (and the resampling) -> the batch at self.sampling_rate and its geometry"""
        if trim_long_silences:
            raise _lib.FtError('VoiceEncoder: trim_long_silences (webrtcvad) is not provided')
        dev = self._device()
        what = 'embed_batch'
        step = frame_step_of(self.sampling_rate, self.hop, rate)
        cov = coverage_fraction(min_coverage)
        ratio = None
        if source_sr is not None:
            up, down = resample_ratio(source_sr, self.sampling_rate)
            ratio = None if up == down else (up, down)
        tensors = list(wavs) if isinstance(wavs, (list, tuple)) else [wavs]
        if any(isinstance(y, torch.Tensor) and not y.is_cuda for y in tensors):
            raise _lib.FtError(f'{what}: tensors must be on the HIP device (numpy arrays are copied in)')
        host_lens: Optional[List[int]] = None
        if wav_len is None:
            if isinstance(wavs, (list, tuple)) and all(getattr(y, 'ndim', None) == 1 for y in wavs):
                host_lens = [int(y.shape[0]) for y in wavs]
        elif not (isinstance(wav_len, torch.Tensor) and wav_len.is_cuda):
            host_lens = [int(v) for v in np.asarray(wav_len).reshape(-1)]
        if host_lens is not None and len(host_lens) and min(host_lens) < 1:
            raise _lib.FtError(f'{what}: every wav needs at least one sample (lengths {host_lens})')
        wav, lens, L, err = resample_intake(wavs, wav_len, dev, what)
        if ratio is not None:
            rs = resample_ragged(self._rs_tabs, wav, lens, L, ratio[0], ratio[1], err)
            wav, lens, L = rs['wav'], rs['wav_len'], resample_len(L, source_sr, self.sampling_rate)
            if host_lens is not None:
                host_lens = [resample_len(n, source_sr, self.sampling_rate) for n in host_lens]
        if host_lens is None and err is None:           # lengths on the device always report through the flag
            err = torch.zeros(1, dtype=torch.int32, device=dev)
        return dev, wav, lens, L, err, host_lens, step, cov

    def _slot_table(self, B: int, L: int, host_lens: Optional[List[int]], step: int, cov: Tuple[int, int], dev):
        """-> (table int32 [P, 2] = (item, first frame), offsets int64 [B + 1], both on the device; the host's counts;
        rows_per_item).  Host lengths: each item's own partials.  Device lengths: the slot count of L for every item."""
        pf, hop = self.partials_n_frames, self.hop
        counts = [partial_count(n, hop, pf, step, cov) for n in host_lens] if host_lens is not None else \
            [partial_count(L, hop, pf, step, cov)] * B
        kmax = partial_count(max(host_lens) if host_lens is not None else L, hop, pf, step, cov)
        rows_per_item = (kmax - 1) * step + pf + -(-self.n_fft // hop)      # stride = rows * hop covers the last frame read
        tab = np.array([(b, s * step) for b, k in enumerate(counts) for s in range(k)], dtype=np.int32).reshape(-1, 2)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        to_dev = lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)
        return to_dev(tab), to_dev(off), counts, rows_per_item

    def stages(self, wavs, wav_len: Optional[Wav] = None, source_sr: Optional[int] = None, rate: float = 1.3,
               min_coverage: float = 0.75, normalize_volume: bool = True, trim_long_silences: bool = False,
               keep: bool = True) -> Dict[str, Any]:
        """embed_batch with every intermediate, for the tests: gain [B], n_partials, frames [B] (from the device), mel
        [B, rows_per_item, n_mels] (power mel, frame-major, zero at t >= frames[b]), table [P, 2], offsets [B + 1],
        host_counts (the host's partial counts; with a device-side wav_len the slot count of L per item), partials
        (the gathered input of every chunk), h_last [P, H], raw [P, E] (relu(linear)), partial_embeds [P, E], embed.
        keep=False (embed_batch) drops `partials` and `h_last`, which would hold every chunk's buffers until the end."""
        dev, wav, lens, L, err, host_lens, step, cov = self._intake(wavs, wav_len, source_sr, rate, min_coverage,
                                                                    trim_long_silences)
        B = wav.shape[0]
        pf, hop, n_fft, Hd, E = self.partials_n_frames, self.hop, self.n_fft, self.hidden, self.embedding
        w_fwd, mel_w, mel_meta = self._tables(dev)
        Fp = w_fwd.shape[0] // 2
        table, offsets, counts, rows = self._slot_table(B, L, host_lens, step, cov, dev)
        P = table.shape[0]
        gain, n_partials, frames = H.spk_gain(wav, lens, L, 10.0 ** (self.target_dBFS / 20.0), hop, pf, step, cov[0],
                                              cov[1], normalize_volume, err, alloc=_alloc)
        packed = H.spk_pack(wav, lens, L, gain, rows * hop, n_fft, alloc=_alloc)
        spec = H.linear_fwd_as(packed, hop, w_fwd, B * rows, n_fft, alloc=_alloc)         # frames read in place
        mel = H.spk_mel_power(spec, Fp, rows, frames, mel_w, mel_meta, self.n_mels, B, alloc=_alloc)
        raw = _alloc(P, E, device=dev)
        gathered, h_last = [], []
        for p0 in range(0, P, max(1, int(PARTIAL_CHUNK))):
            Pc = min(max(1, int(PARTIAL_CHUNK)), P - p0)
            x = H.spk_gather_partials(mel, rows, frames, table, p0, Pc, pf, B, alloc=_alloc)        # [pf, Pc, n_mels]
            if keep:
                gathered.append(x)
            for layer in range(self.num_layers):
                w_ih, w_hh, b_ih, b_hh = (getattr(self.lstm, f'{n}_l{layer}') for n in
                                          ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
                xp = H.linear_fwd(x, w_ih, b_ih)                                              # [pf, Pc, 4 H], time-major
                x, _ = H.lstm_fwd_uni(xp, w_hh, b_hh, Hd, alloc=_alloc)
            if keep:
                h_last.append(x[pf - 1])
            H.linear_fwd(x[pf - 1], self.linear.weight, self.linear.bias, relu=True, out=raw[p0:p0 + Pc])
        partial_embeds = _alloc(P, E, device=dev)
        if host_lens is None:
            partial_embeds.zero_()                      # unused slots stay zero
        embed = H.spk_segment_mean_norm(raw, None, offsets, n_partials, True, rows_out=partial_embeds, alloc=_alloc)
        out = {'gain': gain, 'n_partials': n_partials, 'frames': frames, 'mel': mel.view(B, rows, self.n_mels),
               'table': table, 'offsets': offsets, 'host_counts': counts, 'partials': gathered,
               'h_last': torch.cat(h_last) if len(h_last) > 1 else (h_last[0] if h_last else None),
               'raw': raw, 'partial_embeds': partial_embeds, 'partial_item': table[:, 0].to(torch.int64), 'embed': embed,
               'wav': wav, 'wav_len': lens}
        self._len_flag.check(err, ragged.range_message('embed_batch', 'wav_len', 1, L, 'L'))
        return out

    def embed_batch(self, wavs, wav_len: Optional[Wav] = None, source_sr: Optional[int] = None, rate: float = 1.3,
                    min_coverage: float = 0.75, normalize_volume: bool = True, return_partials: bool = False,
                    trim_long_silences: bool = False) -> Dict[str, torch.Tensor]:
        """Speaker embeddings of a ragged batch.  wavs: a list of 1-D numpy arrays or device tensors, or a padded float32
        [B, L] batch with wav_len int64 [B] on the host or the device; at self.sampling_rate, or at source_sr (then
        resampled first by the package's polyphase resampler).
        -> {'embed': float32 [B, E], unit rows; 'n_partials': int64 [B]} on the device, and with return_partials
        'partial_embeds' float32 [P, E] (unit rows, item after item, ascending) and 'partial_item' int64 [P].  With a
        device-side wav_len P = B * slots(L) and the rows of unused slots (s >= n_partials[b]) are zero.

        An item's embedding does not depend on what sits beyond the lengths or in other items (NaN, Inf): inside one
        batch geometry it is bit-identical; alone against inside a batch it agrees to the recurrence kernels' rounding.
        No epsilon anywhere: a partial whose ReLU output is all zero has norm 0 and makes its utterance NaN."""
        st = self.stages(wavs, wav_len, source_sr, rate, min_coverage, normalize_volume, trim_long_silences, keep=False)
        out = {'embed': st['embed'], 'n_partials': st['n_partials']}
        if return_partials:
            out['partial_embeds'], out['partial_item'] = st['partial_embeds'], st['partial_item']
        return out

    def embed_utterance(self, wav: Wav, return_partials: bool = False, rate: float = 1.3, min_coverage: float = 0.75):
        """resemblyzer's embed_utterance: one 1-D wav at self.sampling_rate -> its embedding [E], or with return_partials
        (embed, partial_embeds [n, E], wav slices); numpy in -> numpy out, device tensor in -> device tensor out.  It is
        embed_batch([wav]), item 0."""
        if getattr(wav, 'ndim', None) != 1:
            raise _lib.FtError('VoiceEncoder: expected a 1-D wav')
        out = self.embed_batch([wav], rate=rate, min_coverage=min_coverage, return_partials=return_partials)
        conv = (lambda t: t.cpu().numpy()) if isinstance(wav, np.ndarray) else (lambda t: t)
        if not return_partials:
            return conv(out['embed'][0])
        slices = compute_partial_slices(int(wav.shape[0]), rate, min_coverage, self.sampling_rate, self.hop,
                                        self.partials_n_frames)[0]
        return conv(out['embed'][0]), conv(out['partial_embeds']), slices

    def mean_speaker_embs(self, embed: torch.Tensor, speakers: Sequence[str]) -> Tuple[Dict[str, int], torch.Tensor]:
        """preprocess.py:218-227: per speaker, the sum of its utterance embeddings / their number / the 2-norm (fp32, in
        ascending item order; the reference accumulates in float64 on the host).  embed [B, E] on the device, speakers:
        B names -> ({name: row}, float32 [S, E] on the device), rows in order of first appearance."""
        if not isinstance(embed, torch.Tensor) or not embed.is_cuda or embed.dim() != 2 or embed.dtype != torch.float32:
            raise _lib.FtError('mean_speaker_embs: embed must be a float32 [B, E] tensor on the HIP device')
        if len(speakers) != embed.shape[0] or embed.shape[0] == 0:
            raise _lib.FtError(f'mean_speaker_embs: {len(speakers)} speaker names for {embed.shape[0]} embeddings')
        names: Dict[str, int] = {}
        members: List[List[int]] = []
        for b, name in enumerate(speakers):
            if name not in names:
                names[name] = len(members)
                members.append([])
            members[names[name]].append(b)
        index = np.array([b for m in members for b in m], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int64)
        to_dev = lambda a: torch.from_numpy(a).pin_memory().to(embed.device, non_blocking=True)
        means = H.spk_segment_mean_norm(embed.contiguous(), to_dev(index), to_dev(off), None, False, alloc=_alloc)
        return names, means


def _save_rows(rows: np.ndarray, ids: Sequence, directory: Union[str, os.PathLike]) -> List[str]:
    os.makedirs(directory, exist_ok=True)
    paths = []
    for row, item_id in zip(rows, ids):
        path = os.path.join(directory, f'{item_id}.npy')
        np.save(path, np.ascontiguousarray(row, dtype=np.float32), allow_pickle=False)
        paths.append(path)
    return paths


def write_speaker_embs(result: Dict[str, torch.Tensor], item_ids: Sequence,
                       speaker_emb_dir: Union[str, os.PathLike]) -> List[str]:
    """embed_batch's result -> speaker_emb/{id}.npy per item: float32 [E] (preprocess.py:173-182).  Copies to the host:
    this is the synchronisation point.  Returns the paths."""
    embed = result['embed'].cpu().numpy()
    if len(item_ids) != embed.shape[0]:
        raise _lib.FtError(f'write_speaker_embs: {len(item_ids)} item ids for {embed.shape[0]} items')
    return _save_rows(embed, item_ids, speaker_emb_dir)


def write_mean_speaker_embs(names: Dict[str, int], means: torch.Tensor,
                            mean_speaker_emb_dir: Union[str, os.PathLike]) -> List[str]:
    """mean_speaker_embs' result -> mean_speaker_emb/{speaker}.npy per speaker: float32 [E] (preprocess.py:218-227)"""
    host = means.cpu().numpy()
    if sorted(names.values()) != list(range(host.shape[0])):
        raise _lib.FtError(f'write_mean_speaker_embs: {len(names)} names for {host.shape[0]} rows')
    order = sorted(names, key=names.get)
    return _save_rows(host, order, mean_speaker_emb_dir)


__all__ = ['PARTIAL_CHUNK', 'VoiceEncoder', 'compute_partial_slices', 'coverage_fraction', 'frame_step_of',
           'partial_count', 'write_mean_speaker_embs', 'write_speaker_embs']
