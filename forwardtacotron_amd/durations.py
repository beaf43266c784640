"""Per-token durations from Tacotron attentions on the device (duration_extraction/ of the reference).

reference                                                 here
duration_extraction/duration_extractor.py:11-84            DurationExtractor(...)(x, mel, attention), same outputs
  (scipy graph + Dijkstra per item, ~3.6 s at 800 x 150)    DurationExtractor.extract_batch: one ft_dur_extract launch
duration_extraction_pipe.py:56-62  attention_score, r=1    align_score of extract_batch
duration_extraction_pipe.py:137-183 extract_durations      extract_durations(model, batches, out_dir)

Semantics (include/fwdtaco_hip.h, ft_dur_extract): a frame is silent if its mean over the mel channels is below
`silence_threshold`; the attention of silent frames gets +shift on silent tokens (pad and punctuation) and -shift on the
others, is clamped to [0, 1], and the cost of a cell is 1 - att.  The cheapest monotonic path (right, down, diagonal;
an edge weighs the cost of the cell it enters) is found by a min-plus DP over the anti-diagonals in float64, whose
distances equal scipy's Dijkstra's bit for bit.  Each frame goes to the last token its row visits.

Where this deliberately differs from the reference:
  - ties: when two predecessors give exactly the same distance, the DP takes the diagonal, then the one above, then the
    one to the left.  Dijkstra's choice depends on heap order, so on items with several optimal paths the durations can
    differ while the cost is the same; on items with a single optimal path they are identical;
  - every frame silent: att_score is NaN (the reference raises ZeroDivisionError); the durations are still computed;
  - mel_len == x_len == 1: durations [1] (the reference fails with an IndexError);
  - the caller's attention tensor is not modified (the reference shifts it in place).
Kept from the reference: the shift is applied only when at least two frames are silent (with exactly one, the
reference's `nonzero().squeeze()` yields a 0-d tensor and it shifts nothing).
"""
import os
from dataclasses import dataclass
from typing import Dict, Iterable, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .hip import _chk, _p, _stream, workspace

# utils/text/symbols.py:21-26: the phoneme table starts with the pad '_' and the ten punctuation marks "!'(),.:;? "
SILENT_PHONEME_INDICES = tuple(range(11))

_STATUS = {1: 'x_len out of range (1 <= x_len <= the token / attention width, at most 1024)',
           2: 'mel_len out of range (1 <= mel_len <= the attention rows and the mel frames)',
           3: 'no workspace for the back-pointers'}


@dataclass
class DurationStats:
    """utils/dataset.py:20-25"""
    att_sharpness_score: float
    att_align_score: float
    max_consecutive_ones: int
    max_duration: int


@dataclass
class DurationBatch:
    """extract_batch's outputs, all on the device: durations [B, Tx] int64 (0 at j >= x_len); per item att_score
    (mean attention along the path over non-silent frames; NaN if every frame is silent), align_score (loc part of
    utils/metrics.py:attention_score, r = 1), cost (the path's summed cost, float64), max_duration and
    max_consecutive_ones (int64)."""
    durations: torch.Tensor
    att_score: torch.Tensor
    align_score: torch.Tensor
    cost: torch.Tensor
    max_duration: torch.Tensor
    max_consecutive_ones: torch.Tensor


class DurationExtractor:
    """duration_extraction/duration_extractor.py:11-22, computed by the ft_dur_extract kernel."""

    def __init__(self, silence_threshold: float, silence_prob_shift: float,
                 silent_phonemes_indices: Iterable[int] = SILENT_PHONEME_INDICES) -> None:
        self.silence_threshold = silence_threshold
        self.silence_prob_shift = silence_prob_shift
        self.silent_phonemes_indices = tuple(int(i) for i in silent_phonemes_indices)
        self._sil_ids = {}

    def _sil_table(self, device) -> torch.Tensor:
        t = self._sil_ids.get(device)
        if t is None:
            t = torch.tensor(self.silent_phonemes_indices or (-1,), dtype=torch.int64, device=device)
            self._sil_ids[device] = t
        return t

    def extract_batch(self, attn: torch.Tensor, x: torch.Tensor, x_len: torch.Tensor, mel: torch.Tensor,
                      mel_len: torch.Tensor, check: bool = True) -> DurationBatch:
        """attn [B, Tm, Tx] fp32 (Tacotron's attn_scores at r = 1), x [B, Tx_x] int64 tokens, mel [B, n_mels, Tmel],
        x_len / mel_len [B] int64 (host or device); item b uses attn[b, :mel_len, :x_len].  One launch for the
        batch.  check=True synchronises and raises FtError if any item's lengths are out of range (such an item gets
        zero durations and NaN scores)."""
        dev = attn.device
        _chk(attn, 'attn')
        _chk(mel, 'mel')
        _chk(x, 'x', torch.int64)
        if attn.dim() != 3 or mel.dim() != 3 or x.dim() != 2:
            raise _lib.FtError('extract_batch: expected attn [B,Tm,Tx], mel [B,n_mels,T], x [B,Tx]')
        B, Tm, Tx = attn.shape
        if mel.shape[0] != B or x.shape[0] != B:
            raise _lib.FtError('extract_batch: batch sizes differ')
        x_len = x_len.to(device=dev, dtype=torch.int64).contiguous()
        mel_len = mel_len.to(device=dev, dtype=torch.int64).contiguous()
        if x_len.shape != (B,) or mel_len.shape != (B,):
            raise _lib.FtError('extract_batch: x_len and mel_len must be [B]')
        Tx_out = x.shape[1]
        dur = torch.empty(B, Tx_out, dtype=torch.int64, device=dev)
        fstats = torch.empty(B, 3, dtype=torch.float64, device=dev)
        istats = torch.empty(B, 3, dtype=torch.int64, device=dev)
        if B > 0:
            sil = self._sil_table(dev)
            ws = workspace(_lib.query('ft_dur_workspace', B, Tm, Tx), dev)
            _lib.call('ft_dur_extract', _p(attn), Tm, Tx, _p(mel), mel.shape[1], mel.shape[2], _p(x), x.shape[1],
                      _p(x_len), _p(mel_len), _p(sil), len(self.silent_phonemes_indices),
                      float(self.silence_threshold), float(self.silence_prob_shift), B, _p(dur), Tx_out, _p(fstats),
                      _p(istats), _p(ws), _stream())
            if check:
                st = istats[:, 2].cpu()
                bad = [(b, int(s)) for b, s in enumerate(st.tolist()) if s != 0]
                if bad:
                    raise _lib.FtError('extract_batch: ' + '; '.join(f'item {b}: {_STATUS.get(s, s)}' for b, s in bad))
        return DurationBatch(durations=dur, att_score=fstats[:, 0], align_score=fstats[:, 1], cost=fstats[:, 2],
                             max_duration=istats[:, 0], max_consecutive_ones=istats[:, 1])

    def __call__(self, x: torch.Tensor, mel: torch.Tensor, attention: torch.Tensor) -> Tuple[torch.Tensor, float]:
        """duration_extractor.py:23-84: x [Tx] tokens, mel [n_mels, Tm], attention [Tm, Tx] -> (durations [Tx] float32
        on x's device, att_score).  Runs on the current HIP device whatever the inputs' device."""
        dev = attention.device if attention.is_cuda else torch.device('cuda', torch.cuda.current_device())
        Tm, Tx = attention.shape
        a = attention.to(device=dev, dtype=torch.float32).contiguous()[None]
        m = mel.to(device=dev, dtype=torch.float32).contiguous()[None]
        t = x.to(device=dev, dtype=torch.int64).contiguous()[None]
        res = self.extract_batch(a, t, torch.tensor([Tx]), m, torch.tensor([Tm]))
        return res.durations[0].to(device=x.device, dtype=torch.float32), float(res.att_score[0])


def extract_durations(model, batches: Iterable[Dict], out_dir: Union[str, os.PathLike],
                      extractor: Optional[DurationExtractor] = None,
                      save_attention: Optional[Union[str, os.PathLike]] = None) -> Dict[str, DurationStats]:
    """duration_extraction_pipe.py:extract_attentions + extract_durations in one pass over the batches, the attention
    staying on the device.  `model` is a Tacotron (r must be 1) with `align(batch) -> attn [B, steps, Tx]`; it is put
    in the extraction mode of train_tacotron.py:119-120 (eval, decoder prenet in train mode).  `batches` are
    datapath.TacoCollator batches, on the device (datapath.DevicePrefetcher) or on the host.  Writes
    <out_dir>/<item_id>.npy int64 durations [x_len] (what paths.alg holds) and, if `save_attention` names a directory,
    <save_attention>/<item_id>.npy attention [mel_len, x_len] (paths.att_pred).  `extractor` defaults to the
    singlespeaker config's settings (silence_threshold -11, silence_prob_shift 0.25).  Returns {item_id:
    DurationStats}."""
    if int(model.r) != 1:
        raise _lib.FtError(f'extract_durations: the model must run at r = 1 (got r = {int(model.r)})')
    extractor = extractor or DurationExtractor(silence_threshold=-11., silence_prob_shift=0.25)
    os.makedirs(out_dir, exist_ok=True)
    if save_attention:
        os.makedirs(save_attention, exist_ok=True)
    model.eval()
    model.decoder.prenet.train()
    stats = {}
    with torch.no_grad():
        for batch in batches:
            attn = model.align(batch)
            mel = batch['mel'].to(attn.device, non_blocking=True)
            x = batch['x'].to(attn.device, non_blocking=True)
            res = extractor.extract_batch(attn.contiguous(), x, batch['x_len'], mel.contiguous(), batch['mel_len'])
            write_durations(res, batch, attn, out_dir, save_attention, stats)
    return stats


def write_durations(res: DurationBatch, batch: Dict, attn: torch.Tensor, out_dir: Union[str, os.PathLike],
                    save_attention: Optional[Union[str, os.PathLike]], stats: Dict[str, DurationStats]) -> None:
    """extract_durations' output for one batch: <out_dir>/<item_id>.npy int64 durations [x_len], the attention
    [mel_len, x_len] under `save_attention` if given, and stats[item_id]"""
    dur = res.durations.cpu().numpy()
    att_score = res.att_score.cpu().numpy()
    align_score = res.align_score.cpu().numpy()
    max_dur = res.max_duration.cpu().numpy()
    max_ones = res.max_consecutive_ones.cpu().numpy()
    x_len = batch['x_len'].cpu().numpy()
    mel_len = batch['mel_len'].cpu().numpy()
    for b, item_id in enumerate(batch['item_id']):
        d = dur[b, :x_len[b]].astype(np.int64)
        np.save(os.path.join(out_dir, f'{item_id}.npy'), d, allow_pickle=False)
        if save_attention:
            np.save(os.path.join(save_attention, f'{item_id}.npy'),
                    attn[b, :mel_len[b], :x_len[b]].cpu().numpy(), allow_pickle=False)
        stats[item_id] = DurationStats(att_sharpness_score=float(att_score[b]),
                                       att_align_score=float(align_score[b]),
                                       max_consecutive_ones=int(max_ones[b]),
                                       max_duration=int(max_dur[b]))
