"""Per-token pitch and energy targets on the device: the last step of the reference's alignment stage.

reference                                                   here
train_tacotron.py:39-93   extract_pitch_energy               extract_pitch_energy(speaker_dict, train_dataset, ...)
  (per item: mel reloaded, Python loop per token, CPU)         batches of items, one ft_token_values launch each
train_tacotron.py:24-35   normalize_values                   normalize_pitch(values): ft_pitch_norm, on the device
train_tacotron.py:110-140 create_align_features              create_align_features(model, batches, ...): durations,
  (--force_align; --extract_pitch runs extract_pitch_energy)   pitch and energy in one pass over the teacher's batches

Semantics (include/fwdtaco_hip.h, ft_token_values / ft_pitch_norm):
  - the energy of frame t is ||exp(mel[:, t])||_2 over the channels of the stored log mel, fp32;
  - token j < min(mel_len, x_len) covers frames [cum_j, cum_j + dur_j); its pitch is the mean of the raw pitch there
    without zeros and values outside [pitch_min_freq, pitch_max_freq] (inclusive; a raw pitch shorter than the mel is
    cut off), its energy the mean of the frame energies; an empty segment gives 0, and so does every token from
    min(mel_len, x_len) on (the reference's zip(range(mel_len), ...));
  - an item whose durations do not sum to mel_len is skipped: no files, and it is not in the statistics;
  - only speakers whose name is longer than one character are processed;
  - the energy is written as it is; the pitch is normalised per speaker over the nonzero token pitches of its items:
    mean and population std, std = 1e10 unless std > 0, v = (v - mean) / std in fp32 where v != 0.
The speaker's values are gathered in item_id order, so batching and dataset order do not change a bit of the output.

Where this deliberately differs from the reference:
  - segment means are summed in fp64 and rounded once, and a speaker's mean and std are fp64 two-pass sums rounded to
    fp32 (numpy: fp32 pairwise sums); the exp is the device's.  Token values agree to a few fp32 ulps;
  - a speaker none of whose items survives gets no files and no statistics (the reference raises ValueError from
    np.concatenate of an empty list);
  - a missing input file raises, and so does a mel file with fewer frames than its dataset mel_len (the reference prints
    the exception and goes on without the item);
  - extract_pitch_energy returns {speaker: (mean, std)} for every processed speaker.  The reference returns the pair of
    whichever speaker its set iteration ends on, and no caller uses it.
"""
import os
import pickle
from dataclasses import dataclass
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .durations import DurationExtractor, DurationStats, write_durations
from .hip import _chk, _p, _stream, workspace

PathLike = Union[str, os.PathLike]

SKIPPED = 1                                  # ft_token_values status: the durations do not sum to mel_len
_STATUS = {2: 'x_len out of range (1 <= x_len <= the duration width, at most 2048)',
           3: 'mel_len out of range (1 <= mel_len <= the mel frames)',
           4: 'pitch_len out of range (0 <= pitch_len <= the pitch width)',
           5: 'a duration is negative',
           6: 'no workspace for the frame values'}


@dataclass
class TokenValuesBatch:
    """extract_batch's outputs, on the device: pitch / energy [B, Tx] fp32 (0 at j >= x_len and on skipped items),
    status [B] int32 (0 ok, SKIPPED: the durations do not sum to mel_len)."""
    pitch: torch.Tensor
    energy: torch.Tensor
    status: torch.Tensor


def _raise_bad(status: torch.Tensor, what: str) -> None:
    bad = [(b, s) for b, s in enumerate(status.cpu().tolist()) if s not in (0, SKIPPED)]
    if bad:
        raise _lib.FtError(f'{what}: ' + '; '.join(f'item {b}: {_STATUS.get(s, s)}' for b, s in bad))


class TokenValues:
    """train_tacotron.py:59-73 for a batch of items, computed by the ft_token_values kernel."""

    @staticmethod
    def extract_batch(mel: torch.Tensor, mel_len: torch.Tensor, pitch: torch.Tensor, pitch_len: torch.Tensor,
                      dur: torch.Tensor, x_len: torch.Tensor, fmin: float, fmax: float,
                      check: bool = True) -> TokenValuesBatch:
        """mel [B, n_mels, Tmel] fp32 (log mel), pitch [B, Tp] fp32 raw pitch (Tp >= 1), dur [B, Tx] int64, all on the
        device; mel_len / pitch_len / x_len [B] int64 (host or device).  Item b uses mel[b, :, :mel_len],
        pitch[b, :pitch_len], dur[b, :x_len].  One launch for the batch.  check=True synchronises and raises FtError
        if any item's inputs are out of range (such an item gets zeros); a skipped item is not an error."""
        dev = mel.device
        _chk(mel, 'mel')
        _chk(pitch, 'pitch')
        _chk(dur, 'dur', torch.int64)
        if mel.dim() != 3 or pitch.dim() != 2 or dur.dim() != 2:
            raise _lib.FtError('extract_batch: expected mel [B,n_mels,T], pitch [B,Tp], dur [B,Tx]')
        B = mel.shape[0]
        if pitch.shape[0] != B or dur.shape[0] != B:
            raise _lib.FtError('extract_batch: batch sizes differ')
        mel_len, pitch_len, x_len = (t.to(device=dev, dtype=torch.int64).contiguous()
                                     for t in (mel_len, pitch_len, x_len))
        if mel_len.shape != (B,) or pitch_len.shape != (B,) or x_len.shape != (B,):
            raise _lib.FtError('extract_batch: mel_len, pitch_len and x_len must be [B]')
        Tx = dur.shape[1]
        out_p = torch.empty(B, Tx, dtype=torch.float32, device=dev)
        out_e = torch.empty(B, Tx, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        if B > 0:
            nbytes = _lib.query('ft_token_values_workspace', B, mel.shape[2])
            ws = workspace(nbytes, dev) if nbytes else None
            _lib.call('ft_token_values', _p(mel), mel.shape[1], mel.shape[2], _p(mel_len), _p(pitch), pitch.shape[1],
                      _p(pitch_len), _p(dur), Tx, _p(x_len), float(fmin), float(fmax), B, _p(out_p), _p(out_e),
                      _p(status), _p(ws), _stream())
            if check:
                _raise_bad(status, 'extract_batch')
        return TokenValuesBatch(pitch=out_p, energy=out_e, status=status)


def normalize_pitch(values: torch.Tensor) -> Tuple[float, float]:
    """normalize_values (train_tacotron.py:24-35) over one speaker's token pitches, in place: `values` [n] fp32 on the
    device, in a fixed item order (the fp64 sums depend on it only in their last bits).  Returns (mean, std) as the
    fp32 values the normalisation used: mean NaN and std 1e10 when no value is nonzero."""
    _chk(values, 'values')
    n = values.numel()
    if n == 0:
        return float('nan'), 1e10
    dev = values.device
    stats = torch.empty(5, dtype=torch.float64, device=dev)
    ws = workspace(_lib.query('ft_pitch_norm_workspace', n), dev)
    _lib.call('ft_pitch_norm', _p(values), n, _p(stats), _p(ws), _stream())
    s = stats.cpu().numpy()
    return float(s[3]), float(s[4])


class _Pending:
    """per speaker, the device token pitches of its surviving items until every item has been seen"""

    def __init__(self, save_path_energy: PathLike) -> None:
        self.save_path_energy = save_path_energy
        self.items: Dict[str, List[Tuple[Any, torch.Tensor]]] = {}

    def add(self, res: TokenValuesBatch, item_ids: Sequence, speakers: Sequence[str], x_len: Sequence[int]) -> None:
        """writes the energies of the batch's surviving items of processed speakers and keeps their pitches"""
        status = res.status.cpu().numpy()
        energy = res.energy.cpu().numpy()
        for b, (item_id, spk) in enumerate(zip(item_ids, speakers)):
            if status[b] != 0 or len(spk) <= 1:
                continue
            xl = int(x_len[b])
            np.save(os.path.join(self.save_path_energy, f'{item_id}.npy'), energy[b, :xl], allow_pickle=False)
            self.items.setdefault(spk, []).append((item_id, res.pitch[b, :xl]))

    def finish(self, save_path_pitch: PathLike) -> Dict[str, Tuple[float, float]]:
        stats = {}
        for spk in sorted(self.items):
            entries = sorted(self.items[spk], key=lambda e: e[0])
            v = torch.cat([t for _, t in entries])
            stats[spk] = normalize_pitch(v)
            host = v.cpu().numpy()
            off = 0
            for item_id, t in entries:
                n = t.numel()
                np.save(os.path.join(save_path_pitch, f'{item_id}.npy'), host[off:off + n], allow_pickle=False)
                off += n
        self.items = {}
        return stats


def _padded(arrays: Sequence[np.ndarray], width: int, dtype) -> np.ndarray:
    out = np.zeros((len(arrays),) + arrays[0].shape[:-1] + (width,), dtype=dtype)
    for k, a in enumerate(arrays):
        out[k, ..., :a.shape[-1]] = a
    return out


def _raw_pitch(raw_pitch_dir: PathLike, item_ids: Sequence) -> Tuple[torch.Tensor, torch.Tensor]:
    """raw_pitch/<id>.npy -> padded [B, max(1, Tp)] fp32 and pitch_len [B] int64 (host)"""
    tracks = [np.asarray(np.load(os.path.join(raw_pitch_dir, f'{i}.npy')), dtype=np.float32).reshape(-1)
              for i in item_ids]
    width = max([1] + [len(t) for t in tracks])
    return torch.from_numpy(_padded(tracks, width, np.float32)), torch.tensor([len(t) for t in tracks])


def _unpickled(obj):
    if isinstance(obj, (str, os.PathLike)):
        with open(obj, 'rb') as f:
            return pickle.load(f)
    return obj


def extract_pitch_energy(speaker_dict, train_dataset, val_dataset, alg_dir: PathLike, mel_dir: PathLike,
                         raw_pitch_dir: PathLike, save_path_pitch: PathLike, save_path_energy: PathLike,
                         pitch_min_freq: float, pitch_max_freq: float, batch_size: int = 32,
                         device: Union[str, torch.device] = 'cuda') -> Dict[str, Tuple[float, float]]:
    """train_tacotron.py:39-93 (also what --extract_pitch runs).  `speaker_dict` ({item_id: speaker name}),
    `train_dataset` and `val_dataset` ([(item_id, mel_len)]) are the reference's pickles (paths.speaker_dict,
    paths.train_dataset, paths.val_dataset) or their unpickled contents; the directories are paths.alg, paths.mel,
    paths.raw_pitch, paths.phon_pitch and paths.phon_energy.  The items of the processed speakers run in item_id order,
    `batch_size` per ft_token_values launch; each speaker's token pitches stay on the device until all of them are
    known, are normalised there and written.  Writes <id>.npy float32 [x_len] per surviving item into both output
    directories.  Returns {speaker: (mean, std)} of every processed speaker (fp32 values; the reference returns only the
    last speaker's pair, which no caller reads)."""
    speaker_dict = _unpickled(speaker_dict)
    all_data = list(_unpickled(train_dataset)) + list(_unpickled(val_dataset))
    names = {v for v in speaker_dict.values() if len(v) > 1}
    items = sorted((item_id, int(mel_len)) for item_id, mel_len in all_data if speaker_dict[item_id] in names)
    os.makedirs(save_path_pitch, exist_ok=True)
    os.makedirs(save_path_energy, exist_ok=True)
    pending = _Pending(save_path_energy)
    with torch.no_grad():
        for s in range(0, len(items), batch_size):
            chunk = items[s:s + batch_size]
            ids = [i for i, _ in chunk]
            mel_len = [m for _, m in chunk]
            mels = [np.load(os.path.join(mel_dir, f'{i}.npy')) for i in ids]
            durs = [np.asarray(np.load(os.path.join(alg_dir, f'{i}.npy')), dtype=np.int64).reshape(-1) for i in ids]
            for i, m, a in zip(ids, mel_len, mels):
                if a.shape[-1] < m:
                    raise _lib.FtError(f'extract_pitch_energy: {i}: the mel has {a.shape[-1]} frames, the dataset '
                                       f'says mel_len {m}')
            x_len = [len(d) for d in durs]
            mel = torch.from_numpy(_padded(mels, max(a.shape[-1] for a in mels), np.float32)).to(device)
            dur = torch.from_numpy(_padded(durs, max([1] + x_len), np.int64)).to(device)
            pitch, pitch_len = _raw_pitch(raw_pitch_dir, ids)
            res = TokenValues.extract_batch(mel, torch.tensor(mel_len), pitch.to(device), pitch_len, dur,
                                            torch.tensor(x_len), pitch_min_freq, pitch_max_freq)
            pending.add(res, ids, [speaker_dict[i] for i in ids], x_len)
        return pending.finish(save_path_pitch)


def create_align_features(model, batches: Iterable[Dict], alg_dir: PathLike, raw_pitch_dir: PathLike,
                          save_path_pitch: PathLike, save_path_energy: PathLike, pitch_min_freq: float,
                          pitch_max_freq: float, extractor: Optional[DurationExtractor] = None,
                          save_attention: Optional[PathLike] = None
                          ) -> Tuple[Dict[str, DurationStats], Dict[str, Tuple[float, float]]]:
    """train_tacotron.py:110-140 in one pass over the teacher's batches.  `model`, `batches`, `extractor` and
    `save_attention` are those of durations.extract_durations, whose alg/ (and attention) files this writes unchanged.
    Per batch, ft_token_values runs behind ft_dur_extract on the same stream, on the batch's mel and the durations
    still on the device; only raw_pitch/<item_id>.npy is read from disk.  Speakers are the batches' speaker_name
    entries.  The token pitches stay on the device until the last batch, then are normalised per speaker and written
    with the energies, as extract_pitch_energy writes them.  Returns (the duration stats, which the reference pickles
    to paths.duration_stats, {speaker: (pitch mean, pitch std)})."""
    if int(model.r) != 1:
        raise _lib.FtError(f'create_align_features: the model must run at r = 1 (got r = {int(model.r)})')
    extractor = extractor or DurationExtractor(silence_threshold=-11., silence_prob_shift=0.25)
    for d in (alg_dir, save_path_pitch, save_path_energy) + ((save_attention,) if save_attention else ()):
        os.makedirs(d, exist_ok=True)
    model.eval()
    model.decoder.prenet.train()
    stats: Dict[str, DurationStats] = {}
    pending = _Pending(save_path_energy)
    with torch.no_grad():
        for batch in batches:
            pitch, pitch_len = _raw_pitch(raw_pitch_dir, batch['item_id'])
            attn = model.align(batch)
            dev = attn.device
            mel = batch['mel'].to(dev, non_blocking=True).contiguous()
            x = batch['x'].to(dev, non_blocking=True)
            res = extractor.extract_batch(attn.contiguous(), x, batch['x_len'], mel, batch['mel_len'])
            tv = TokenValues.extract_batch(mel, batch['mel_len'], pitch.to(dev, non_blocking=True), pitch_len,
                                           res.durations, batch['x_len'], pitch_min_freq, pitch_max_freq, check=False)
            write_durations(res, batch, attn, alg_dir, save_attention, stats)
            _raise_bad(tv.status, 'create_align_features')
            pending.add(tv, batch['item_id'], batch['speaker_name'], batch['x_len'].tolist())
        return stats, pending.finish(save_path_pitch)
