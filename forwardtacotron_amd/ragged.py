"""The intake of a ragged batch, shared by audio.DSP (preprocess_batch, resample_batch), vocoder.GriffinLim
(griffinlim_batch), pitch.LibrosaPitchExtractor (extract_batch) and speaker.VoiceEncoder (embed_batch).  The contract,
stated here once:
  * a batch is a list of 1-D wavs (gather_wavs pads them into one [B, ld] device buffer) or a padded batch with its
    lengths, int64 [B], on the host or on the device (device_lens);
  * host lengths are checked before any launch, and the FtError names the offending list;
  * device lengths are clamped inside the kernels (csrc/ft_common.h: ft_item_len), so nothing indexes out of bounds, and
    one thread per item raises a device flag that LenFlag.check reads after ONE synchronisation at the end of the call;
  * nothing is sized from device values, and with host lengths nothing synchronises.
Every validation failure is raised before the first device operation.  `what` is the caller's name in the messages;
`alloc` is the caller's module-level allocator (the seam the tests poison)."""
from typing import Optional

import numpy as np
import torch

from ._lib import FtError


def gather_wavs(wavs, device, what: str, row_multiple: int = 1, allow_all_empty: bool = True, alloc=torch.empty):
    """list of 1-D numpy arrays or tensors -> (wav [B, ld] fp32 on the device, zero beyond each item; lens [B] int64 on
    the device; Lmax), ld = max(1, Lmax) rounded up to a multiple of row_multiple.  All numpy: one host buffer and one
    copy; otherwise a fill and one copy per item.  No synchronisation either way."""
    if len(wavs) == 0:
        raise FtError(f'{what}: an empty batch')
    if any(getattr(y, 'ndim', None) != 1 for y in wavs):
        raise FtError(f'{what}: every wav must be a 1-D array or tensor')
    lens = [int(y.shape[0]) for y in wavs]
    Lmax = max(lens)
    if Lmax == 0 and not allow_all_empty:
        raise FtError(f'{what}: every wav of the batch is empty')
    ld = -(-max(1, Lmax) // row_multiple) * row_multiple
    wav = alloc(len(wavs), ld, dtype=torch.float32, device=device)
    if all(isinstance(y, np.ndarray) for y in wavs):
        host = np.zeros((len(wavs), ld), dtype=np.float32)
        for b, y in enumerate(wavs):
            host[b, :lens[b]] = y
        wav.copy_(torch.from_numpy(host))
    else:
        wav.zero_()
        for b, y in enumerate(wavs):
            wav[b, :lens[b]] = torch.as_tensor(y).to(device, torch.float32)
    return wav, torch.tensor(lens, dtype=torch.int64).pin_memory().to(device, non_blocking=True), Lmax


def range_message(what: str, name: str, lo: int, hi: int, hi_name: str) -> str:
    return f'{what}: every {name} must be in [{lo}, {hi_name} = {hi}]'


def device_lens(lens, B: int, lo: int, hi: int, what: str, name: str, hi_name: str, device, flag: bool = True):
    """lengths int64 [B] on the host or the device -> (lens on the device, flag).  Host lengths must lie in [lo, hi] and
    are copied from pinned memory without blocking; their flag is None.  Device lengths are taken as they are, with a
    zeroed int32 device flag for the kernels to raise (LenFlag.check reads it), or None with flag=False: the caller's
    kernels clamp silently."""
    if not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(np.asarray(lens))
    if lens.dim() != 1 or lens.numel() != B or lens.dtype != torch.int64:
        raise FtError(f'{what}: {name} must be int64 [B = {B}]')
    if not lens.is_cuda:
        if int(lens.min()) < lo or int(lens.max()) > hi:
            raise FtError(f'{range_message(what, name, lo, hi, hi_name)} (got {lens.tolist()})')
        return lens.pin_memory().to(device, non_blocking=True), None
    return lens.contiguous(), torch.zeros(1, dtype=torch.int32, device=device) if flag else None


def intake(wavs, wav_len, device, what: str, row_multiple: int = 1, allow_all_empty: bool = True, flag: bool = True,
           alloc=torch.empty):
    """Both forms of a batch of wavs -> (wav [B, ld] on the device, lens [B] int64 on the device, L, flag or None): a
    list of 1-D wavs without wav_len (gather_wavs), or a padded float32 [B, L] array or tensor with wav_len
    (device_lens into [0, L]; the tensor is moved to the device as it is laid out)."""
    if wav_len is None:
        if isinstance(wavs, (np.ndarray, torch.Tensor)):
            raise FtError(f'{what}: a padded [B, L] batch needs wav_len; without it pass a list of 1-D wavs')
        return gather_wavs(wavs, device, what, row_multiple, allow_all_empty, alloc) + (None,)
    if isinstance(wavs, np.ndarray):
        wavs = torch.from_numpy(np.ascontiguousarray(wavs, dtype=np.float32))
    if not isinstance(wavs, torch.Tensor) or wavs.dim() != 2 or wavs.dtype != torch.float32:
        raise FtError(f'{what}: with wav_len, the batch must be a float32 [B, L] tensor')
    B, L = wavs.shape
    if B < 1 or (L < 1 and not allow_all_empty):
        raise FtError(f'{what}: an empty batch')
    lens, err = device_lens(wav_len, B, 0, L, what, 'wav_len', 'L', device, flag)
    return wavs.to(device), lens, L, err


class LenFlag:
    """The read-back of device_lens' flag through ONE pinned host word, kept on the object that owns this: that object
    must not run calls with device-side lengths from two threads or on two streams at once."""

    def __init__(self) -> None:
        self._host: Optional[torch.Tensor] = None

    def check(self, flag: Optional[torch.Tensor], message: str) -> None:
        """flag None (host lengths: checked up front): nothing.  Otherwise copy the flag without blocking, synchronise
        the current stream once, and raise FtError(message) if a kernel raised it."""
        if flag is None:
            return
        if self._host is None:
            self._host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._host.copy_(flag, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        if int(self._host[0]) != 0:
            raise FtError(message)
