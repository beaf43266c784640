"""The poison-filling allocator the GPU tests put in place of a module's `_empty` (audio, vocoder, melgan, hifigan,
pitch): every buffer the module allocates starts as NaN (floating point), 255 (bytes) or a junk integer, so a kernel that
reads what it never wrote shows up in the result."""
import torch


def poison(*shape, dtype=torch.float32, device=None):
    t = torch.empty(*shape, dtype=dtype, device=device)
    if dtype.is_floating_point:
        return t.fill_(float('nan'))
    if dtype == torch.int16:                      # (the GAN vocoders' wav_int16)
        return t.fill_(-12345)
    return t.fill_(255) if dtype == torch.uint8 else t.fill_(-123456789)
