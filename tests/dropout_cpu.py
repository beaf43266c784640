"""The counter-based dropout mask of the HIP kernels, restated in numpy from the formula and the comment at ft_hash32 /
ft_dropout_keep in csrc/ft_common.h.  Pure integer arithmetic (plus one exact int -> float32 conversion), so it is bit
for bit what the kernels compute; tests/test_gpu_dropout.py ties the two together.  Nothing here touches the GPU or the
package's own mask: the masks built here feed the float64 / fp32 oracles of the dropout-on tests.

Which flat index a site uses (site_mask's `shape`):
  softmax + dropout (fp32 mode) and the fused attention (bf16 mode): the probabilities [B,nh,T,T], index
      ((b * nh + h) * T + q) * T + k -- the UNPADDED key count, whatever the leading dimension of the score buffer;
  add + LayerNorm with dropout on the residual branch: [rows, D], index row * D + c, rows = B * T batch-major;
  everything else (ops.DropoutFn): the contiguous form of the tensor DropoutFn receives.
"""
import numpy as np
import torch

GOLDEN = 0x9E3779B97F4A7C15          # stride of base._seed()'s stream
MASK62 = (1 << 62) - 1
MASK64 = (1 << 64) - 1


def hash32(seed: int, idx) -> np.ndarray:
    """ft_hash32(seed, idx): seed a Python int (taken mod 2^64), idx an integer array (or int) of 64-bit indices"""
    seed = int(seed) & MASK64
    lo, hi = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    i = np.atleast_1d(np.asarray(idx)).astype(np.uint64)          # arrays wrap silently mod 2^32, as the kernel does
    h = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32) ^ ((i >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B1))
    h = (h ^ lo) * np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(15)
    h = (h + hi) * np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0x27D4EB2F)
    h ^= h >> np.uint32(16)
    return h.reshape(np.shape(idx))


def u24(seed: int, idx) -> np.ndarray:
    """(h >> 8) * 2^-24 as float32: exact, 24 bits fit the significand"""
    return (hash32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_at(seed: int, idx, p: float) -> np.ndarray:
    """ft_dropout_keep at the given indices: u >= float32(p)"""
    return u24(seed, idx) >= np.float32(p)


def keep(seed: int, n: int, p: float, offset: int = 0) -> np.ndarray:
    """bool [n]: element offset + i is kept"""
    return keep_at(seed, np.arange(n, dtype=np.uint64) + np.uint64(offset), p)


def drop_probability(p: float) -> float:
    """exact probability of u < float32(p) for a uniform 24-bit u: ceil(float32(p) * 2^24) / 2^24"""
    return float(np.ceil(np.float64(np.float32(p)) * 2.0 ** 24)) / 2.0 ** 24


def seed_stream(torch_seed: int, count: int, start: int = 1):
    """the seeds base._seed() returns for draws start .. start + count - 1 after torch.manual_seed(torch_seed) has
    re-based it: one torch.randint(0, 2**62, (1,)) from the host generator, then (base + GOLDEN * k) mod 2^62.  The
    global generator is left as it was."""
    g = torch.Generator()
    g.manual_seed(torch_seed)
    base = int(torch.randint(0, 2 ** 62, (1,), generator=g).item())
    return [(base + GOLDEN * k) & MASK62 for k in range(start, start + count)]


def site_mask(seed: int, shape, p: float, dtype=np.float64) -> np.ndarray:
    """keep * 1/(1-p) over the flat element index of a contiguous tensor of `shape` (see the module docstring for which
    tensor each site indexes); p <= 0: ones, as the sites draw nothing then"""
    n = int(np.prod(shape))
    if p <= 0.0:
        return np.ones(shape, dtype=dtype)
    k = keep(seed, n, p).reshape(shape)
    return k.astype(dtype) * (dtype(1.0) / (dtype(1.0) - dtype(np.float32(p))))    # the kernels get p as a float
