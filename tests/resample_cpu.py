"""Float64 numpy restatement of the sample-rate conversion of forwardtacotron_amd/audio.py (csrc/ft_resample.hip): the
polyphase design of scipy.signal.resample_poly (Kaiser 5.0; librosa res_type='polyphase'), written out as one formula.
No scipy in here: tests/test_resample_cpu.py holds this file to scipy, and tests/test_gpu_resample.py holds the kernel to
this file.

    g = gcd(source_sr, target_sr), up = target_sr / g, down = source_sr / g, R = max(up, down), half = 10 R
    h[i] = (1 / R) sinc((i - half) / R) kaiser(2 half + 1, 5.0)[i]   for i in [0, 2 half];   h /= sum(h);   h *= up
    n_out = ceil(n_in * up / down)
    y[n] = sum over k in [0, n_in) with 0 <= half + n down - k up <= 2 half, ascending k, of h[half + n down - k up] x[k]
"""
import math

import numpy as np

CASES = {'48000->22050': (48000, 22050), '44100->22050': (44100, 22050), '16000->22050': (16000, 22050),
         '22050->16000': (22050, 16000), '22050->44100': (22050, 44100)}
LENGTHS = (1, 2, 7, 319, 320, 321, 1500)
EPS32 = 2.0 ** -24


def ratio(source_sr, target_sr):
    g = math.gcd(source_sr, target_sr)
    return target_sr // g, source_sr // g


def out_len(n_in, up, down):
    return (n_in * up + down - 1) // down


def filt(up, down):
    """-> (h float64 [2 half + 1], half)"""
    R = max(up, down)
    half = 10 * R
    i = np.arange(2 * half + 1)
    h = (1.0 / R) * np.sinc((i - half) / R) * np.kaiser(2 * half + 1, 5.0)
    h /= h.sum()
    h *= up
    return h, half


def terms(n_in, up, down, half):
    """for every output n: (k_first, k_last) inclusive, the samples inside the filter and inside the signal (empty if
    k_first > k_last)"""
    n = np.arange(out_len(n_in, up, down), dtype=np.int64)
    c = half + n * down
    k_first = np.maximum(0, -((2 * half - c) // up))             # ceil((c - 2 half) / up)
    k_last = np.minimum(n_in - 1, c // up)
    return c, k_first, k_last


def resample(x, up, down, dtype=np.float64):
    """-> (y, S, T_n): y[n] summed sequentially in ascending k in `dtype` (float64: the reference; float32: h rounded
    once, every product and every partial sum rounded -- the order of the device, without its fused multiply-add);
    S[n] = sum_k |h[.]| |x[k]| in float64 and T_n = the number of terms, the two factors of the a-priori error bound"""
    x = np.asarray(x)
    assert x.ndim == 1
    if up == down:
        return x.astype(dtype), np.abs(x.astype(np.float64)), np.ones(len(x), dtype=np.int64)
    h64, half = filt(up, down)
    hd, xd = h64.astype(dtype), x.astype(dtype)
    x64 = np.abs(x.astype(np.float64))
    c, k_first, k_last = terms(len(x), up, down, half)
    y = np.zeros(len(c), dtype=dtype)
    S = np.zeros(len(c), dtype=np.float64)
    T_n = np.maximum(0, k_last - k_first + 1)
    for j in range(int(T_n.max()) if len(c) else 0):            # the j-th term of every output at once: ascending k
        k = k_first + j
        on = k <= k_last
        kk = np.where(on, k, 0)
        idx = np.where(on, c - kk * up, 0)
        y = np.where(on, (y + hd[idx] * xd[kk]).astype(dtype), y)
        S += np.where(on, np.abs(h64[idx]) * x64[kk], 0.0)
    return y, S, T_n


def bound(S, T_n):
    """|y_fp32 - y_fp64| <= (T_n + 2) 2^-24 sum_k |h| |x|: one rounding of h and one of the product per term (a fused
    multiply-add has only the first), T_n - 1 roundings of the partial sums, each at most 2^-24 of a partial sum that
    sum_k |h| |x| bounds, and the second-order terms inside the slack of 2"""
    return (T_n + 2) * EPS32 * S


def signal(n, seed):
    """a speech-like float32 test signal in [-1, 1]: two tones, a decaying one and noise"""
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(seed)
    return (0.5 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1200 * t) * np.exp(-3 * t)
            + 0.05 * rng.standard_normal(n)).astype(np.float32)
