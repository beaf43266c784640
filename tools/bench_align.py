"""Duration extraction on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_align.py [--batch 32] [--iters 20] [--warmup 3] [--seed 0]

A seeded batch of B items with Tx ~ U[120, 180] tokens and Tm ~ U[700, 900] frames (near-diagonal attentions, 80 mel
channels, a silent stretch per item) runs through DurationExtractor.extract_batch (one ft_dur_extract launch).
Reported: ms per batch (HIP events, mean over --iters after --warmup), items/s, and the algorithmic work behind it,
computed from the shapes: the DP visits every cell once (three fp64 compares and one fp64 add: 4 flop per cell) and
reads each cell's attention twice (the DP and the align-score argmax), the mel once, and writes the durations.
The Tacotron teacher stages (encoder, attention recurrence, mel path) are not part of this package yet: their fields
are null.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from forwardtacotron_amd.durations import DurationExtractor  # noqa: E402


def make_batch(B, seed, n_mels=80):
    rng = np.random.default_rng(seed)
    x_len = rng.integers(120, 181, B)
    mel_len = rng.integers(700, 901, B)
    Tx, Tm = int(x_len.max()), int(mel_len.max()) + 1
    attn = np.zeros((B, Tm, Tx), np.float32)
    mel = np.full((B, n_mels, Tm), -11.5129, np.float32)
    x = np.zeros((B, Tx), np.int64)
    for b in range(B):
        m, t = int(mel_len[b]), int(x_len[b])
        centre = np.linspace(0, t - 1, m) + rng.normal(0, 2., m)
        logits = -0.2 * (np.arange(t)[None, :] - centre[:, None]) ** 2 + rng.normal(0, 1., (m, t))
        a = np.exp(logits - logits.max(1, keepdims=True))
        attn[b, :m, :t] = a / a.sum(1, keepdims=True)
        mel[b, :, :m] = rng.normal(-6., 3., (n_mels, m))
        s = int(rng.integers(0, m - 40))
        mel[b, :, s:s + 40] = -11.5
        x[b, :t] = rng.integers(0, 60, t)
    return (torch.from_numpy(attn).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(x_len),
            torch.from_numpy(mel).cuda(), torch.from_numpy(mel_len))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    attn, x, x_len, mel, mel_len = make_batch(a.batch, a.seed)
    x_len_d, mel_len_d = x_len.cuda(), mel_len.cuda()
    ext = DurationExtractor(silence_threshold=-11., silence_prob_shift=0.25)
    res = ext.extract_batch(attn, x, x_len_d, mel, mel_len_d)          # checked launch
    assert bool((res.durations.sum(1).cpu() == mel_len).all())
    for _ in range(a.warmup):
        ext.extract_batch(attn, x, x_len_d, mel, mel_len_d, check=False)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.iters):
        ext.extract_batch(attn, x, x_len_d, mel, mel_len_d, check=False)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.iters
    cells = int((x_len * mel_len).sum())
    n_mels = mel.shape[1]
    bytes_ = 2 * 4 * cells + 4 * n_mels * int(mel_len.sum()) + 8 * x.numel() + 8 * x.numel()
    print(json.dumps({
        'metric': 'duration_extraction', 'batch': a.batch, 'mean_x_len': float(x_len.float().mean()),
        'mean_mel_len': float(mel_len.float().mean()), 'max_diagonals': int((x_len + mel_len - 1).max()),
        'encoder_ms': None, 'recurrence_ms': None, 'recurrence_us_per_step': None, 'mel_path_ms': None,
        'durations_ms': round(ms, 4), 'durations_items_per_s': round(a.batch / ms * 1e3, 1),
        'durations_us_per_diagonal': round(ms * 1e3 / int((x_len + mel_len - 1).max()), 4),
        'durations_cells': cells, 'durations_flop': 4 * cells, 'durations_bytes': bytes_,
    }))


if __name__ == '__main__':
    main()
