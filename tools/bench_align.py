"""Duration extraction on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_align.py [--batch 32] [--iters 20] [--warmup 3] [--seed 0]

A seeded batch of B items with Tx ~ U[120, 180] tokens and Tm ~ U[700, 900] frames (near-diagonal attentions, 80 mel
channels, a silent stretch per item) runs through DurationExtractor.extract_batch (one ft_dur_extract launch).
Reported: ms per batch (HIP events, mean over --iters after --warmup), items/s, and the algorithmic work behind it,
computed from the shapes: the DP visits every cell once (three fp64 compares and one fp64 add: 4 flop per cell) and
reads each cell's attention twice (the DP and the align-score argmax), the mel once, and writes the durations.
Then the Tacotron teacher (forwardtacotron_amd/tacotron.py): a seed-0 full-size singlespeaker model in extraction mode
(eval, decoder prenet dropout on) over the same batch at r = 1 (S = max(mel_len) + 1 decoder steps):
  encoder_ms            encoder, token projections, decoder prenet and the prenet half of the GRU input projection
  recurrence_ms         ft_taco_attend alone (3 launches per decoder step); recurrence_us_per_step = / S
  recurrence_host_us_per_step   host time to enqueue those launches (no sync): close to the device time per step means
                        the recurrence is host-bound (recurrence_bound); the kernel-trace sums of rocprofv3 give the other
                        side of that comparison (profiles/tacotron_teacher.txt)
  mel_path_ms           rnn_input, the two one-direction LSTM-512 layers (lstm_layer_ms each: projection + recurrence),
                        mel_proj, postnet, post_proj
  align_ms / forward_ms the public calls end to end
  torch_fp32_*_ms       the float restatement of the tests (tests/taco_cpu.py, stock torch ops, per-step loop) in fp32 on
                        the same GPU (--no-torch skips it)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd.durations import DurationExtractor  # noqa: E402
from forwardtacotron_amd.tacotron import Tacotron  # noqa: E402

# configs/singlespeaker.yaml, tacotron.model
SINGLESPEAKER = dict(embed_dims=256, num_chars=135, encoder_dims=128, decoder_dims=256, n_mels=80, postnet_dims=128,
                     encoder_k=16, lstm_dims=512, postnet_k=8, num_highways=4, dropout=0.5, stop_threshold=-11.,
                     speaker_emb_dim=0)


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


def timed(fn, iters, warmup):
    """ms per call (HIP events around `iters` back-to-back calls after `warmup`)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def teacher(x, mel, iters, warmup, with_torch):
    torch.manual_seed(0)
    model = Tacotron(**SINGLESPEAKER).cuda().eval()
    model.decoder.prenet.train()                     # extraction mode (train_tacotron.py:118-119)
    B = x.shape[0]
    batch = {'x': x, 'mel': mel, 'speaker_emb': torch.zeros(B, 0, device='cuda')}
    out = {}
    with torch.no_grad():
        ep, epq, P = model._attend_inputs(x, mel, None)
        S = P.shape[0]
        out['decoder_steps'] = S
        out['encoder_ms'] = timed(lambda: model._attend_inputs(x, mel, None), iters, warmup)
        out['recurrence_ms'] = timed(lambda: model._attend(ep, epq, P, False), iters, warmup)
        out['recurrence_us_per_step'] = out['recurrence_ms'] * 1e3 / S
        torch.cuda.synchronize()
        t = time.perf_counter()
        model._attend(ep, epq, P, False)
        host = (time.perf_counter() - t) * 1e6 / S
        torch.cuda.synchronize()
        out['recurrence_host_us_per_step'] = host
        out['launches_per_decoder_step'] = 3         # GRU cell, LSA energies, softmax + context (ft_taco.hip)
        out['recurrence_bound'] = 'host' if host >= 0.9 * out['recurrence_us_per_step'] else 'device'
        _, hist = model._attend(ep, epq, P, True)
        out['mel_path_ms'] = timed(lambda: model._mel_path(hist), iters, warmup)
        x1 = H.linear_fwd(hist, model.decoder.rnn_input.weight, model.decoder.rnn_input.bias)
        out['lstm_layer_ms'] = timed(lambda: model._lstm(model.decoder.res_rnn1, x1), iters, warmup)
        out['lstm_us_per_step'] = out['lstm_layer_ms'] * 1e3 / S
        out['align_ms'] = timed(lambda: model.align(batch), iters, warmup)
        out['forward_ms'] = timed(lambda: model(batch), iters, warmup)
        if with_torch:
            sys.path.insert(0, os.path.join(ROOT, 'tests'))
            import taco_cpu
            P32 = {k: v.detach() for k, v in model.state_dict().items()}
            cfg = dict(encoder_k=16, postnet_k=8, num_highways=4)
            model.eval()                             # the restatement runs without dropout masks
            out['torch_fp32_align_ms'] = timed(lambda: taco_cpu.forward(P32, batch, cfg, 1, with_mel=False), 1, 1)
            out['torch_fp32_forward_ms'] = timed(lambda: taco_cpu.forward(P32, batch, cfg, 1), 1, 1)
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-torch', action='store_true', help='skip the stock-torch fp32 comparison')
    ap.add_argument('--no-teacher', action='store_true', help='duration extraction only')
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
    taco = dict.fromkeys(('encoder_ms', 'recurrence_ms', 'recurrence_us_per_step', 'mel_path_ms'))
    if not a.no_teacher:
        taco = teacher(x, mel, a.iters, a.warmup, not a.no_torch)
    print(json.dumps({
        'metric': 'duration_extraction', 'batch': a.batch, 'mean_x_len': float(x_len.float().mean()),
        'mean_mel_len': float(mel_len.float().mean()), 'max_diagonals': int((x_len + mel_len - 1).max()),
        **taco,
        'durations_ms': round(ms, 4), 'durations_items_per_s': round(a.batch / ms * 1e3, 1),
        'durations_us_per_diagonal': round(ms * 1e3 / int((x_len + mel_len - 1).max()), 4),
        'durations_cells': cells, 'durations_flop': 4 * cells, 'durations_bytes': bytes_,
    }))


if __name__ == '__main__':
    main()
