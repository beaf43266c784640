"""MelGAN.inference_batch on the mels of a ragged synthesis batch, against the same generator in stock fp32 torch.

    python tools/bench_melgan_batch.py [--items 32] [--min-len 20] [--max-len 128] [--rounds 8] [--warmup 2] [--window 0.5]

The sentences, the acoustic model and its generate_batch call are those of tools/bench_generate_batch.py; its 'mel_post'
and 'mel_len' go into a full-width MelGAN (default initialisation, seed 0).  Three ways to turn them into audio on the
same GPU, in the same process, timed in alternating rounds (ours, per-item, padded, ours, ...):

  ours     : one MelGAN.inference_batch(mel_post, mel_len) call
  per-item : the stock torch generator (nn.Conv1d / nn.ConvTranspose1d / nn.ReflectionPad1d with the folded weights, as
             the hub model is after remove_weight_norm) called once per item on mel[b:b+1, :, :mel_len[b]] + the ten
             appended frames -- what a user of the reference does today
  padded   : that generator called ONCE on the padded batch (items shorter than Tmax get wrong samples near their end:
             a speed reference only)

Each is warmed up at the shapes it is timed at; a timed window holds as many back-to-back repetitions as fill --window
seconds and ends in one device synchronise; times are per repetition.  Before any timing, ours is compared with the
per-item stock result item by item.  Then the per-kernel split of ours: device events around every launch of one call
(median over --rounds calls), summed per stage, with the FLOP and the least bytes (input read once, output written once)
counted from the items' own lengths.  Prints everything and one JSON line.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from forwardtacotron_amd import data, hip  # noqa: E402
from forwardtacotron_amd import melgan as M  # noqa: E402
from forwardtacotron_amd.model import ForwardTacotron  # noqa: E402


class StockResStack(nn.Module):
    def __init__(self, src):
        super().__init__()
        self.blocks = nn.ModuleList([nn.Sequential(nn.LeakyReLU(0.2), nn.ReflectionPad1d(d), _plain(b[2]), nn.LeakyReLU(0.2),
                                                   _plain(b[4])) for b, d in zip(src.blocks, M.DILATIONS)])
        self.shortcuts = nn.ModuleList([_plain(s) for s in src.shortcuts])

    def forward(self, x):
        for block, shortcut in zip(self.blocks, self.shortcuts):
            x = shortcut(x) + block(x)
        return x


def _plain(conv):
    """a weight-normed convolution -> the same stock module with the folded weight (remove_weight_norm)"""
    w = M.fold_weight_norm(conv.weight_v.detach(), conv.weight_g.detach())
    if isinstance(conv, nn.ConvTranspose1d):
        out = nn.ConvTranspose1d(conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.padding[0])
    else:
        out = nn.Conv1d(conv.in_channels, conv.out_channels, conv.kernel_size[0], dilation=conv.dilation[0])
    with torch.no_grad():
        out.weight.copy_(w)
        out.bias.copy_(conv.bias)
    return out


def stock_generator(voc):
    layers = []
    for m in voc.generator:
        if isinstance(m, M.ResStack):
            layers.append(StockResStack(m))
        elif isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
            layers.append(_plain(m))
        else:
            layers.append(type(m)(m.padding) if isinstance(m, nn.ReflectionPad1d) else
                          nn.LeakyReLU(0.2) if isinstance(m, nn.LeakyReLU) else nn.Tanh())
    return nn.Sequential(*layers)


def stage_costs(voc, mel_len):
    """[(name, FLOP, least bytes)] per launch of one inference_batch call, from the items' own lengths"""
    frames = sum(n + M.TAIL_FRAMES for n in mel_len)
    ch = voc.channels
    out = [('conv_in', frames * 2 * 7 * voc.mel_channel * ch[0], 4 * frames * (voc.mel_channel + ch[0]))]
    scale = 1
    for i, (_, s, _) in enumerate(voc.upsamples):
        rows = frames * scale * s
        out.append((f'upsample{i}', rows * 2 * 2 * ch[i] * ch[i + 1], 4 * (rows // s * ch[i] + rows * ch[i + 1])))
        scale *= s
        for d in M.DILATIONS:
            out.append((f'resblock{i}.d{d}', rows * 2 * 5 * ch[i + 1] ** 2, 4 * 2 * rows * ch[i + 1]))
    rows = frames * scale
    out.append(('conv_out', rows * 2 * 7 * ch[4], 4 * rows * ch[4] + 6 * sum(mel_len) * scale))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_melgan_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

    cfg = dict(data.SINGLESPEAKER_MODEL)
    torch.manual_seed(0)
    model = ForwardTacotron(**cfg)
    with torch.no_grad():
        model.dur_pred.lin.weight.mul_(30.0)
        model.dur_pred.lin.bias.fill_(2.5)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(a.seed)
    x_len = torch.randint(a.min_len, a.max_len + 1, (a.items,), generator=g)
    Tx = int(x_len.max())
    x = torch.zeros(a.items, Tx, dtype=torch.long)
    for b in range(a.items):
        x[b, :int(x_len[b])] = torch.randint(1, cfg['num_chars'], (int(x_len[b]),), generator=g)
    torch.manual_seed(0)
    voc = M.MelGAN().cuda().eval()
    stock = stock_generator(voc).cuda().eval()
    with torch.no_grad():
        gen = model.generate_batch(x.cuda(), x_len)
    torch.cuda.synchronize()
    hip.check_rnn_status()
    mel, mel_len_d = gen['mel_post'], gen['mel_len']
    mel_len = mel_len_d.tolist()
    mel_len_h = torch.tensor(mel_len, dtype=torch.int64)
    B, n_mels, Tmax = mel.shape
    hop = voc.hop_length
    tail = torch.full((1, n_mels, M.TAIL_FRAMES), M.PAD_VALUE, device=mel.device)
    singles = [torch.cat((mel[b:b + 1, :, :n], tail), dim=2) for b, n in enumerate(mel_len)]
    padded_in = torch.cat((mel, tail.expand(B, -1, -1)), dim=2)

    def ours():
        return voc.inference_batch(mel, mel_len_h)

    def per_item():
        outs = []
        for s in singles:
            audio = stock((s + 5.0) / 5.0).squeeze()[:-(hop * M.TAIL_FRAMES)]
            outs.append((M.MAX_WAV_VALUE * audio).clamp(min=-M.MAX_WAV_VALUE, max=M.MAX_WAV_VALUE - 1).short())
        return outs

    def padded():
        audio = stock((padded_in + 5.0) / 5.0).squeeze(1)[:, :-(hop * M.TAIL_FRAMES)]
        return (M.MAX_WAV_VALUE * audio).clamp(min=-M.MAX_WAV_VALUE, max=M.MAX_WAV_VALUE - 1).short()

    with torch.no_grad():
        oo, ol = ours(), per_item()
        torch.cuda.synchronize()
        worst = max(int((oo['wav_int16'][b, :hop * n].int() - ol[b].int()).abs().max()) for b, n in enumerate(mel_len))
        wf = max(float((oo['wav'][b, :hop * n] - stock((s + 5.0) / 5.0).squeeze()[:hop * n]).abs().max())
                 for (b, n), s in zip(enumerate(mel_len), singles))
        print(f'{B} items, frames {min(mel_len)}..{max(mel_len)} (sum {sum(mel_len)}), Tmax {Tmax}; ours vs stock per item: '
              f'max |int16 diff| {worst}, max |wav diff| {wf:.2e}')

        def timed(fn, reps=1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3 / reps

        fns = {'ours': ours, 'per-item': per_item, 'padded': padded}
        w = {}
        for _ in range(max(1, a.warmup)):
            for k, fn in fns.items():
                w[k] = timed(fn)
        reps = {k: max(1, math.ceil(a.window * 1e3 / w[k])) for k in fns}
        print(f'window {a.window} s: repetitions {reps}')
        t = {k: [] for k in fns}
        for r in range(a.rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, reps[k]))
            print(f'round {r}: ' + '   '.join(f'{k} {t[k][-1]:9.3f} ms' for k in fns))
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in fns:
            print(f'{k:9s} median {med[k]:9.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})')
        print(f"per-item / ours = {med['per-item'] / med['ours']:.2f}x   padded / ours = {med['padded'] / med['ours']:.2f}x")

        # ---- the per-kernel split: device events around every launch of one call ------------------------------------
        costs = stage_costs(voc, mel_len)
        names = ('melgan_conv_in', 'melgan_upsample', 'melgan_resblock', 'melgan_conv_out')
        real = {n: getattr(hip, n) for n in names}
        marks = []

        def wrap(fn):
            def run(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*args, **kw)
                e1.record()
                marks.append((e0, e1))
                return out
            return run
        for n in names:
            setattr(hip, n, wrap(real[n]))
        per_call = []
        for _ in range(a.rounds):
            marks.clear()
            ours()
            torch.cuda.synchronize()
            per_call.append([e0.elapsed_time(e1) for e0, e1 in marks])
        for n in names:
            setattr(hip, n, real[n])
    assert all(len(c) == len(costs) for c in per_call)
    split = [statistics.median(c[i] for c in per_call) for i in range(len(costs))]
    print(f'per-kernel split (median of {a.rounds} calls, device events; sum {sum(split):.3f} ms):')
    print(f'  {"launch":16s} {"ms":>8s} {"GFLOP":>8s} {"TFLOP/s":>8s} {"MB":>8s} {"GB/s":>8s}')
    rows = []
    for (name, flop, nbytes), ms in zip(costs, split):
        rows.append({'launch': name, 'ms': round(ms, 4), 'gflop': round(flop / 1e9, 3), 'mb': round(nbytes / 1e6, 1)})
        print(f'  {name:16s} {ms:8.3f} {flop / 1e9:8.2f} {flop / ms / 1e9:8.1f} {nbytes / 1e6:8.1f} {nbytes / ms / 1e6:8.0f}')
    total = sum(c[1] for c in costs)
    print(f'  total {total / 1e9:.1f} GFLOP: {total / med["ours"] / 1e9:.1f} TFLOP/s over the whole call')
    print(json.dumps({'items': B, 'frames': sum(mel_len), 'Tmax': Tmax, 'ours_ms_median': round(med['ours'], 3),
                      'stock_per_item_ms_median': round(med['per-item'], 3), 'stock_padded_ms_median': round(med['padded'], 3),
                      'rounds': a.rounds, 'repetitions': reps, 'max_int16_diff': worst, 'max_wav_diff': wf, 'gflop': round(total / 1e9, 1),
                      'split': rows}))


if __name__ == '__main__':
    main()
