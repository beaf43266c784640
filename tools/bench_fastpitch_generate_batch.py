"""FastPitch ragged-batch synthesis against the loop of single-sentence calls it replaces, and against itself without
the length-aware attention kernel.

    python tools/bench_fastpitch_generate_batch.py [--items 32] [--min-len 20] [--max-len 128] [--rounds 10]
                                                   [--warmup 3] [--window 0.5] [--modes fp32,bf16]

The production FastPitch (data.FASTPITCH_MODEL, default initialisation, seed 0; the duration predictor's output layer is
rescaled so that a token lasts a few frames, as a trained model's does), one ragged batch of --items sentences with x_len
drawn from [--min-len, --max-len] under a fixed seed -- the batch of tools/bench_generate_batch.py.  Per matmul mode,
three ways to synthesise them on the same GPU:

  batch  : one generate_batch(x, x_len) call                       (ft_attn_fwd_lens reads the lengths on the device)
  masked : the same call with FT_ATTN_LENS=0                        (mha_fwd's attention route with a byte mask + mask_rows)
  loop   : generate(x[b:b+1, :x_len[b]]) for every item

All three are warmed up at the very shapes they are timed at, then timed in alternation (batch, masked, loop, batch, ...)
with a host clock around work that ends in a device synchronise.  A timed window holds as many back-to-back repetitions
as fill --window seconds (one synchronise at its end); times are per repetition.  Before any timing the results are
compared item by item at the timed shapes.  Also reported: C-ABI entry calls per repetition (host-side count of
_lib.call: one call is one launch for most entries, a few for the GEMM launchers), the frames, the share of the packed
rows that is padding, and the attention alone at the frame-side shape (device events).  Prints per-round times,
medians and one JSON line per mode.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from forwardtacotron_amd import _lib, data, hip  # noqa: E402
from forwardtacotron_amd import fastpitch as FPM  # noqa: E402

_calls = [0]
_real_call = _lib.call


def _counting_call(name, *args):
    _calls[0] += 1
    return _real_call(name, *args)


def count_calls(fn):
    _lib.call = _counting_call
    _calls[0] = 0
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.call = _real_call
    return _calls[0]


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def attention_alone(B, T, lens, d, nh, mode, reps=20):
    """the frame-side attention on its own: ft_attn_fwd_lens vs the masked route of the mode -> (us, us), device events"""
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, T, 3 * d, generator=g).cuda()
    key_pad = (torch.arange(T, device='cuda')[None, :] >= lens[:, None]).to(torch.uint8).contiguous()
    scale = 1.0 / math.sqrt(d // nh)

    def new():
        return hip.attn_fwd_lens(qkv, lens, nh, scale)

    def old():
        if mode == 'bf16':
            return hip.mask_rows(hip.attn_fwd(qkv, key_pad, nh, scale, 0.0, 0)[0], lens)
        return hip.mask_rows(FPM._attn_unfused(qkv, key_pad, nh, scale, 0.0, 0)[0], lens)

    out = []
    with hip.gemm_precision(mode):
        for fn in (new, old):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--modes', default='fp32,bf16')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_fastpitch_generate_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

    cfg = dict(data.FASTPITCH_MODEL)
    torch.manual_seed(0)
    model = FPM.FastPitch(**cfg)
    with torch.no_grad():
        model.dur_pred.lin.weight.mul_(3.0)
        model.dur_pred.lin.bias.fill_(2.5)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(a.seed)
    x_len = torch.randint(a.min_len, a.max_len + 1, (a.items,), generator=g)
    Tx = int(x_len.max())
    x = torch.zeros(a.items, Tx, dtype=torch.long)
    for b in range(a.items):
        x[b, :int(x_len[b])] = torch.randint(1, cfg['num_chars'], (int(x_len[b]),), generator=g)
    xd = x.cuda()
    singles = [xd[b:b + 1, :int(x_len[b])].contiguous() for b in range(a.items)]

    def batch():
        os.environ['FT_ATTN_LENS'] = '1'
        return model.generate_batch(xd, x_len)

    def masked():
        os.environ['FT_ATTN_LENS'] = '0'
        try:
            return model.generate_batch(xd, x_len)
        finally:
            os.environ['FT_ATTN_LENS'] = '1'

    def loop():
        return [model.generate(s) for s in singles]

    for mode in a.modes.split(','):
        model.matmul_dtype = mode
        print(f'==== matmul mode {mode} ====')
        # results first: the three must agree at the shapes that are timed
        ob, om, ol = batch(), masked(), loop()
        torch.cuda.synchronize()
        mel_len = ob['mel_len'].tolist()
        flips = [b for b in range(a.items) if ol[b]['mel'].shape[2] != mel_len[b]]
        if flips and mode == 'fp32':
            raise SystemExit(f'items {flips}: other frame counts in the batch than alone')
        worst, bit_equal = 0.0, not flips
        for b in range(a.items):
            if b in flips:          # bf16: a duration within the mode's rounding noise of a half-integer
                continue
            n = mel_len[b]
            d = (ob['mel'][b, :, :n] - ol[b]['mel'][0]).abs().max().item()
            worst = max(worst, d)
            bit_equal &= torch.equal(ob['mel'][b, :, :n], ol[b]['mel'][0])
        same_len = om['mel_len'].tolist() == mel_len
        vs_masked = (ob['mel'] - om['mel']).abs().max().item() if same_len else float('nan')
        Tm = max(mel_len)
        pad_share = 1.0 - sum(mel_len) / (a.items * Tm)
        print(f'{a.items} items, x_len {int(x_len.min())}..{Tx} (sum {int(x_len.sum())}), frames {min(mel_len)}..{Tm} '
              f'(sum {sum(mel_len)}, {100 * pad_share:.1f} % of the {a.items} x {Tm} packed rows are padding)')
        print(f'batch vs loop: max |diff| {worst:.3e}, bit-equal {bit_equal}, items with another frame count {flips}; '
              f'batch vs masked: max |diff| {vs_masked:.3e}')
        calls = {n: count_calls(f) for n, f in (('batch', batch), ('masked', masked), ('loop', loop))}
        print(f'C-ABI calls per repetition: batch {calls["batch"]}, masked {calls["masked"]}, loop {calls["loop"]}')
        w = {}
        for _ in range(max(1, a.warmup)):
            w = {'batch': timed(batch), 'masked': timed(masked), 'loop': timed(loop)}
        reps = {k: max(1, math.ceil(a.window * 1e3 / v)) for k, v in w.items()}
        print(f'window {a.window} s: {reps["batch"]} batch calls, {reps["masked"]} masked calls, {reps["loop"]} passes '
              f'over the loop')
        t = {'batch': [], 'masked': [], 'loop': []}
        for r in range(a.rounds):
            for k, fn in (('batch', batch), ('masked', masked), ('loop', loop)):
                t[k].append(timed(fn, reps[k]))
            print(f'round {r}: batch {t["batch"][-1]:8.3f} ms   masked {t["masked"][-1]:8.3f} ms   loop {t["loop"][-1]:8.3f} ms')
        med = {k: statistics.median(v) for k, v in t.items()}
        print('median: ' + '   '.join(f'{k} {med[k]:.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})' for k in t)
              + f'   loop / batch = {med["loop"] / med["batch"]:.2f}x   masked / batch = {med["masked"] / med["batch"]:.3f}x')
        att_new, att_old = attention_alone(a.items, Tm, ob['mel_len'], cfg['d_model'], cfg['postnet_heads'], mode)
        print(f'frame-side attention alone [B {a.items}, T {Tm}, heads {cfg["postnet_heads"]}, hd '
              f'{cfg["d_model"] // cfg["postnet_heads"]}]: ft_attn_fwd_lens {att_new:.1f} us, masked route + mask_rows '
              f'{att_old:.1f} us')
        print(json.dumps({'mode': mode, 'items': a.items, 'x_len_min': int(x_len.min()), 'x_len_max': Tx,
                          'frames': sum(mel_len), 'Tm': Tm, 'pad_share': round(pad_share, 4),
                          'batch_ms_median': round(med['batch'], 3), 'masked_ms_median': round(med['masked'], 3),
                          'loop_ms_median': round(med['loop'], 3), 'rounds': a.rounds, 'calls': calls,
                          'attn_lens_us': round(att_new, 1), 'attn_masked_us': round(att_old, 1),
                          'max_abs_diff_vs_loop': worst, 'bit_equal_vs_loop': bit_equal}))


if __name__ == '__main__':
    main()
