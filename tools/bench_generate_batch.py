"""Ragged-batch synthesis against the loop of single-sentence calls it replaces.

    python tools/bench_generate_batch.py [--items 32] [--min-len 20] [--max-len 128] [--rounds 10] [--warmup 3]
                                         [--window 0.5]

The production single-speaker ForwardTacotron (default initialisation, seed 0; the duration predictor's output layer is
shifted so that a token lasts a few frames, as a trained model's does), one ragged batch of --items sentences with x_len
drawn from [--min-len, --max-len] under a fixed seed.  Two ways to synthesise them on the same GPU:

  batch : one generate_batch(x, x_len) call
  loop  : generate(x[b:b+1, :x_len[b]]) for every item

Both are warmed up at the very shapes they are timed at, then timed in alternation (batch, loop, batch, loop, ...) with a
host clock around work that ends in a device synchronise.  A timed window holds as many back-to-back repetitions as fill
--window seconds (counted from the warm-up's last call; one synchronise at the end of the window), so that it measures
the device and not the clock; times are per repetition.  Before any timing the two results are compared item by item at
the timed shapes.  Prints per-round times, medians and one JSON line.  Needs a GPU: there is no CPU fallback.
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

from forwardtacotron_amd import data, hip  # noqa: E402
from forwardtacotron_amd.model import ForwardTacotron  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_generate_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

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
    xd = x.cuda()
    singles = [xd[b:b + 1, :int(x_len[b])].contiguous() for b in range(a.items)]

    def batch():
        return model.generate_batch(xd, x_len)

    def loop():
        return [model.generate(s) for s in singles]

    # results first: the two must agree at the shapes that are timed
    ob, ol = batch(), loop()
    torch.cuda.synchronize()
    hip.check_rnn_status()
    mel_len = ob['mel_len'].tolist()
    worst, bit_equal = 0.0, True
    for b in range(a.items):
        n = ol[b]['mel'].shape[2]
        if n != mel_len[b]:
            raise SystemExit(f'item {b}: {mel_len[b]} frames in the batch, {n} alone')
        for k in ('mel', 'mel_post'):
            d = (ob[k][b, :, :n] - ol[b][k][0]).abs().max().item()
            worst = max(worst, d)
            bit_equal &= torch.equal(ob[k][b, :, :n], ol[b][k][0])
    print(f'{a.items} items, x_len {int(x_len.min())}..{Tx} (sum {int(x_len.sum())}), frames {min(mel_len)}..{max(mel_len)} '
          f'(sum {sum(mel_len)}); batch vs loop: max |diff| {worst:.3e}, bit-equal {bit_equal}')

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    wb = wl = 0.0
    for _ in range(max(1, a.warmup)):
        wb, wl = timed(batch), timed(loop)
    nb, nl = (max(1, math.ceil(a.window * 1e3 / w)) for w in (wb, wl))
    print(f'window {a.window} s: {nb} generate_batch calls, {nl} passes over the loop')
    tb, tl = [], []
    for r in range(a.rounds):
        tb.append(timed(batch, nb))
        tl.append(timed(loop, nl))
        print(f'round {r}: batch {tb[-1]:8.3f} ms   loop {tl[-1]:8.3f} ms')
    hip.check_rnn_status()
    mb, ml = statistics.median(tb), statistics.median(tl)
    print(f'median: batch {mb:.3f} ms (min {min(tb):.3f}, max {max(tb):.3f})   loop {ml:.3f} ms (min {min(tl):.3f}, '
          f'max {max(tl):.3f})   loop / batch = {ml / mb:.2f}x   {ml / a.items:.3f} ms per single call')
    print(json.dumps({'items': a.items, 'x_len_min': int(x_len.min()), 'x_len_max': Tx, 'frames': sum(mel_len),
                      'batch_ms_median': round(mb, 3), 'loop_ms_median': round(ml, 3), 'rounds': a.rounds,
                      'calls_per_window': [nb, nl], 'max_abs_diff': worst, 'bit_equal': bit_equal}))


if __name__ == '__main__':
    main()
