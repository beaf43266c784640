"""Multispeaker ragged-batch synthesis (MultiForwardTacotron, MultiFastPitch) against the loop of single-sentence calls it
replaces, and MultiFastPitch against itself without the wide-head length-aware attention kernel.

    python tools/bench_multi_generate_batch.py [--items 32] [--min-len 20] [--max-len 128] [--rounds 10] [--warmup 3]
                                               [--window 0.5] [--models mfp,mft] [--modes fp32,bf16]

The production configs (data.MULTI_FASTPITCH_MODEL, data.MULTISPEAKER_MODEL; default initialisation, seed 0, the duration
predictor's output layer rescaled so that a token lasts a few frames), the ragged batch of the other two generate_batch
benches (tools/bench_generate_batch.py: --items sentences, x_len drawn from [--min-len, --max-len] under a fixed seed),
one unit-norm speaker row per sentence, all different.  Ways to synthesise them on the same GPU, in the same process:

  batch  : one generate_batch(x, x_len, speaker_emb) call; MultiFastPitch with FT_ATTN_LENS=1 (head widths 192 / 256 in
           ft_attn_fwd_lens's wide-head layout)
  masked : MultiFastPitch only: the same call with FT_ATTN_LENS=0 (the [B,h,T,T] route with a byte mask + mask_rows)
  loop   : generate(x[b:b+1, :x_len[b]], speaker_emb[b:b+1]) for every item

All are warmed up at the very shapes they are timed at, then timed in alternation with a host clock around work that
ends in a device synchronise; a timed window holds as many back-to-back repetitions as fill --window seconds.  Before any
timing the results are compared item by item.  For MultiFastPitch also the frame-side attention launch alone (device
events).  Prints per-round times, medians and one JSON line per model and mode.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fastpitch_generate_batch import count_calls, timed  # noqa: E402
from forwardtacotron_amd import data, hip  # noqa: E402
from forwardtacotron_amd import fastpitch as FPM  # noqa: E402


def attention_alone(B, T, lens, d, nh, mode, reps=20):
    """the frame-side attention on its own: ft_attn_fwd_lens vs the masked route (no fused byte-mask kernel exists at
    these widths: _attn_unfused in both modes) -> (us, us), device events"""
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(B, T, 3 * d, generator=g).cuda()
    key_pad = (torch.arange(T, device='cuda')[None, :] >= lens[:, None]).to(torch.uint8).contiguous()
    scale = 1.0 / math.sqrt(d // nh)
    fns = (lambda: hip.attn_fwd_lens(qkv, lens, nh, scale),
           lambda: hip.mask_rows(FPM._attn_unfused(qkv, key_pad, nh, scale, 0.0, 0)[0], lens))
    out = []
    with hip.gemm_precision(mode):
        for fn in fns:
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


def build(kind):
    torch.manual_seed(0)
    if kind == 'mfp':
        from forwardtacotron_amd.multi_fastpitch import MultiFastPitch
        cfg = dict(data.MULTI_FASTPITCH_MODEL)
        model, scale = MultiFastPitch(**cfg), 3.0
    else:
        from forwardtacotron_amd.multi_model import MultiForwardTacotron
        cfg = dict(data.MULTISPEAKER_MODEL)
        model, scale = MultiForwardTacotron(**cfg), 30.0
    with torch.no_grad():
        model.dur_pred.lin.weight.mul_(scale)
        model.dur_pred.lin.bias.fill_(2.5)
    return cfg, model.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--models', default='mfp,mft')
    ap.add_argument('--modes', default='fp32,bf16', help='matmul modes of MultiFastPitch (MultiForwardTacotron is fp32)')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_multi_generate_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

    g = torch.Generator().manual_seed(a.seed)
    x_len = torch.randint(a.min_len, a.max_len + 1, (a.items,), generator=g)
    Tx = int(x_len.max())
    x = torch.zeros(a.items, Tx, dtype=torch.long)
    for b in range(a.items):
        x[b, :int(x_len[b])] = torch.randint(1, 135, (int(x_len[b]),), generator=g)
    xd = x.cuda()
    singles = [xd[b:b + 1, :int(x_len[b])].contiguous() for b in range(a.items)]

    for kind in a.models.split(','):
        cfg, model = build(kind)
        semb = torch.randn(a.items, cfg['speaker_emb_dims'], generator=g)
        semb = (semb / semb.norm(dim=1, keepdim=True)).cuda()
        rows = [semb[b:b + 1].contiguous() for b in range(a.items)]

        def call(switch):
            os.environ['FT_ATTN_LENS'] = switch
            try:
                return model.generate_batch(xd, x_len, semb)
            finally:
                os.environ.pop('FT_ATTN_LENS')

        arms = {'batch': lambda: call('1'), 'loop': lambda: [model.generate(s, r) for s, r in zip(singles, rows)]}
        if kind == 'mfp':
            arms['masked'] = lambda: call('0')
        for mode in (a.modes.split(',') if kind == 'mfp' else ['fp32']):
            model.matmul_dtype = mode
            print(f'==== {type(model).__name__}, matmul mode {mode} ====')
            res = {k: f() for k, f in arms.items()}
            torch.cuda.synchronize()
            ob, ol = res['batch'], res['loop']
            mel_len = ob['mel_len'].tolist()
            flips = [b for b in range(a.items) if ol[b]['mel'].shape[2] != mel_len[b]]
            if flips and mode == 'fp32':
                raise SystemExit(f'items {flips}: other frame counts in the batch than alone')
            worst = max([0.0] + [(ob['mel'][b, :, :mel_len[b]] - ol[b]['mel'][0]).abs().max().item()
                                 for b in range(a.items) if b not in flips])
            pc_same = all(ob['pitch_cond'][b, :int(x_len[b])].tolist() == ol[b]['pitch_cond'].reshape(-1).tolist()
                          for b in range(a.items))
            Tm = max(mel_len)
            pad_share = 1.0 - sum(mel_len) / (a.items * Tm)
            print(f'{a.items} items, x_len {int(x_len.min())}..{Tx} (sum {int(x_len.sum())}), frames {min(mel_len)}..{Tm} '
                  f'(sum {sum(mel_len)}, {100 * pad_share:.1f} % of the {a.items} x {Tm} packed rows are padding)')
            print(f'batch vs loop: max |diff| {worst:.3e}, pitch_cond equal {pc_same}, items with another frame count {flips}')
            if 'masked' in res and res['masked']['mel_len'].tolist() == mel_len:
                print(f'batch vs masked: max |diff| {(ob["mel"] - res["masked"]["mel"]).abs().max().item():.3e}')
            calls = {n: count_calls(f) for n, f in arms.items()}
            print('C-ABI calls per repetition: ' + ', '.join(f'{k} {v}' for k, v in calls.items()))
            w = {}
            for _ in range(max(1, a.warmup)):
                w = {k: timed(f) for k, f in arms.items()}
            reps = {k: max(1, math.ceil(a.window * 1e3 / v)) for k, v in w.items()}
            t = {k: [] for k in arms}
            for r in range(a.rounds):
                for k, f in arms.items():
                    t[k].append(timed(f, reps[k]))
                print(f'round {r}: ' + '   '.join(f'{k} {t[k][-1]:8.3f} ms' for k in arms))
            med = {k: statistics.median(v) for k, v in t.items()}
            line = 'median: ' + '   '.join(f'{k} {med[k]:.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})' for k in t) \
                + f'   loop / batch = {med["loop"] / med["batch"]:.2f}x'
            rec = {'model': type(model).__name__, 'mode': mode, 'items': a.items, 'frames': sum(mel_len), 'Tm': Tm,
                   'pad_share': round(pad_share, 4), 'rounds': a.rounds, 'calls': calls, 'max_abs_diff_vs_loop': worst,
                   **{f'{k}_ms_median': round(v, 3) for k, v in med.items()}}
            if kind == 'mfp':
                line += f'   masked / batch = {med["masked"] / med["batch"]:.3f}x'
                d, nh = cfg['d_model'] + cfg['speaker_emb_dims'], cfg['postnet_heads']
                att_new, att_old = attention_alone(a.items, Tm, ob['mel_len'], d, nh, mode)
                rec.update(attn_lens_us=round(att_new, 1), attn_masked_us=round(att_old, 1))
            print(line)
            if kind == 'mfp':
                print(f'frame-side attention alone [B {a.items}, T {Tm}, heads {nh}, hd {d // nh}]: ft_attn_fwd_lens '
                      f'{att_new:.1f} us, masked route + mask_rows {att_old:.1f} us')
            print(json.dumps(rec))


if __name__ == '__main__':
    main()
