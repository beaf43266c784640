"""HiFiGAN.inference_batch on the mels of a ragged synthesis batch, against the same generator in stock fp32 torch.

    python tools/bench_hifigan_batch.py [--preset v1] [--items 32] [--min-len 20] [--max-len 128] [--rounds 8] [--warmup 2]
                                        [--window 0.5]

The sentences, the acoustic model and its generate_batch call are those of tools/bench_melgan_batch.py; its 'mel_post'
and 'mel_len' go into a HiFi-GAN of the preset (default initialisation, seed 0).  Three ways to turn them into audio on
the same GPU, in the same process, timed in alternating rounds (ours, per-item, padded, ours, ...):

  ours     : one HiFiGAN.inference_batch(mel_post, mel_len) call
  per-item : the restatement of tests/hifigan_cpu.py (stock nn.Conv1d / nn.ConvTranspose1d, weight norm removed as the
             published inference script does) called once per item on mel[b:b+1, :, :mel_len[b]]
  padded   : that generator called ONCE on the padded batch (items shorter than Tmax get wrong samples near their end:
             a speed reference only)

Each is warmed up at the shapes it is timed at; a timed window holds as many back-to-back repetitions as fill --window
seconds and ends in one device synchronise; times are per repetition.  Before any timing, ours is compared with the
per-item stock result item by item.  Then
  * the A/B of ResBlock1's pair: per stage width that has the fused kernel and per (k, d), the fused launch against the
    two launches of the residual convolution, on the stage's real input, in alternating windows;
  * the per-stage split of ours: device events around every launch of one call (median over --rounds calls), summed per
    stage, with the FLOP counted from the items' own lengths.
Prints everything and one JSON line.  Needs a GPU: there is no CPU fallback.

    python tools/bench_hifigan_batch.py --fp16-ab [--preset v1] [--rounds 8] [--window 0.5]

times HiFiGAN.matmul_dtype = 'fp16' against 'fp32' instead: ONE module, the mode switched between alternating windows
(fp32, fp16, fp32 again -- fp32 is measured twice, and the distance between its slowest and its fastest window is the
margin below which a difference between the modes means nothing), then the per-stage split of one call per mode, and max |wav_fp16 - wav_fp32|
with the signal-to-noise ratio of the fp16 wav against the fp32 wav over the valid samples of the batch.
profiles/hifigan_fp16.txt is this output.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import hifigan_cpu as R  # noqa: E402
from forwardtacotron_amd import data, hip  # noqa: E402
from forwardtacotron_amd import hifigan as M  # noqa: E402
from forwardtacotron_amd.model import ForwardTacotron  # noqa: E402


def stock_generator(voc, cfg):
    ref = R.RefGenerator(**cfg)
    ref.load_state_dict(voc.state_dict())
    for m in ref.modules():
        if hasattr(m, 'weight_g'):
            torch.nn.utils.remove_weight_norm(m)
    return ref.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--preset', default='v1', choices=['v1', 'v2', 'v3'])
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--fp16-ab', action='store_true', help="time matmul_dtype 'fp16' against 'fp32' (twice) and stop")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hifigan_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

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
    vcfg = {'v1': R.V1, 'v2': R.V2, 'v3': R.V3}[a.preset]
    torch.manual_seed(0)
    voc = M.HiFiGAN(**vcfg)
    stock = stock_generator(voc, vcfg)
    voc = voc.cuda().eval()
    with torch.no_grad():
        gen = model.generate_batch(x.cuda(), x_len)
    torch.cuda.synchronize()
    hip.check_rnn_status()
    mel, mel_len_d = gen['mel_post'], gen['mel_len']
    mel_len = mel_len_d.tolist()
    mel_len_h = torch.tensor(mel_len, dtype=torch.int64)
    B, n_mels, Tmax = mel.shape
    hop = voc.hop_length
    frames = sum(mel_len)
    singles = [mel[b:b + 1, :, :n].contiguous() for b, n in enumerate(mel_len)]

    def ours():
        return voc.inference_batch(mel, mel_len_h)

    def quant(audio):
        return (M.MAX_WAV_VALUE * audio).clamp(min=-M.MAX_WAV_VALUE, max=M.MAX_WAV_VALUE - 1).short()

    def per_item():
        return [quant(stock(s).squeeze()) for s in singles]

    def padded():
        return quant(stock(mel).squeeze(1))

    def timed(fn, reps=1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / reps

    def alternate(fns, rounds, show=True, window=None):
        window = a.window if window is None else window
        w = {}
        for _ in range(max(1, a.warmup)):
            for k, fn in fns.items():
                w[k] = timed(fn)
        reps = {k: max(1, math.ceil(window * 1e3 / w[k])) for k in fns}
        t = {k: [] for k in fns}
        for r in range(rounds):
            for k, fn in fns.items():
                t[k].append(timed(fn, reps[k]))
            if show:
                print(f'round {r}: ' + '   '.join(f'{k} {t[k][-1]:9.3f} ms' for k in fns))
        return t, reps

    # ---- the per-stage split: device events around every launch of one call -------------------------------------------
    names = ('hifigan_conv_in', 'hifigan_upsample', 'hifigan_resconv', 'hifigan_resconv_h16', 'hifigan_respair',
             'hifigan_conv_out')

    def stage_split(call, ref_ms):
        """-> (rows, launches' total ms): `call` run a.rounds times with device events around every launch"""
        real = {n: getattr(hip, n) for n in names}
        marks = []

        def wrap(name, fn):
            def run(*args, **kw):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(*args, **kw)
                e1.record()
                if name == 'hifigan_conv_in':
                    key, flop = 'conv_in', frames * 2 * 7 * n_mels * args[4]
                elif name == 'hifigan_upsample':
                    cin, cout, sc, s = args[0].shape[1], args[8], args[4], args[5]
                    key, flop = f'upsample x{sc * s} {cin}->{cout}', frames * sc * s * 2 * 2 * cin * cout
                elif name == 'hifigan_conv_out':
                    key, flop = 'conv_out', frames * args[4] * 2 * 7 * args[0].shape[1]
                else:
                    C, sc = args[0].shape[1], args[4]
                    k = args[6].shape[0]
                    key = f'residual x{sc} C{C}'
                    flop = frames * sc * 2 * k * C * C * (2 if name == 'hifigan_respair' else 1)
                marks.append((key, flop, e0, e1))
                return out
            return run
        for n in names:
            setattr(hip, n, wrap(n, real[n]))
        per_call = []
        with torch.no_grad():
            for _ in range(a.rounds):
                marks.clear()
                call()
                torch.cuda.synchronize()
                per_call.append([(key, flop, e0.elapsed_time(e1)) for key, flop, e0, e1 in marks])
        for n in names:
            setattr(hip, n, real[n])
        keys = []
        for key, _, _ in per_call[0]:
            if key not in keys:
                keys.append(key)
        print(f'per-stage split (median of {a.rounds} calls, device events around each launch; {len(per_call[0])} launches):')
        print(f'  {"stage":26s} {"launches":>8s} {"ms":>8s} {"GFLOP":>8s} {"TFLOP/s":>8s}')
        rows, total, total_ms = [], 0, 0.0
        for key in keys:
            ms = statistics.median(sum(t_ for k_, _, t_ in c if k_ == key) for c in per_call)
            flop = sum(f_ for k_, f_, _ in per_call[0] if k_ == key)
            n = sum(1 for k_, _, _ in per_call[0] if k_ == key)
            total, total_ms = total + flop, total_ms + ms
            rows.append({'stage': key, 'launches': n, 'ms': round(ms, 4), 'gflop': round(flop / 1e9, 3)})
            print(f'  {key:26s} {n:8d} {ms:8.3f} {flop / 1e9:8.2f} {flop / ms / 1e9:8.1f}')
        print(f'  sum of the launches {total_ms:.3f} ms; total {total / 1e9:.1f} GFLOP ({total / frames / 1e9:.3f} per frame): '
              f'{total / ref_ms / 1e9:.1f} TFLOP/s over the whole call')
        return rows, total

    def in_mode(mode):
        def run():
            voc.matmul_dtype = mode
            return voc.inference_batch(mel, mel_len_h)
        return run

    if a.fp16_ab:
        with torch.no_grad():
            w32, w16 = in_mode('fp32')()['wav'], in_mode('fp16')()['wav']
            torch.cuda.synchronize()
            valid = torch.cat([(w16[b, :hop * n] - w32[b, :hop * n]).double() for b, n in enumerate(mel_len)])
            sig = torch.cat([w32[b, :hop * n].double() for b, n in enumerate(mel_len)])
            diff = float(valid.abs().max())
            snr = 10 * math.log10(float(sig.pow(2).sum() / valid.pow(2).sum()))
            print(f"{a.preset}: {B} items, frames {min(mel_len)}..{max(mel_len)} (sum {frames}), Tmax {Tmax}; matmul_dtype "
                  f"'fp16' against 'fp32': max |wav_fp16 - wav_fp32| {diff:.3e} (max |wav_fp32| {float(sig.abs().max()):.3e}, "
                  f'rms {float(sig.pow(2).mean().sqrt()):.3e}), SNR {snr:.1f} dB')
            t, reps = alternate({'fp32': in_mode('fp32'), 'fp16': in_mode('fp16'), 'fp32 again': in_mode('fp32')}, a.rounds)
        print(f'window {a.window} s: repetitions {reps}')
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in t:
            print(f'{k:10s} median {med[k]:9.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})')
        both = t['fp32'] + t['fp32 again']
        spread = max(both) - min(both)                      # of every fp32 window, first and second set
        gain = min(med['fp32'], med['fp32 again']) - med['fp16']
        print(f"fp32 / fp16 = {min(med['fp32'], med['fp32 again']) / med['fp16']:.3f}x; fp32's own spread {spread:.3f} ms, fp16 is "
              f"{gain:+.3f} ms ahead: {'faster beyond the spread' if gain > spread else 'NOT faster beyond the spread'}")
        splits = {}
        for mode in ('fp32', 'fp16'):
            print(f"matmul_dtype = '{mode}':")
            splits[mode], _ = stage_split(in_mode(mode), med[mode])
        voc.matmul_dtype = 'fp32'
        print(json.dumps({'preset': a.preset, 'items': B, 'frames': frames, 'Tmax': Tmax, 'rounds': a.rounds,
                          'repetitions': reps, 'fp32_ms_median': round(med['fp32'], 3), 'fp16_ms_median': round(med['fp16'], 3),
                          'fp32_again_ms_median': round(med['fp32 again'], 3), 'max_wav_diff': diff, 'snr_db': round(snr, 2),
                          'split': splits}))
        return

    with torch.no_grad():
        oo, ol = ours(), per_item()
        torch.cuda.synchronize()
        worst = max(int((oo['wav_int16'][b, :hop * n].int() - ol[b].int()).abs().max()) for b, n in enumerate(mel_len))
        wf = max(float((oo['wav'][b, :hop * n] - stock(s).squeeze()).abs().max()) for (b, n), s in zip(enumerate(mel_len), singles))
        print(f'{a.preset}: {B} items, frames {min(mel_len)}..{max(mel_len)} (sum {frames}), Tmax {Tmax}; ours vs stock per '
              f'item: max |int16 diff| {worst}, max |wav diff| {wf:.2e}')

        t, reps = alternate({'ours': ours, 'per-item': per_item, 'padded': padded}, a.rounds)
        print(f'window {a.window} s: repetitions {reps}')
        med = {k: statistics.median(v) for k, v in t.items()}
        for k in t:
            print(f'{k:9s} median {med[k]:9.3f} ms (min {min(t[k]):.3f}, max {max(t[k]):.3f})')
        print(f"per-item / ours = {med['per-item'] / med['ours']:.2f}x   padded / ours = {med['padded'] / med['ours']:.2f}x")

        # ---- A/B of ResBlock1's pair: one fused launch against two launches of the residual convolution ----------------
        ab = []
        if voc.resblock == '1':
            stages = voc.inference_batch(mel, mel_len_h, keep_stages=True)['stages']
            nk = len(voc.resblock_kernel_sizes)
            scale = 1
            print('pair A/B (ms per pair over the whole batch, median of alternating windows; plan = what the model runs):')
            for i, u in enumerate(voc.upsample_rates):
                scale *= u
                xd = stages[2 * i + 1]
                C = xd.shape[1]
                if not hip.hifigan_tile_rows('respair', C):
                    print(f'  C {C:3d}: no fused kernel at this width (two launches)')
                    continue
                out, midb = torch.empty_like(xd), torch.empty_like(xd)
                for j, (k, ds) in enumerate(zip(voc.resblock_kernel_sizes, voc.resblock_dilation_sizes)):
                    blk = voc.resblocks[i * nk + j]
                    for m, d in enumerate(ds):
                        w1, b1 = voc._panel(blk.convs1[m])
                        w2, b2 = voc._panel(blk.convs2[m])
                        args = (xd, mel_len_d, B, Tmax, scale)

                        def fused():
                            hip.hifigan_respair(*args, d, w1, b1, w2, b2, out=out)

                        def two():
                            hip.hifigan_resconv(*args, d, w1, b1, out=midb)
                            hip.hifigan_resconv(midb, mel_len_d, B, Tmax, scale, 1, w2, b2, res=xd, out=out)
                        tt, _ = alternate({'fused': fused, 'two': two}, max(3, a.rounds // 2), show=False, window=a.window / 5)
                        f, s2 = statistics.median(tt['fused']), statistics.median(tt['two'])
                        flop = frames * scale * 2 * 2 * k * C * C
                        plan = 'fused' if M.pair_is_fused(C, k, d) else 'two'
                        ab.append({'C': C, 'k': k, 'd': d, 'fused_ms': round(f, 4), 'two_ms': round(s2, 4), 'plan': plan})
                        print(f'  C {C:3d} k {k:2d} d {d}: fused {f:7.4f} ({flop / f / 1e9:6.1f} TFLOP/s)   two {s2:7.4f} '
                              f'({flop / s2 / 1e9:6.1f} TFLOP/s)   fused / two {f / s2:.2f}   plan {plan}'
                              f'{"" if (f <= s2) == (plan == "fused") else "   <-- plan is not the winner"}')

    rows, total = stage_split(ours, med['ours'])
    print(json.dumps({'preset': a.preset, 'items': B, 'frames': frames, 'Tmax': Tmax, 'ours_ms_median': round(med['ours'], 3),
                      'stock_per_item_ms_median': round(med['per-item'], 3), 'stock_padded_ms_median': round(med['padded'], 3),
                      'rounds': a.rounds, 'repetitions': reps, 'max_int16_diff': worst, 'max_wav_diff': wf,
                      'gflop': round(total / 1e9, 1), 'pair_ab': ab, 'split': rows}))


if __name__ == '__main__':
    main()
