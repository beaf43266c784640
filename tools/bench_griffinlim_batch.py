"""Batched Griffin-Lim against the loop of per-item calls it replaces.

    python tools/bench_griffinlim_batch.py [--items 32] [--min-len 20] [--max-len 128] [--n-iter 32] [--rounds 5]
                                           [--warmup 2] [--window 0.5]

The mels are those of tools/bench_generate_batch.py: the production single-speaker ForwardTacotron (default
initialisation, seed 0, duration predictor shifted so that a token lasts a few frames), one ragged batch of --items
sentences with x_len drawn from [--min-len, --max-len] under a fixed seed, synthesised by generate_batch.  Two ways to turn
them into audio on the same GPU, in one process:

  loop  : griffinlim(mel[b, :, :mel_len[b]], init_u=...) for every item (the initial phases already on the device: the
          host draw of griffinlim(seed=...) is timed once, separately)
  batch : one griffinlim_batch(mel, mel_len, seed=...)

Both are warmed up at the shapes they are timed at, then timed in alternation with a host clock around work that ends in
a device synchronise; a timed window holds as many back-to-back repetitions as fill --window seconds; times are per
repetition.  Before any timing, batch and loop are compared item by item on the same initial phases.  Then the batch's
GEMMs and its element-wise launches are replayed alone, back to back at the batch's shapes, for the split between the
two.  Prints launch counts, the share of wasted rows, medians and one JSON line.  Needs a GPU: there is no CPU fallback.
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
from forwardtacotron_amd.model import ForwardTacotron  # noqa: E402
from forwardtacotron_amd.vocoder import GriffinLim, gl_batch_geometry  # noqa: E402

DSP_CFG = dict(num_mels=80, sample_rate=22050, hop_length=256, win_length=1024, n_fft=1024, fmin=0, fmax=8000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=32)
    ap.add_argument('--min-len', type=int, default=20)
    ap.add_argument('--max-len', type=int, default=128)
    ap.add_argument('--n-iter', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=float, default=0.5, help='seconds of work per timed window')
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_griffinlim_batch: needs an MI355X (no CPU fallback, no time without a GPU)')

    cfg = dict(data.SINGLESPEAKER_MODEL)
    torch.manual_seed(0)
    model = ForwardTacotron(**cfg)
    with torch.no_grad():
        model.dur_pred.lin.weight.mul_(30.0)
        model.dur_pred.lin.bias.fill_(2.5)
    model = model.cuda().eval()
    g = torch.Generator().manual_seed(a.seed)
    x_len = torch.randint(a.min_len, a.max_len + 1, (a.items,), generator=g)
    x = torch.zeros(a.items, int(x_len.max()), dtype=torch.long)
    for b in range(a.items):
        x[b, :int(x_len[b])] = torch.randint(1, cfg['num_chars'], (int(x_len[b]),), generator=g)
    gen = model.generate_batch(x.cuda(), x_len)
    mel = gen['mel_post'].clamp(-11.5, 2.0).contiguous()             # an untrained model's "log-mel"
    mel_len = gen['mel_len'].cpu()
    lens = mel_len.tolist()
    B, _, Tmax = mel.shape
    del model, gen

    gl = GriffinLim(**DSP_CFG)
    geo = gl_batch_geometry(B, Tmax, gl.n_fft, gl.hop)
    Tcap, rows, Fp = geo['Tcap'], geo['rows'], gl.Fp
    wasted = 1.0 - sum(lens) / rows
    print(f'{B} items, x_len {int(x_len.min())}..{int(x_len.max())}, frames {min(lens)}..{max(lens)} (sum {sum(lens)}); '
          f'Tcap {Tcap}, {rows} packed rows, {100 * wasted:.1f} % of them past their item')

    # the same initial phases for both routes: drawn by the batch's generator, cut per item for the loop
    ml_dev = mel_len.cuda()
    _, u = hip.gl_init_ragged(torch.ones(rows, Fp, device='cuda'), ml_dev, B, Tcap, Tmax, seed=a.seed, want_u=True)
    singles = [mel[b, :, :lens[b]].contiguous() for b in range(B)]
    us = [u[b * Tcap:b * Tcap + lens[b]].contiguous() for b in range(B)]

    def batch():
        return gl.griffinlim_batch(mel, mel_len, n_iter=a.n_iter, seed=a.seed)

    def loop():
        return [gl.griffinlim(singles[b], n_iter=a.n_iter, init_u=us[b]) for b in range(B)]

    def loop_seed():
        return [gl.griffinlim(singles[b], n_iter=a.n_iter, seed=a.seed) for b in range(B)]

    c0 = sum(hip.gemm_variant_counts().values())
    ob = batch()
    c1 = sum(hip.gemm_variant_counts().values())
    ol = loop()
    c2 = sum(hip.gemm_variant_counts().values())
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(B):
        n = gl.hop * (lens[b] - 1)
        assert ol[b].numel() == n and int(ob['wav_len'][b]) == n
        if n:
            worst = max(worst, float((ob['wav'][b, :n] - ol[b]).abs().max() / ol[b].abs().max().clamp_min(1.0)))
    # launches: GEMMs are counted by the library; the element-wise ones follow from the call structure
    ew_batch = 2 + 2 * gl.nnls_iter + 1 + 2 * a.n_iter + 1
    ew_loop = B * (1 + 2 * gl.nnls_iter + 1 + 2 * a.n_iter + 1 + 1)            # + the clone of the result
    print(f'batch vs loop after {a.n_iter} iterations: max |diff| / max(1, |wav|) {worst:.3e}')
    print(f'launches: batch {c1 - c0} GEMMs + {ew_batch} element-wise; loop {c2 - c1} GEMMs + {ew_loop} element-wise')

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
    print(f'window {a.window} s: {nb} griffinlim_batch calls, {nl} passes over the loop')
    tb, tl = [], []
    for r in range(a.rounds):
        tb.append(timed(batch, nb))
        tl.append(timed(loop, nl))
        print(f'round {r}: batch {tb[-1]:9.3f} ms   loop {tl[-1]:9.3f} ms')
    mb, ml = statistics.median(tb), statistics.median(tl)
    t_seed = timed(loop_seed)
    print(f'median: batch {mb:.3f} ms (min {min(tb):.3f}, max {max(tb):.3f})   loop {ml:.3f} ms (min {min(tl):.3f}, '
          f'max {max(tl):.3f})   loop / batch = {ml / mb:.2f}x   (loop with the host draw of seed=: {t_seed:.3f} ms, once)')

    # the split: the batch's GEMMs alone and its element-wise launches alone, back to back at the batch's shapes
    S = gl.mel_to_stft_batch(mel, mel_len)
    M = hip.gl_exp_transpose_ragged(mel, ml_dev, Tcap)
    proj = hip.gl_init_ragged(S, ml_dev, B, Tcap, Tmax, seed=a.seed)
    tprev = torch.zeros_like(proj)
    frames = hip.linear_fwd_as(proj, 2 * Fp, gl.w_inv, rows, 2 * Fp)
    w2 = gl.w2
    ypad = hip.overlap_add_ragged(frames, w2, ml_dev, B, Tcap, Tmax, gl.n_fft, gl.hop)
    rebuilt = hip.linear_fwd_as(ypad, gl.hop, gl.w_fwd, rows, gl.n_fft)
    R = hip.linear_fwd_as(S, Fp, gl.mel_basis, rows, Fp)
    G = hip.linear_fwd_as(R, gl.n_mels, gl.mel_basis_t, rows, gl.n_mels)
    X = S.clone()
    st = hip._stream()

    def gemms_dft():
        for _ in range(a.n_iter):
            hip.linear_fwd_as(proj, 2 * Fp, gl.w_inv, rows, 2 * Fp)
            hip.linear_fwd_as(ypad, gl.hop, gl.w_fwd, rows, gl.n_fft)
        hip.linear_fwd_as(proj, 2 * Fp, gl.w_inv, rows, 2 * Fp)

    def gemms_nnls():
        hip.linear_fwd_as(M, gl.n_mels, gl.mel_pinv, rows, gl.n_mels)
        for _ in range(gl.nnls_iter):
            hip.linear_fwd_as(S, Fp, gl.mel_basis, rows, Fp)
            hip.linear_fwd_as(R, gl.n_mels, gl.mel_basis_t, rows, gl.n_mels)

    def elementwise():
        hip.gl_exp_transpose_ragged(mel, ml_dev, Tcap)
        hip.gl_relu(X)
        for _ in range(gl.nnls_iter):
            _lib.call('ft_sub', R.data_ptr(), M.data_ptr(), R.data_ptr(), R.numel(), st)
            _lib.call('ft_nnls_step', X.data_ptr(), G.data_ptr(), gl.inv_lip, X.numel(), st)
        hip.gl_init_ragged(S, ml_dev, B, Tcap, Tmax, seed=a.seed)
        for it in range(a.n_iter):
            hip.overlap_add_ragged(frames, w2, ml_dev, B, Tcap, Tmax, gl.n_fft, gl.hop)
            hip.gl_phase_ragged(rebuilt, tprev, S, ml_dev, proj, B, Tcap, Tmax, 0.5, it > 0)
        hip.overlap_add_ragged(frames, w2, ml_dev, B, Tcap, Tmax, gl.n_fft, gl.hop, as_wav=True)

    parts = {}
    for name, fn in (('gemm_dft', gemms_dft), ('gemm_nnls', gemms_nnls), ('elementwise', elementwise)):
        timed(fn)
        reps = max(1, math.ceil(a.window * 1e3 / max(timed(fn), 1e-3)))
        parts[name] = statistics.median(timed(fn, reps) for _ in range(3))
    print('replayed alone: ' + ', '.join(f'{k} {v:.3f} ms' for k, v in parts.items())
          + f'   (sum {sum(parts.values()):.3f} ms against {mb:.3f} ms for the call)')
    print(json.dumps({'items': B, 'frames': sum(lens), 'Tmax': Tmax, 'Tcap': Tcap, 'rows': rows,
                      'wasted_row_share': round(wasted, 4), 'n_iter': a.n_iter, 'nnls_iter': gl.nnls_iter,
                      'batch_ms_median': round(mb, 3), 'loop_ms_median': round(ml, 3), 'loop_seed_ms': round(t_seed, 3),
                      'launches_batch': [c1 - c0, ew_batch], 'launches_loop': [c2 - c1, ew_loop],
                      'split_ms': {k: round(v, 3) for k, v in parts.items()}, 'rounds': a.rounds,
                      'calls_per_window': [nb, nl], 'max_rel_diff': worst}))


if __name__ == '__main__':
    main()
