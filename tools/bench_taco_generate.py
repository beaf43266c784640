"""Autoregressive Tacotron.generate at full size: prints one JSON line.

    python tools/bench_taco_generate.py [--tx 150] [--steps 1000] [--iters 5] [--warmup 2] [--no-torch]

A seed-0 full-size singlespeaker model (configs/singlespeaker.yaml, r = 1) generates from a seeded Tx-token input with
the stop disabled (stop_threshold = -1e9), so every call runs all S = steps decoder steps.  Reported:
  ms_per_call             Tacotron.generate end to end (HIP events, mean over --iters after --warmup): encoder, the
                          decoder steps, the postnet and the copies of the numpy outputs
  us_per_step             marginal device time per decoder step: (time at steps - time at steps/2) / (steps/2)
  host_enqueue_us_per_step  host time spent in the ft_taco_gen_steps calls (they only enqueue), per step; well below
                          us_per_step means the step is device-bound
  launches_per_step       kernel launches per decoder step of ft_taco_gen_steps
  stop_step / steps_run / steps_wasted   a run with stop_threshold = +1e3 (stops at the first eligible step): the
                          steps already enqueued past the stop when S_out was read back (GEN_CHUNK = gen_chunk)
  torch_fp32_*            the float restatement of the tests (tests/taco_gen_cpu.py, stock torch ops, the
                          reference's per-step stop test and host sync) in fp32 on the same GPU (--no-torch skips it)
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

from forwardtacotron_amd import _lib  # noqa: E402
from forwardtacotron_amd import tacotron as T  # noqa: E402

# configs/singlespeaker.yaml, tacotron.model
SINGLESPEAKER = dict(embed_dims=256, num_chars=135, encoder_dims=128, decoder_dims=256, n_mels=80, postnet_dims=128,
                     encoder_k=16, lstm_dims=512, postnet_k=8, num_highways=4, dropout=0.5, stop_threshold=-11.,
                     speaker_emb_dim=0)
LAUNCHES_PER_STEP = 8        # csrc/ft_taco.hip, ft_taco_gen_steps


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tx', type=int, default=150)
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-torch', action='store_true', help='skip the stock-torch fp32 comparison')
    a = ap.parse_args()
    torch.manual_seed(0)
    m = T.Tacotron(**SINGLESPEAKER).cuda()
    m.stop_threshold.fill_(-1e9)
    x = torch.from_numpy(np.random.default_rng(0).integers(1, 135, (1, a.tx))).cuda()
    out = dict(tx=a.tx, steps=a.steps, r=1, lstm_dims=512, gen_chunk=T.GEN_CHUNK, launches_per_step=LAUNCHES_PER_STEP)
    with torch.no_grad():
        full = timed(lambda: m.generate(x, steps=a.steps), a.iters, a.warmup)
        half = timed(lambda: m.generate(x, steps=a.steps // 2), a.iters, a.warmup)
        out['ms_per_call'] = round(full, 3)
        out['us_per_step'] = round(1e3 * (full - half) / (a.steps - a.steps // 2), 2)

        # host time inside the enqueue-only step entry
        spent = [0.0]
        real_call = _lib.call

        def counting(name, *args):
            t = time.perf_counter()
            real_call(name, *args)
            if name == 'ft_taco_gen_steps':
                spent[0] += time.perf_counter() - t

        T._lib.call = counting
        try:
            m.generate(x, steps=a.steps)
        finally:
            T._lib.call = real_call
        out['host_enqueue_us_per_step'] = round(1e6 * spent[0] / a.steps, 2)
        out['bound'] = 'device' if out['host_enqueue_us_per_step'] < 0.8 * out['us_per_step'] else 'host'

        m.stop_threshold.fill_(1e3)
        _, _, attn = m.generate(x, steps=a.steps)
        out['stop_step'] = int(attn.shape[0])
        out['steps_run'] = int(m._gen_steps_run)
        out['steps_wasted'] = out['steps_run'] - out['stop_step']
        m.stop_threshold.fill_(-1e9)

        if not a.no_torch:
            sys.path.insert(0, os.path.join(ROOT, 'tests'))
            import taco_gen_cpu
            m.eval()
            P32 = {k: v.detach() for k, v in m.state_dict().items()}
            cfg = dict(SINGLESPEAKER, stop_threshold=-1e9)
            t = timed(lambda: taco_gen_cpu.generate(P32, x, cfg, 1, a.steps), 1, 1)
            out['torch_fp32_ms_per_call'] = round(t, 3)
            out['torch_fp32_us_per_step'] = round(1e3 * t / a.steps, 2)
            out['speedup_vs_torch_fp32'] = round(t / full, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
