"""Tacotron teacher training: forward_train + backward on an LJSpeech-shaped batch, one JSON line per r.

    python tools/bench_taco_train.py [--batch 32] [--rounds 10] [--warmup 2] [--seed 0] [--r 1 2] [--no-torch]

A seed-0 full-size singlespeaker model in train() over a seeded batch of B items with Tx ~ U[120, 180] tokens and
Tm ~ U[700, 900] frames, loss l1_loss(m1, mel) + l1_loss(m2, mel) as trainer/taco_trainer.py:96-98.  Per r:
  forward_ms, backward_ms, step_ms    HIP events, mean over --rounds after --warmup (step = forward + loss + backward)
  attend_bwd_ms                       ft_taco_attend_bwd alone on the step's own operands; attend_bwd_us_per_step = / S
  attend_bwd_launches_per_step        5 (softmax, energy, conv, GRU, carry)
  lstm_zone_fwd_us_per_step / lstm_zone_bwd_us_per_step    one residual LSTMCell, one launch per step each
  torch_fp32_step_ms                  the yardstick: autograd through the tests' stock-torch restatement
                                      (tests/taco_train_cpu.py, per-step Python loop) in fp32 on the same GPU, same masks
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd.tacotron import Tacotron, l1_loss  # noqa: E402

SINGLESPEAKER = dict(embed_dims=256, num_chars=135, encoder_dims=128, decoder_dims=256, n_mels=80, postnet_dims=128,
                     encoder_k=16, lstm_dims=512, postnet_k=8, num_highways=4, dropout=0.5, stop_threshold=-11.,
                     speaker_emb_dim=0)


def make_batch(B, seed, r, n_mels=80):
    rng = np.random.default_rng(seed)
    x_len = rng.integers(120, 181, B)
    mel_len = rng.integers(700, 901, B)
    Tx, Tm = int(x_len.max()), int(mel_len.max()) + 1
    Tm += (r - Tm % r) % r
    mel = np.full((B, n_mels, Tm), -11.5129, np.float32)
    x = np.zeros((B, Tx), np.int64)
    for b in range(B):
        mel[b, :, :mel_len[b]] = rng.normal(-6., 3., (n_mels, int(mel_len[b])))
        x[b, :x_len[b]] = rng.integers(1, 60, int(x_len[b]))
    return {'x': torch.from_numpy(x).cuda(), 'mel': torch.from_numpy(mel).cuda()}


def events(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(rounds):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / rounds


def run(r, a):
    torch.manual_seed(0)
    model = Tacotron(**SINGLESPEAKER).cuda().train()
    model.r = r
    batch = make_batch(a.batch, a.seed, r)
    B, Tx = batch['x'].shape
    S = math.ceil(batch['mel'].shape[2] / r)
    out = dict(metric='tacotron_train', r=r, batch=B, Tx=Tx, frames=int(batch['mel'].shape[2]), decoder_steps=S)

    def step():
        model.zero_grad(set_to_none=True)
        m1, m2, _ = model.forward_train(batch)
        (l1_loss(m1, batch['mel']) + l1_loss(m2, batch['mel'])).backward()

    out['step_ms'] = events(step, a.rounds, a.warmup)
    out['forward_ms'] = events(lambda: model.forward_train(batch), a.rounds, 1)
    out['backward_ms'] = out['step_ms'] - out['forward_ms']

    # the two recurrences' backward alone, on operands of the step's shapes
    dec = model.decoder
    gru, lsa = dec.attn_rnn, dec.attn_net
    with torch.no_grad():
        f = lambda *s: torch.randn(*s, device='cuda') * 0.1
        ep, epq, P = f(B, Tx, 256), f(B, Tx, 256), f(S, B, 768)
        attn, hist = model._attend(ep, epq, P, True)
        dhist = f(S, B, 512)
        args = (ep, epq, P, gru.weight_ih, gru.weight_hh, gru.bias_hh, lsa.W.weight, lsa.W.bias, lsa.conv.weight,
                lsa.L.weight, lsa.L.bias, lsa.v.weight, hist, attn, dhist)
        out['attend_bwd_ms'] = events(lambda: H.taco_attend_bwd(*args), a.rounds, 1)
        out['attend_bwd_us_per_step'] = out['attend_bwd_ms'] * 1e3 / S
        out['attend_bwd_launches_per_step'] = 5
        Ld = model.lstm_dims
        cell = dec.res_rnn1
        xp, dout = f(S, B, 4 * Ld), f(S, B, Ld)
        seed = (1 << 40) + 12345
        gates, c, _ = H.taco_lstm_zone_fwd(xp, cell.weight_hh, cell.bias_hh, 0.1, seed)
        whhT = H.transpose2d(cell.weight_hh)
        out['lstm_zone_fwd_us_per_step'] = events(
            lambda: H.taco_lstm_zone_fwd(xp, cell.weight_hh, cell.bias_hh, 0.1, seed), a.rounds, 1) * 1e3 / S
        out['lstm_zone_bwd_us_per_step'] = events(
            lambda: H.taco_lstm_zone_bwd(dout, gates, c, whhT, 0.1, seed), a.rounds, 1) * 1e3 / S

    if not a.no_torch:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import taco_train_cpu as TT
        cfg = dict(SINGLESPEAKER)
        shapes = TT.site_shapes(cfg, B, Tx, S, r, cfg['lstm_dims'], cfg['postnet_dims'])
        masks = {k: v.float().cuda() for k, v in TT.masks_from_seeds(model.last_seeds, model._site_p(), shapes).items()}
        P32 = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() and v.dim() > 0 and
                   'running_' not in k else v.detach().clone()) for k, v in model.state_dict().items()}

        def torch_step():
            m1, m2, _, _ = TT.forward(P32, batch, cfg, r, masks)
            loss = torch.nn.functional.l1_loss(m1, batch['mel']) + torch.nn.functional.l1_loss(m2, batch['mel'])
            torch.autograd.grad(loss, [v for v in P32.values() if v.requires_grad], allow_unused=True)

        out['torch_fp32_step_ms'] = events(torch_step, 1, 1)
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--r', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--no-torch', action='store_true', help='skip the stock-torch fp32 yardstick')
    a = ap.parse_args()
    for r in a.r:
        print(json.dumps(run(r, a)), flush=True)


if __name__ == '__main__':
    main()
