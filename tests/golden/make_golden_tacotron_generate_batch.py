"""Golden fixture for tests/test_tacotron_generate_batch_cpu.py and tests/test_gpu_tacotron_generate_batch.py, generated
by IMPORTING the reference's models/tacotron.py (a checkout of it is needed), exactly as
make_golden_tacotron_generate.py does.  Every case builds the reference Tacotron under torch.manual_seed(seed), records
the layout and a SHA-256 of each tensor of that freshly initialised state_dict, gives every BatchNorm non-trivial running
statistics and records, PER ITEM, the reference's own Tacotron.generate of that sentence ALONE (eval mode, B = 1): what
generate_batch must give the item inside a ragged batch.  Weights are not stored.

Cases (tiny = make_golden_tacotron.TINY):
  s1    tiny, seed 4, mel_proj.weight * 30, r = 1, steps 48, lengths 1 5 9 12 7 3, ONE threshold for all items: three
        distinct mid-run stops within the first 32 steps, one in the second 32, two items that never stop
  s2    the same with seed 12, r = 2, steps 64: one item stops at the first eligible step (s = 6), one never
  t17   tiny, r = 3, steps 30, B = 17 (lengths cycling through 1..12), stop disabled: crosses the 16-item tile
  full  configs/singlespeaker.yaml sizes, seed 0, r = 2, steps 48, lengths 40 17 1, stop disabled (lstm_dims = 512)
  spk   tiny with speaker_emb_dim = 16, three items, three different speaker rows
Tokens: g = np.random.default_rng(77), then g.integers(1, 135, (1, L)) for each length in order.

The thresholds of s1 and s2 are derived here from a run with the stop disabled: among the midpoints between neighbouring
per-step maxima, the first one (ascending) that keeps every item's every eligible step (s * r > 10) up to the item's
stop at least MARGIN = 1e-3 away from the threshold -- ten times the GPU parity tolerance, so the stop steps are exact
there -- and gives the stop pattern named above.  The script fails loudly when there is none.

Output tacotron_generate_batch.npz, per case <c>/: cfg (JSON, stop_threshold included), r, seed, steps, sd_keys /
sd_shapes / sd_sha256, bn/<key>, mel_proj_scale (s1, s2), x [B,Tx] (zero past x_len), x_len, speaker_emb (spk), s_out [B],
and per item <c>/<b>/: mel_outputs, linear, attn_scores.

    python tests/golden/make_golden_tacotron_generate_batch.py <reference checkout>    (or FT_REFERENCE=<checkout>)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden_tacotron import FULL, TINY, bn_stats, sha256  # noqa: E402
import taco_gen_batch_cpu as GB  # noqa: E402

MARGIN = 1e-3
CASES = {
    's1': dict(cfg=TINY, seed=4, r=1, steps=48, lens=[1, 5, 9, 12, 7, 3], mel_proj_scale=30., stop='s1'),
    's2': dict(cfg=TINY, seed=12, r=2, steps=64, lens=[1, 5, 9, 12, 7, 3], mel_proj_scale=30., stop='s2'),
    't17': dict(cfg=TINY, seed=3, r=3, steps=30, lens=[1 + i % 12 for i in range(17)]),
    'full': dict(cfg=FULL, seed=0, r=2, steps=48, lens=[40, 17, 1]),
    'spk': dict(cfg=dict(TINY, speaker_emb_dim=16), seed=2, r=2, steps=30, lens=[4, 9, 6]),
}


def build(RefTacotron, cfg, c):
    torch.manual_seed(c['seed'])
    ref = RefTacotron(**cfg)
    ref.r = c['r']
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    stats = bn_stats(sd, 100 + c['seed'])
    ref.load_state_dict(stats, strict=False)
    if 'mel_proj_scale' in c:
        with torch.no_grad():
            ref.decoder.mel_proj.weight.mul_(c['mel_proj_scale'])
    return ref, sd, stats


def stops_of(maxes, thr, r):
    """per item: the first step s with s * r > 10 whose maximum is below thr, or None"""
    return [next((s for s, m in enumerate(ms) if s * r > 10 and m < thr), None) for ms in maxes]


def margins_ok(maxes, thr, stops, r):
    for ms, st in zip(maxes, stops):
        for s, m in enumerate(ms[:len(ms) if st is None else st + 1]):
            if s * r > 10 and abs(m - thr) < MARGIN:
                return False
    return True


def pattern_ok(kind, stops, r, S):
    """the stop pattern a case must have (module docstring); tests/test_tacotron_generate_batch_cpu.py re-asserts it"""
    first = 10 // r + 1
    hit = [s for s in stops if s is not None]
    if len(set(hit)) != len(hit) or any(s >= S - 1 for s in hit):
        return False
    if kind == 's1':
        return stops.count(None) == 2 and sum(first < s < 32 for s in hit) == 3 and sum(32 <= s for s in hit) == 1
    return stops.count(None) == 1 and hit.count(first) == 1 and len(hit) == 5


def pick_threshold(kind, maxes, r, S):
    vals = sorted({float(m) for ms in maxes for s, m in enumerate(ms) if s * r > 10})
    for lo, hi in zip(vals, vals[1:]):
        thr = float(np.float32(0.5 * (lo + hi)))
        stops = stops_of(maxes, thr, r)
        if margins_ok(maxes, thr, stops, r) and pattern_ok(kind, stops, r, S):
            return thr, stops
    raise SystemExit(f'{kind}: no threshold gives the stop pattern with a margin of {MARGIN}')


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    try:
        from models.tacotron import Tacotron as RefTacotron
    finally:
        sys.path.remove(ref_dir)
    out = {}
    for name, c in CASES.items():
        cfg = dict(c['cfg'])
        r, steps, lens = c['r'], c['steps'], c['lens']
        S = -(-steps // r)
        B, Tx = len(lens), max(lens)
        g = np.random.default_rng(77)
        x = np.zeros((B, Tx), np.int64)
        for b, n in enumerate(lens):
            x[b, :n] = g.integers(1, 135, (1, n))[0]
        semb = None
        if cfg['speaker_emb_dim'] > 0:
            semb = torch.from_numpy(g.normal(0., 1., (B, cfg['speaker_emb_dim'])).astype(np.float32))
        alone = lambda ref, b: ref.generate(torch.from_numpy(x[b:b + 1, :lens[b]]),
                                            None if semb is None else semb[b:b + 1], steps=steps)
        want = None
        if 'stop' in c:
            ref, _, _ = build(RefTacotron, dict(cfg, stop_threshold=-1e9), c)
            with torch.no_grad():
                maxes = [[float(m) for m in alone(ref, b)[0].reshape(80, S, r).max(axis=(0, 2))] for b in range(B)]
            thr, want = pick_threshold(c['stop'], maxes, r, S)
            assert margins_ok(maxes, thr, want, r) and pattern_ok(c['stop'], want, r, S)
            cfg['stop_threshold'] = thr
        else:
            cfg['stop_threshold'] = -1e9
        ref, sd, stats = build(RefTacotron, cfg, c)
        p = name + '/'
        out[p + 'cfg'] = np.array(json.dumps(cfg))
        out[p + 'r'], out[p + 'seed'], out[p + 'steps'] = np.array(r), np.array(c['seed']), np.array(steps)
        out[p + 'sd_keys'] = np.array(list(sd.keys()), dtype='S')
        out[p + 'sd_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()], dtype='S')
        out[p + 'sd_sha256'] = np.array([sha256(v) for v in sd.values()], dtype='S')
        for k, v in stats.items():
            out[p + 'bn/' + k] = v.numpy()
        if 'mel_proj_scale' in c:
            out[p + 'mel_proj_scale'] = np.array(c['mel_proj_scale'], np.float32)
        out[p + 'x'], out[p + 'x_len'] = x, np.array(lens, np.int64)
        if semb is not None:
            out[p + 'speaker_emb'] = semb.numpy()
        s_out = []
        with torch.no_grad():
            for b in range(B):
                mel, lin, attn = alone(ref, b)
                q = f'{p}{b}/'
                out[q + 'mel_outputs'], out[q + 'linear'], out[q + 'attn_scores'] = mel, lin, attn
                s_out.append(attn.shape[0])
        out[p + 's_out'] = np.array(s_out, np.int64)
        if want is not None:
            assert s_out == [S if s is None else s + 1 for s in want], (s_out, want)
        # the float64 batched, masked restatement agrees with every item alone
        P = {k: v.double() if v.is_floating_point() else v for k, v in ref.state_dict().items()}
        with torch.no_grad():
            got = GB.generate_batch(P, torch.from_numpy(x), torch.tensor(lens), cfg, r, steps, semb)
        assert got['steps_out'].tolist() == s_out, (name, got['steps_out'].tolist(), s_out)
        diff = 0.0
        for b in range(B):
            q, T, n = f'{p}{b}/', s_out[b] * r, lens[b]
            diff = max(diff, float(np.abs(got['mel'][b, :, :T].numpy() - out[q + 'mel_outputs']).max()),
                       float(np.abs(got['linear'][b, :, :T].numpy() - out[q + 'linear']).max()),
                       float(np.abs(got['attn'][b, :s_out[b], :n].numpy() - out[q + 'attn_scores']).max()))
        assert diff < 1e-5, (name, diff)
        print(name, 'B', B, 'Tx', Tx, 's_out', s_out, 'of', S, 'restatement diff %.2e' % diff, 'stop_threshold',
              cfg['stop_threshold'])
    path = os.path.join(HERE, 'tacotron_generate_batch.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ['FT_REFERENCE'])
