"""Fixture of FastPitch.generate_batch: tests/golden/fastpitch_generate_batch.npz.

Needs the reference checkout (FT_REFERENCE, as make_golden.py).  The tiny FastPitch config of make_golden_fastpitch.py
(all dropouts 0, conv1_kernel = 5) with every parameter moved off its init, the duration predictor's output layer
rescaled so that durations spread over roughly 0..6, a ragged batch of 5 sentences of non-zero tokens, and for every
sentence the reference's own generate() on that sentence ALONE -- what generate_batch has to reproduce per item.

The seed is searched until
  * at least one item takes the `fill_(2.)` fallback (fast_pitch.py:176-177) and at least one does not,
  * every valid dur_hat is at least MARGIN away from every integer (the fallback's truncation) and
  * from every half-integer (the LengthRegulator's rounding, common_layers.py:21),
so that a rounding flip can never hide behind the 5e-5 parity bar (MARGIN is 20x that bar), and the durations really
spread (SPREAD).  The `pe` buffers are stored truncated to PE_ROWS rows (helpers.fp_state rebuilds them).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden_fastpitch import PE_ROWS, TINY_FP, put_sd  # noqa: E402  (puts the reference checkout on sys.path)
from make_golden_generate_batch import margins  # noqa: E402
from models.fast_pitch import FastPitch  # noqa: E402

MARGIN = 1e-3
X_LEN = [7, 1, 4, 7, 2]
TX = 7
ALPHA = 0.9
DUR_SCALE, DUR_BIAS = 3.0, 2.5       # dur_pred.lin: weight *= DUR_SCALE, bias = DUR_BIAS
SPREAD = (0.5, 4.5)                  # the valid dur_hat reach below / above these (durations over roughly 0..6)


def build(seed: int):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    model = FastPitch(**TINY_FP)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        model.dur_pred.lin.weight.mul_(DUR_SCALE)
        model.dur_pred.lin.bias.fill_(DUR_BIAS)
    model.eval()
    x = torch.zeros(len(X_LEN), TX, dtype=torch.long)
    for b, L in enumerate(X_LEN):
        x[b, :L] = torch.randint(1, TINY_FP['num_chars'], (L,), generator=g)
    items, fallback, worst_int, worst_half, spread = [], [], 1.0, 1.0, []
    for b, L in enumerate(X_LEN):
        xb = x[b:b + 1, :L].clone()
        with torch.no_grad():
            raw = model.dur_pred(xb, alpha=ALPHA).squeeze(2)          # what generate() decides the fallback on
        fallback.append(bool(torch.sum(raw.long()) <= 0))
        mi, mh = margins(raw.numpy().astype(np.float64))
        worst_int, worst_half = min(worst_int, mi), min(worst_half, mh)
        spread += raw.flatten().tolist()
        out = model.generate(xb, alpha=ALPHA)
        out['dur_hat'] = raw
        items.append(out)
    ok = any(fallback) and not all(fallback) and worst_int >= MARGIN and worst_half >= MARGIN and \
        min(spread) < SPREAD[0] and max(spread) > SPREAD[1]
    return ok, model, x, items, fallback, (worst_int, worst_half, min(spread), max(spread))


def main():
    for seed in range(1000):
        ok, model, x, items, fallback, info = build(seed)
        if ok:
            break
    else:
        raise SystemExit('no seed satisfies the fixture conditions')
    assert any(fallback) and not all(fallback)
    assert info[0] >= MARGIN and info[1] >= MARGIN
    assert bool((x[torch.arange(TX)[None, :] < torch.tensor(X_LEN)[:, None]] != 0).all())
    out = {'x': x.numpy(), 'x_len': np.asarray(X_LEN, dtype=np.int64), 'alpha': np.float64(ALPHA),
           'fallback': np.asarray(fallback), 'seed': np.int64(seed), 'pe_rows': np.int64(PE_ROWS)}
    put_sd(out, 'sd/', model.state_dict())
    for b, o in enumerate(items):
        for k, v in o.items():
            out[f'item{b}/{k}'] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, 'fastpitch_generate_batch.npz'), **out)
    print(f'fastpitch_generate_batch.npz: seed {seed}, fallback {fallback}, margins int {info[0]:.2e} half {info[1]:.2e}, '
          f'dur_hat in [{info[2]:.2f}, {info[3]:.2f}], mel_len {[int(o["mel"].shape[2]) for o in items]}')


if __name__ == '__main__':
    main()
