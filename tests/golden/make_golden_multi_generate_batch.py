"""Fixture of MultiForwardTacotron.generate_batch: tests/golden/multi_generate_batch.npz.

Needs the reference checkout (FT_REFERENCE, as make_golden.py).  The tiny multispeaker config with every parameter moved
off its init (randomize_bn + 0.1 randn), the duration predictor's output layer rescaled, a ragged batch of 5 sentences of
non-zero tokens (no 1-token sentence: the reference's generate() raises on one), five DIFFERENT unit-norm speaker rows,
and for every sentence the reference's own generate() on that sentence alone with its own speaker row -- what
generate_batch has to reproduce per item -- plus its raw dur_hat and its pitch_cond logits.

The seed is searched until
  * at least one item takes the `fill_(2.)` fallback (multi_forward_tacotron.py:254-255) and at least one does not,
  * every valid dur_hat is at least MARGIN away from every integer and every half-integer (make_golden_generate_batch.py),
  * the top two pitch_cond logits of every valid token differ by at least MARGIN, so that an argmax flip cannot hide
    behind the 5e-5 parity bar either (MARGIN is 20x that bar), and at least two classes occur,
  * the durations really spread (SPREAD).
make_golden_multi_fastpitch_generate_batch.py builds the MultiFastPitch twin with the functions of this file.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import TINY_MULTI, randomize_bn  # noqa: E402  (puts the reference checkout, FT_REFERENCE, on sys.path)
from make_golden_generate_batch import margins  # noqa: E402

MARGIN = 1e-3
X_LEN = [7, 2, 4, 7, 3]
TX = 7
ALPHA = 0.9
DUR_SCALE, DUR_BIAS = 20.0, 0.8      # dur_pred.lin: weight *= DUR_SCALE, bias = DUR_BIAS (a higher bias leaves no fallback item)
SPREAD = (0.5, 4.5)                  # the valid dur_hat reach below / above these


def logit_margin(logits: np.ndarray) -> float:
    """smallest gap between the two largest logits of a token, logits [..., K]"""
    s = np.sort(logits.astype(np.float64), axis=-1)
    return float((s[..., -1] - s[..., -2]).min())


def build(seed: int, make_model, cfg, dur_scale, dur_bias, logits_of):
    """logits_of(model, x, semb) -> the pitch_cond logits [1,T,K] as the model's generate() forms them"""
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    model = make_model(**cfg)
    randomize_bn(model, g)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn(p.shape, generator=g))
        model.dur_pred.lin.weight.mul_(dur_scale)
        model.dur_pred.lin.bias.fill_(dur_bias)
    model.eval()
    x = torch.zeros(len(X_LEN), TX, dtype=torch.long)
    for b, L in enumerate(X_LEN):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    semb = torch.randn(len(X_LEN), cfg['speaker_emb_dims'], generator=g)
    semb = semb / semb.norm(dim=1, keepdim=True)
    items, fallback, worst_int, worst_half, worst_logit, spread, classes = [], [], 1.0, 1.0, 1e9, [], set()
    for b, L in enumerate(X_LEN):
        xb, sb = x[b:b + 1, :L].clone(), semb[b:b + 1].clone()
        with torch.no_grad():
            logits = logits_of(model, xb, sb)
            pc = torch.argmax(logits, dim=2)
            raw = model.dur_pred(xb, pc, sb, alpha=ALPHA).squeeze(2)  # what generate() decides the fallback on
        fallback.append(bool(torch.sum(raw.long()) <= 0))
        mi, mh = margins(raw.numpy().astype(np.float64))
        worst_int, worst_half = min(worst_int, mi), min(worst_half, mh)
        worst_logit = min(worst_logit, logit_margin(logits.numpy()))
        spread += raw.flatten().tolist()
        classes |= set(pc.flatten().tolist())
        out = model.generate(xb, sb, alpha=ALPHA)
        assert torch.equal(out['pitch_cond'].reshape(-1), pc.reshape(-1))
        out['dur_hat'] = raw
        out['pitch_cond_logits'] = logits
        items.append(out)
    ok = any(fallback) and not all(fallback) and min(worst_int, worst_half, worst_logit) >= MARGIN and \
        len(classes) >= 2 and min(spread) < SPREAD[0] and max(spread) > SPREAD[1]
    return ok, model, x, semb, items, fallback, (worst_int, worst_half, worst_logit, min(spread), max(spread), sorted(classes))


def search(name, make_model, cfg, dur_scale, dur_bias, logits_of, put_state):
    for seed in range(1000):
        ok, model, x, semb, items, fallback, info = build(seed, make_model, cfg, dur_scale, dur_bias, logits_of)
        if ok:
            break
    else:
        raise SystemExit('no seed satisfies the fixture conditions')
    assert any(fallback) and not all(fallback)
    assert min(info[:3]) >= MARGIN and len(info[5]) >= 2
    assert bool((x[torch.arange(TX)[None, :] < torch.tensor(X_LEN)[:, None]] != 0).all())
    out = {'x': x.numpy(), 'x_len': np.asarray(X_LEN, dtype=np.int64), 'speaker_emb': semb.numpy(), 'alpha': np.float64(ALPHA),
           'fallback': np.asarray(fallback), 'seed': np.int64(seed)}
    put_state(out, model.state_dict())
    for b, o in enumerate(items):
        for k, v in o.items():
            out[f'item{b}/{k}'] = v.detach().numpy()
    np.savez_compressed(os.path.join(HERE, name), **out)
    print(f'{name}: seed {seed}, fallback {fallback}, margins int {info[0]:.2e} half {info[1]:.2e} logit {info[2]:.2e}, '
          f'dur_hat in [{info[3]:.2f}, {info[4]:.2f}], classes {info[5]}, mel_len {[int(o["mel"].shape[2]) for o in items]}')


def main():
    from models.multi_forward_tacotron import MultiForwardTacotron

    def put_state(out, sd):
        for k, v in sd.items():
            out['sd/' + k] = v.clone().numpy()

    search('multi_generate_batch.npz', MultiForwardTacotron, TINY_MULTI, DUR_SCALE, DUR_BIAS,
           lambda m, x, s: m.pitch_cond_pred(x, s), put_state)


if __name__ == '__main__':
    main()
