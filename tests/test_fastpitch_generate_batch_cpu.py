"""CPU: the fixture of FastPitch.generate_batch (tests/golden/fastpitch_generate_batch.npz, captured from the imported
reference by tests/golden/make_golden_fastpitch_generate_batch.py) meets its own conditions, and oracle/fp_oracle.py's
generate on every item alone reproduces it."""
import numpy as np
import pytest
import torch

from oracle import fp_oracle as FP
from helpers import TINY_FP, fp_state, load_npz, maxdiff

MARGIN = 1e-3
KEYS = ('mel', 'mel_post', 'dur', 'pitch', 'energy')


@pytest.fixture(scope='module')
def G():
    return load_npz('fastpitch_generate_batch.npz')


def test_fixture_meets_its_conditions(G):
    x, x_len = G['x'], G['x_len']
    B, Tx = x.shape
    assert x_len.tolist() == [7, 1, 4, 7, 2] and Tx == 7 and TINY_FP['conv1_kernel'] == 5
    valid = np.arange(Tx)[None, :] < x_len[:, None]
    assert (x[valid] >= 1).all() and (x[valid] < TINY_FP['num_chars']).all() and (x[~valid] == 0).all()
    fallback = G['fallback'].tolist()
    assert any(fallback) and not all(fallback)
    spread = []
    for b in range(B):
        d = G[f'item{b}/dur_hat'].astype(np.float64)
        assert d.shape == (1, int(x_len[b]))
        assert np.abs(d - np.round(d)).min() >= MARGIN, b                       # the fallback's truncation
        assert np.abs((d - 0.5) - np.round(d - 0.5)).min() >= MARGIN, b         # the LengthRegulator's rounding
        assert fallback[b] == bool(np.trunc(d).sum() <= 0), b
        dur = G[f'item{b}/dur']
        if fallback[b]:
            assert (dur == 2.0).all()
        assert G[f'item{b}/mel'].shape[2] == int(np.floor(np.maximum(dur, 0) + 0.5).sum()), b
        spread += d.flatten().tolist()
    assert min(spread) < 0.5 and max(spread) > 4.5


def test_oracle_reproduces_every_item_alone(G):
    P = fp_state(G, 'sd/')
    alpha = float(G['alpha'])
    x = torch.from_numpy(G['x'])
    for b, L in enumerate(G['x_len'].tolist()):
        out = FP.generate(P, x[b:b + 1, :L].clone(), TINY_FP, alpha=alpha)
        assert out['mel'].shape == G[f'item{b}/mel'].shape, b
        for k in KEYS:
            d = maxdiff(out[k], G[f'item{b}/{k}'])
            assert d < 1e-5, (b, k, d)                                          # test_oracle_fastpitch.py::test_generate
