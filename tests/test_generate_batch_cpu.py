"""CPU: the generate_batch fixture (tests/golden/generate_batch.npz) is what the oracle computes for every item ALONE and
keeps its rounding margins; ForwardTacotron.generate_batch refuses what it cannot run."""
import numpy as np
import pytest
import torch

from helpers import TINY, load_npz, maxdiff, sub

MARGIN = 1e-3          # tests/golden/make_golden_generate_batch.py: 20x the 5e-5 parity bar of the GPU tests
KEYS = ('mel', 'mel_post', 'dur', 'pitch', 'energy')


@pytest.fixture(scope='module')
def G():
    return load_npz('generate_batch.npz')


def test_fixture_items_equal_the_oracle_alone(G):
    from oracle import ft_oracle as O
    P = sub(G, 'sd/')
    x, x_len, alpha = torch.from_numpy(G['x']), G['x_len'].tolist(), float(G['alpha'])
    assert x.shape == (5, 7) and x_len == [7, 1, 4, 7, 2] and alpha == 0.9
    for b, L in enumerate(x_len):
        out = O.generate(P, x[b:b + 1, :L].clone(), TINY, alpha=alpha)
        for k in KEYS:
            assert maxdiff(out[k], G[f'item{b}/{k}']) < 1e-5, (b, k)
        # the returned durations are the fallback's / the LengthRegulator's (clamped) form of dur_hat
        raw = torch.from_numpy(G[f'item{b}/dur_hat'])
        fell = bool(torch.sum(raw.long()) <= 0)
        assert fell == bool(G['fallback'][b])
        want = torch.full_like(raw, 2.) if fell else raw.clamp_min(0.)
        assert torch.equal(torch.from_numpy(G[f'item{b}/dur']), want), b
        frames = int(torch.sum((want + 0.5).long()))
        assert G[f'item{b}/mel'].shape == (1, TINY['n_mels'], frames)


def test_fixture_margins(G):
    fb = G['fallback'].tolist()
    assert any(fb) and not all(fb), 'one item must take the duration fallback and one must not'
    lo, hi = np.inf, -np.inf
    for b in range(5):
        d = G[f'item{b}/dur_hat'].astype(np.float64)
        assert np.abs(d - np.round(d)).min() >= MARGIN, f'item {b}: a dur_hat sits on an integer (fallback truncation)'
        assert np.abs((d - 0.5) - np.round(d - 0.5)).min() >= MARGIN, f'item {b}: a dur_hat sits on a rounding boundary'
        lo, hi = min(lo, d.min()), max(hi, d.max())
    assert lo < 0.5 and hi > 4.5, 'the rescaled duration predictor must spread its durations'


def test_generate_batch_refuses_what_it_cannot_run(G):
    from forwardtacotron_amd import _lib, model
    m = model.ForwardTacotron(**TINY)
    x = torch.from_numpy(G['x'])
    with pytest.raises(_lib.FtError, match='HIP'):
        m.generate_batch(x, torch.from_numpy(G['x_len']))                 # CPU tensors: no fallback
    with pytest.raises(_lib.FtError, match='x_len'):
        m.generate_batch(x, torch.tensor([7, 0, 4, 7, 2]))
    with pytest.raises(_lib.FtError, match='x_len'):
        m.generate_batch(x, torch.tensor([7, 1, 4, 8, 2]))
    with pytest.raises(_lib.FtError, match='x_len'):
        m.generate_batch(x, torch.tensor([7, 1, 4]))                       # one length per item
