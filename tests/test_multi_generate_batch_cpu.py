"""CPU: the two fixtures of the speaker-conditioned generate_batch meet the conditions their makers searched the seed for
(tests/golden/make_golden_multi_generate_batch.py), and the CPU oracle reproduces the MultiFastPitch one per item."""
import numpy as np
import pytest
import torch

from helpers import TINY_MFP, fp_state, load_npz, maxdiff

MARGIN = 1e-3
SPREAD = (0.5, 4.5)
X_LEN = [7, 2, 4, 7, 3]
KEYS = ('mel', 'mel_post', 'dur', 'pitch', 'energy')


@pytest.mark.parametrize('name', ['multi_generate_batch.npz', 'multi_fastpitch_generate_batch.npz'])
def test_fixture_meets_its_conditions(name):
    G = load_npz(name)
    x, x_len, semb = G['x'], G['x_len'], G['speaker_emb']
    B, Tx = x.shape
    assert (B, Tx) == (5, 7) and x_len.tolist() == X_LEN and float(G['alpha']) == 0.9
    assert bool((x[np.arange(Tx)[None, :] < x_len[:, None]] != 0).all())                   # non-zero tokens
    assert semb.shape[0] == B and semb.dtype == np.float32
    assert np.allclose(np.linalg.norm(semb.astype(np.float64), axis=1), 1.0, atol=1e-6)
    for a in range(B):
        for b in range(a + 1, B):
            assert not np.array_equal(semb[a], semb[b])                                     # five different speakers
    fallback, spread, classes = [], [], set()
    for b in range(B):
        L = int(x_len[b])
        d = G[f'item{b}/dur_hat'].astype(np.float64)
        logits = np.sort(G[f'item{b}/pitch_cond_logits'].astype(np.float64), axis=-1)
        assert d.shape == (1, L) and logits.shape == (1, L, 3)
        assert np.abs(d - np.round(d)).min() >= MARGIN, b
        assert np.abs((d - 0.5) - np.round(d - 0.5)).min() >= MARGIN, b
        assert (logits[..., -1] - logits[..., -2]).min() >= MARGIN, b
        pc = G[f'item{b}/pitch_cond'].reshape(-1)
        assert pc.tolist() == np.argmax(G[f'item{b}/pitch_cond_logits'][0], axis=-1).tolist()
        classes |= set(pc.tolist())
        fb = bool(np.trunc(d).sum() <= 0)
        assert fb == bool(G['fallback'][b])
        if fb:
            assert bool((G[f'item{b}/dur'] == 2.0).all())
        fallback.append(fb)
        spread += d.flatten().tolist()
    assert any(fallback) and not all(fallback)
    assert len(classes) >= 2
    assert min(spread) < SPREAD[0] and max(spread) > SPREAD[1]


def test_oracle_reproduces_the_multi_fastpitch_fixture_per_item():
    from oracle import fp_oracle as O
    G = load_npz('multi_fastpitch_generate_batch.npz')
    P = fp_state(G, 'sd/')
    x, semb = torch.from_numpy(G['x']), torch.from_numpy(G['speaker_emb'])
    for b, L in enumerate(G['x_len'].tolist()):
        out = O.multi_generate(P, x[b:b + 1, :L].clone(), semb[b:b + 1].clone(), TINY_MFP, alpha=float(G['alpha']))
        assert out['pitch_cond'].reshape(-1).tolist() == G[f'item{b}/pitch_cond'].reshape(-1).tolist(), b
        for k in KEYS:
            d = maxdiff(out[k], G[f'item{b}/{k}'])
            assert d < 1e-5, (b, k, d)              # test_fastpitch_generate_batch_cpu.py
