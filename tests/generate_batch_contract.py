"""The contract of generate_batch (base.AcousticModel.generate_batch), stated once for every model that has the method:
each item of a ragged batch gets what generate() gives it alone.  A model's GPU test file keeps its own module fixture

    fx = (fixture, model on the device, x, x_len, generate_batch of the zero-padded fixture batch on the host)

and its tests call the checks below with it and the model's tiny config.  The fixture batches (B = 5, Tx = 7, x_len
[7, 1, 4, 7, 2]) hold a 1-token item, two full ones and neighbours of unequal length."""
import numpy as np
import pytest
import torch

from helpers import maxdiff

PAD = float(np.float32(-11.5129))
KEYS = ('mel', 'mel_post', 'dur', 'pitch', 'energy')
BAR = 5e-5              # test_gpu_model.py::test_generate_golden / test_gpu_fastpitch.py (generate vs the golden fixture)


def valid(out, b, L, n):
    return {'mel': out['mel'][b:b + 1, :, :n], 'mel_post': out['mel_post'][b:b + 1, :, :n], 'dur': out['dur'][b:b + 1, :L],
            'pitch': out['pitch'][b:b + 1, :, :L], 'energy': out['energy'][b:b + 1, :, :L]}


def check_padding(out, b, L, n, pad=PAD):
    for k in ('mel', 'mel_post'):
        assert bool((out[k][b, :, n:] == pad).all()), (b, k, 'padded frames must hold padding_value exactly')
    assert bool((out['dur'][b, L:] == 0).all()) and bool((out['pitch'][b, :, L:] == 0).all()) and \
        bool((out['energy'][b, :, L:] == 0).all()), (b, 'padded tokens must be exactly 0')


def check_golden(fx, cfg):
    G, m, x, x_len, out = fx
    B, Tx = x.shape
    frames = [G[f'item{b}/mel'].shape[2] for b in range(B)]
    assert out['mel_len'].dtype == torch.int64 and out['mel_len'].tolist() == frames
    Tm = max(frames)
    assert out['mel'].shape == out['mel_post'].shape == (B, cfg['n_mels'], Tm)
    assert out['dur'].shape == (B, Tx) and out['pitch'].shape == out['energy'].shape == (B, 1, Tx)
    for b in range(B):
        L, n = int(x_len[b]), frames[b]
        for k, v in valid(out, b, L, n).items():
            d = maxdiff(v, G[f'item{b}/{k}'])
            print(f'item {b} {k}: {d:.3e}')
            assert d < BAR, (b, k, d)
        check_padding(out, b, L, n)


def check_pad_content_is_irrelevant(fx, cfg):
    G, m, x, x_len, out = fx
    g = torch.Generator().manual_seed(3)
    junk = torch.randint(1, cfg['num_chars'], x.shape, generator=g)
    pad = torch.arange(x.shape[1])[None, :] >= x_len[:, None]
    x2 = torch.where(pad, junk, x.cpu()).cuda()
    assert bool((x2.cpu()[pad] != 0).all()) and x2.shape == x.shape
    out2 = m.generate_batch(x2, x_len.cuda(), alpha=float(G['alpha']))      # (x_len on the device this time)
    assert set(out2) == set(out)
    for k in out:
        assert torch.equal(out2[k].cpu(), out[k]), f'{k} depends on what the padding holds'


def check_neighbours_are_irrelevant(fx, cfg):
    G, m, x, x_len, out = fx
    alpha = float(G['alpha'])
    b, L = 2, int(x_len[2])                       # 4 tokens; in the batch of 5 it sits between a 1- and a 7-token item
    n = int(out['mel_len'][b])
    in5 = valid(out, b, L, n)
    g = torch.Generator().manual_seed(4)
    x2 = torch.zeros(2, 9, dtype=torch.long)
    x2[0] = torch.randint(1, cfg['num_chars'], (9,), generator=g)
    x2[1, :L] = x[b, :L].cpu()
    o2 = m.generate_batch(x2.cuda(), torch.tensor([9, L]), alpha=alpha)
    assert int(o2['mel_len'][1]) == n
    in2 = valid({k: v.cpu() for k, v in o2.items()}, 1, L, n)
    alone = m.generate(x[b:b + 1, :L].contiguous(), alpha=alpha)
    assert alone['mel'].shape[2] == n
    for k in KEYS:
        a = alone[k].cpu()
        assert maxdiff(in5[k], a) < BAR and maxdiff(in2[k], a) < BAR and maxdiff(in5[k], in2[k]) < BAR, k


def check_existing_generate_differs_in_a_padded_batch(fx, cfg):
    """why the method exists: in the zero-padded batch generate() gives a short item's own tokens another result"""
    G, m, x, x_len, out = fx
    o = m.generate(x, alpha=float(G['alpha']))
    b, L = 4, int(x_len[4])                       # 2 tokens beside 7-token neighbours
    d = maxdiff(o['pitch'][b:b + 1, :, :L].cpu(), G[f'item{b}/pitch'])
    print(f'generate() in the padded batch, item {b} pitch: {d:.3e} off the per-item result')
    assert d > BAR


def check_user_function_applies_per_token(fx, cfg):
    """the user callables see the masked series and their results are masked by a select: doubling the pitch doubles
    it bit for bit (padding stays exactly 0), leaves the durations alone and reaches the mel"""
    G, m, x, x_len, out = fx
    out2 = {k: v.cpu() for k, v in m.generate_batch(x, x_len, alpha=float(G['alpha']), pitch_function=lambda p: 2 * p).items()}
    assert torch.equal(out2['pitch'], 2 * out['pitch'])
    assert torch.equal(out2['dur'], out['dur'])
    assert not torch.equal(out2['mel'], out['mel'])


def check_bad_user_function_raises_and_nothing_sticks(fx, cfg):
    """a callable that returns another shape raises from inside the predictors' side stream: the caller's stream is
    current again afterwards and the next call is what it was"""
    from forwardtacotron_amd._lib import FtError
    G, m, x, x_len, out = fx
    B, Tx = x.shape
    before = torch.cuda.current_stream()
    with pytest.raises(FtError, match='_function must return'):
        m.generate_batch(x, x_len, alpha=float(G['alpha']), energy_function=lambda e: e.reshape(B, Tx))
    assert torch.cuda.current_stream() == before
    again = m.generate_batch(x, x_len, alpha=float(G['alpha']))
    assert set(again) == set(out)
    for k in out:
        assert torch.equal(again[k].cpu(), out[k]), k


def check_overlap_switch_is_bit_neutral(fx, cfg, monkeypatch):
    """FT_GEN_OVERLAP=0 runs the predictors in front of the prenet on the caller's stream: same kernels, same bits"""
    G, m, x, x_len, out = fx
    monkeypatch.setenv('FT_GEN_OVERLAP', '0')
    o = m.generate_batch(x, x_len, alpha=float(G['alpha']))
    assert set(o) == set(out)
    for k in out:
        assert torch.equal(o[k].cpu(), out[k]), k
