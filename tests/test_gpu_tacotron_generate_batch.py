"""GPU: Tacotron.generate_batch (forwardtacotron_amd/tacotron.py, ft_taco_gen_batch_steps) against the reference's
generate of every sentence alone (tests/golden/tacotron_generate_batch.npz), against generate() on the same model and
GPU, and its exact properties: batch permutation, independence of the other items' tokens and of the padding,
chunking (also around every stop step), the per-item stop arithmetic, the refusals.

TOL is the bound tests/test_gpu_tacotron_generate.py holds generate() to against the reference."""
import numpy as np
import pytest
import torch

from forwardtacotron_amd import _lib, base
from forwardtacotron_amd import hip as H
from forwardtacotron_amd import tacotron as T
from test_tacotron_generate_batch_cpu import CASES, GOLD, batch_case, item_errors

pytestmark = pytest.mark.gpu

TOL = 1e-4
KEYS = ('mel', 'linear', 'attn', 'mel_len', 'steps_out')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _model(gold, name, threshold=None):
    m, cfg, r, steps, x, x_len, semb = batch_case(gold, name)
    m = m.cuda()
    if threshold is not None:
        m.stop_threshold.fill_(threshold)
    return m, cfg, r, steps, x.cuda(), x_len, None if semb is None else semb.cuda()


def _gen(m, x, x_len, steps, semb=None):
    out = m.generate_batch(x, x_len, semb, steps=steps)
    torch.cuda.synchronize()
    H.check_rnn_status()
    assert set(out) == set(KEYS)
    assert all(out[k].is_cuda for k in KEYS) and out['mel_len'].dtype == out['steps_out'].dtype == torch.int64
    return out


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in KEYS)


def _check_padding(out, x_len):
    for b in range(out['mel'].shape[0]):
        t, s, n = int(out['mel_len'][b]), int(out['steps_out'][b]), int(x_len[b])
        for k in ('mel', 'linear'):
            assert bool((out[k][b, :, t:] == base.PAD_VALUE).all()), (k, b)
            assert bool(torch.isfinite(out[k][b, :, :t]).all()), (k, b)
        assert not bool(out['attn'][b, s:].any()) and not bool(out['attn'][b, :, n:].any()), b
    assert int(out['mel'].shape[2]) == int(out['mel_len'].max()) and int(out['attn'].shape[1]) == int(out['steps_out'].max())


@pytest.mark.parametrize('name', CASES)
def test_generate_batch_matches_reference_fixture(gold, name):
    m, cfg, r, steps, x, x_len, semb = _model(gold, name)
    out = _gen(m, x, x_len, steps, semb)
    err = item_errors(gold, name, out)
    print(name, 'largest |valid part - reference alone|:', err)
    assert max(err.values()) <= TOL, err
    _check_padding(out, x_len)
    assert m.training                                   # train() on return, like generate
    # x_len on the device gives the same result
    assert _same(out, _gen(m, x, x_len.cuda(), steps, semb))


@pytest.mark.parametrize('name', ['s1', 'full'])
def test_generate_batch_matches_generate(gold, name):
    m, cfg, r, steps, x, x_len, semb = _model(gold, name)
    out = _gen(m, x, x_len, steps, semb)
    worst = dict(mel=0.0, linear=0.0, attn=0.0)
    for b in range(x.shape[0]):
        n = int(x_len[b])
        mel, lin, attn = m.generate(x[b:b + 1, :n], None if semb is None else semb[b:b + 1], steps=steps)
        s = attn.shape[0]
        assert int(out['steps_out'][b]) == s, b
        for k, got, ref in (('mel', out['mel'][b, :, :s * r], mel), ('linear', out['linear'][b, :, :s * r], lin),
                            ('attn', out['attn'][b, :s, :n], attn)):
            worst[k] = max(worst[k], float(np.abs(got.double().cpu().numpy() - ref).max()))
    print(name, 'largest |generate_batch - generate|:', worst)
    assert max(worst.values()) <= TOL, worst


def test_permuting_the_batch_permutes_the_outputs(gold):
    m, _, _, steps, x, x_len, _ = _model(gold, 's1')
    out = _gen(m, x, x_len, steps)
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    got = _gen(m, x[perm.cuda()], x_len[perm], steps)
    for k in KEYS:
        assert torch.equal(got[k], out[k][perm.cuda()]), k


@pytest.mark.parametrize('name', ['s1', 't17'])
def test_other_items_and_padding_do_not_reach_an_item(gold, name):
    m, _, r, steps, x, x_len, _ = _model(gold, name)
    out = _gen(m, x, x_len, steps)
    B, Tx = x.shape
    g = torch.Generator().manual_seed(5)
    for b in (0, 3, B - 1):
        x2 = torch.randint(1, 135, (B, Tx), generator=g).cuda()
        x2[b, :int(x_len[b])] = x[b, :int(x_len[b])]
        got = _gen(m, x2, x_len, steps)
        s, n = int(out['steps_out'][b]), int(x_len[b])
        assert int(got['steps_out'][b]) == s and int(got['mel_len'][b]) == s * r
        assert torch.equal(got['mel'][b, :, :s * r], out['mel'][b, :, :s * r]), b
        assert torch.equal(got['linear'][b, :, :s * r], out['linear'][b, :, :s * r]), b
        assert torch.equal(got['attn'][b, :s, :n], out['attn'][b, :s, :n]), b
        _check_padding(got, x_len)


def test_chunking_does_not_change_outputs(gold, monkeypatch):
    m, _, _, steps, x, x_len, _ = _model(gold, 's1')
    outs = []
    for k in (1, 5, 64):
        monkeypatch.setattr(T, 'GEN_CHUNK', k)
        outs.append(_gen(m, x, x_len, steps))
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])


def test_stops_at_chunk_boundaries(gold, monkeypatch):
    m, _, _, steps, x, x_len, _ = _model(gold, 's1')
    base_out = _gen(m, x, x_len, steps)
    assert base_out['steps_out'].tolist() == gold['s1/s_out'].tolist()
    for s_out in sorted(set(gold['s1/s_out'].tolist())):
        for k in (s_out - 1, s_out, s_out + 1):
            monkeypatch.setattr(T, 'GEN_CHUNK', k)
            assert _same(base_out, _gen(m, x, x_len, steps)), (s_out, k)


@pytest.mark.parametrize('r', [1, 2, 3])
def test_stop_arithmetic(gold, r):
    m, _, _, _, x, x_len, _ = _model(gold, 's1', threshold=1e3)
    m.r = r
    B = x.shape[0]
    out = _gen(m, x, x_len, 48)
    assert out['steps_out'].tolist() == [10 // r + 2] * B and out['mel_len'].tolist() == [(10 // r + 2) * r] * B
    assert out['mel'].shape == (B, 80, (10 // r + 2) * r)
    out = _gen(m, x, x_len, 5)                             # steps before the stop point: runs to S
    assert out['steps_out'].tolist() == [-(-5 // r)] * B
    _check_padding(out, x_len)


def test_refusals(gold):
    m, _, _, _, x, x_len, _ = _model(gold, 's1')
    with pytest.raises(_lib.FtError, match='generate_batch'):
        m.cpu().generate_batch(x.cpu(), x_len, steps=10)
    m.cuda()
    m.r = 21
    with pytest.raises(_lib.FtError, match='generate_batch'):
        m.generate_batch(x, x_len, steps=10)
    m.r = 1
    for steps in (0, -3, torch.tensor(0)):
        with pytest.raises(_lib.FtError, match='generate_batch'):
            m.generate_batch(x, x_len, steps=steps)
    with pytest.raises(_lib.FtError, match='generate_batch'):                       # B = 0
        m.generate_batch(x[:0], x_len[:0], steps=10)
    with pytest.raises(_lib.FtError, match='generate_batch'):
        m.generate_batch(torch.ones(2, 1025, dtype=torch.int64, device='cuda'), torch.tensor([3, 4]), steps=10)
    for bad in (torch.tensor([1, 5, 9, 13, 7, 3]), torch.tensor([0, 5, 9, 12, 7, 3]), torch.tensor([1, 5, 9]),
                torch.tensor([1, 5, 9, 12, 7, 3], dtype=torch.int32)):
        with pytest.raises(_lib.FtError, match='generate_batch'):                   # host x_len: before any launch
            m.generate_batch(x, bad, steps=10)
    for bad in (torch.tensor([1, 5, 9, 13, 7, 3]), torch.tensor([0, 5, 9, 12, 7, 3])):
        with pytest.raises(_lib.FtError, match='generate_batch'):                   # device x_len: the device flag
            m.generate_batch(x, bad.cuda(), steps=10)
    torch.cuda.synchronize()
    assert m.training
    ms, cfg, _, _, xs, xl, semb = _model(gold, 'spk')
    E = cfg['speaker_emb_dim']
    for bad in (None, torch.rand(3, E + 1).cuda(), torch.rand(2, E).cuda(), torch.rand(1, E).cuda()):
        with pytest.raises(_lib.FtError, match='generate_batch'):
            ms.generate_batch(xs, xl, bad, steps=10)
    # the C entries check their own bounds
    q = lambda *a: _lib.query('ft_taco_gen_batch_workspace', *a)
    assert q(0, 8, 40, 1) == 0 and q(2, 1025, 40, 1) == 0 and q(2, 8, 0, 1) == 0 and q(2, 8, 40, 21) == 0
    nb = q(2, 8, 40, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    fp = torch.zeros(4096, device='cuda').data_ptr()
    for B, Tx, L, r, S, s0, n, size in ((0, 8, 40, 1, 4, 0, 1, nb), (2, 1025, 40, 1, 4, 0, 1, nb), (2, 8, 0, 1, 4, 0, 1, nb),
                                        (2, 8, 40, 21, 4, 0, 1, nb), (2, 8, 40, 1, 4, 3, 2, nb), (2, 8, 40, 1, 4, -1, 1, nb),
                                        (2, 8, 40, 1, 4, 0, 1, nb - 1)):
        with pytest.raises(_lib.FtError, match='taco_gen_batch_steps'):
            _lib.call('ft_taco_gen_batch_steps', *(fp,) * 7, 384, *(fp,) * 20, 0.0, *(fp,) * 6, B, Tx, L, r, S, s0, n,
                      ws.data_ptr(), size, H._stream())
