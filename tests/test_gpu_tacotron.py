"""GPU: the Tacotron teacher's teacher-forced forward and align() (forwardtacotron_amd/tacotron.py, ft_taco_attend) against
the reference fixtures (tests/golden/tacotron.npz), the float64 restatement (tests/taco_cpu.py) on a full-size ragged
batch and in extraction mode, duration extraction end to end, and the one-direction LSTM entry (ft_lstm_fwd_uni)."""
import math
import os

import numpy as np
import pytest
import torch

import taco_cpu as R
from forwardtacotron_amd import _lib
from forwardtacotron_amd import hip as H
from forwardtacotron_amd.durations import DurationExtractor, extract_durations
from forwardtacotron_amd.tacotron import Tacotron, dropout_seed
from test_tacotron_cpu import FULL_CFG, case_batch, case_model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'tacotron.npz')
TOL = 1e-4


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _dev(batch):
    return {k: v.cuda() if torch.is_tensor(v) else v for k, v in batch.items()}


def _maxdiff(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).double()).abs().max())


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_forward_matches_reference_fixture(gold, name):
    m, _ = case_model(gold, name)
    m = m.cuda()
    p = name + '/'
    with torch.no_grad():
        mel, lin, attn = m(_dev(case_batch(gold, name)))
    torch.cuda.synchronize()
    H.check_rnn_status()
    for got, key in ((mel, 'mel_outputs'), (lin, 'linear'), (attn, 'attn_scores')):
        assert tuple(got.shape) == gold[p + key].shape, key
        assert _maxdiff(got, gold[p + key]) <= TOL, (key, _maxdiff(got, gold[p + key]))


@pytest.mark.parametrize('name', ['a', 'b', 'c', 'd'])
def test_align_is_forward_attention_bit_for_bit(gold, name, monkeypatch):
    m, _ = case_model(gold, name)
    m = m.cuda()
    batch = _dev(case_batch(gold, name))
    with torch.no_grad():
        attn_f = m(batch)[2]
        calls = []
        for meth in ('_mel_path', '_lstm', '_add'):
            monkeypatch.setattr(m, meth, lambda *a, _m=meth, **k: calls.append(_m))
        attn_a = m.align(batch)
    assert not calls, 'align ran the mel path'
    assert torch.equal(attn_a, attn_f)


def _extraction_model(gold, name):
    m, cfg = case_model(gold, name)
    m = m.cuda().eval()
    m.decoder.prenet.train()
    return m, cfg


def _masks(S, B, seed1, seed2):
    """the decoder prenet's two dropout masks, rebuilt from the documented seed order"""
    ones1 = torch.ones(S, B, 256, device='cuda')
    ones2 = torch.ones(S, B, 128, device='cuda')
    return {'dec1': H.dropout(ones1, 0.5, seed1).double().cpu(), 'dec2': H.dropout(ones2, 0.5, seed2).double().cpu()}


@pytest.mark.parametrize('name', ['a', 'b'])
def test_extraction_mode_matches_restatement_with_masks(gold, name):
    m, cfg = _extraction_model(gold, name)
    batch = case_batch(gold, name)
    r = m.r
    S = math.ceil(batch['mel'].shape[2] / r)
    B = batch['x'].shape[0]
    with torch.no_grad():
        torch.manual_seed(1234)
        mel, lin, attn = m(_dev(batch))
        torch.manual_seed(1234)
        attn2 = m.align(_dev(batch))
        torch.manual_seed(1234)
        s1, s2 = dropout_seed(), dropout_seed()
    assert torch.equal(attn, attn2), 'the same torch seed must give the same attention'
    masks = _masks(S, B, s1, s2)
    assert 0.4 < float((masks['dec1'] == 0).double().mean()) < 0.6
    P = {k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in m.state_dict().items()}
    rmel, rlin, rattn = R.forward(P, batch, cfg, r, masks=masks)
    assert _maxdiff(attn, rattn) <= TOL
    assert _maxdiff(mel, rmel) <= TOL
    assert _maxdiff(lin, rlin) <= TOL
    # and the masks matter: without them the attention differs
    _, _, plain = R.forward(P, batch, cfg, r, with_mel=False)
    assert _maxdiff(attn, plain) > 1e-3


def ragged_batch(B, seed, tx=(120, 201), tm=(500, 900), n_mels=80, semb_dim=0):
    """TacoCollator-shaped batch on the host: x padded with 0, mel with -11.5129 to max(mel_len) + 1 frames"""
    g = np.random.default_rng(seed)
    x_len = g.integers(tx[0], tx[1], B)
    x_len[0] = tx[1] - 1
    mel_len = g.integers(tm[0], tm[1], B)
    mel_len[-1] = tm[1] - 1
    Tx, steps = int(x_len.max()), int(mel_len.max()) + 1
    x = np.zeros((B, Tx), np.int64)
    mel = np.full((B, n_mels, steps), -11.5129, np.float32)
    for b in range(B):
        x[b, :x_len[b]] = g.integers(1, 135, x_len[b])
        mel[b, :, :mel_len[b]] = g.normal(-5., 2., (n_mels, mel_len[b]))
    return {'x': torch.from_numpy(x), 'mel': torch.from_numpy(mel), 'x_len': torch.from_numpy(x_len),
            'mel_len': torch.from_numpy(mel_len), 'speaker_emb': torch.zeros(B, semb_dim),
            'item_id': [f's{seed}_item{b:03d}' for b in range(B)]}


def _full_model(seed=0):
    torch.manual_seed(seed)
    m = Tacotron(**FULL_CFG)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if k.endswith('running_mean'):
                v.copy_(0.1 * torch.randn(v.shape, generator=g))
            elif k.endswith('running_var'):
                v.copy_(0.5 + torch.rand(v.shape, generator=g))
    return m.cuda().eval()


def test_full_size_ragged_batch_matches_restatement():
    """B = 32, Tx up to 200, steps up to 900, against float64.  The error is reported per block of 100 steps: the bound
    is the package's 1e-4 everywhere, and the per-block maxima show whether it grows with S."""
    m = _full_model()
    batch = ragged_batch(32, seed=5, tm=(600, 900))
    with torch.no_grad():
        mel, lin, attn = m(_dev(batch))
    torch.cuda.synchronize()
    H.check_rnn_status()
    P = {k: v.detach().double().cpu() if v.is_floating_point() else v.cpu() for k, v in m.state_dict().items()}
    with torch.no_grad():
        rmel, rlin, rattn = R.forward(P, batch, dict(encoder_k=16, postnet_k=8, num_highways=4), 1)
    S = attn.shape[1]
    ea = (attn.double().cpu() - rattn).abs().amax(dim=(0, 2))
    em = (mel.double().cpu() - rmel).abs().amax(dim=(0, 1))
    blocks = [(s, float(ea[s:s + 100].max()), float(em[s:s + 100].max())) for s in range(0, S, 100)]
    print('steps, max |attn err|, max |mel err| per 100 steps:', blocks)
    assert float(ea.max()) <= TOL, blocks
    assert float(em.max()) <= TOL, blocks
    assert _maxdiff(lin, rlin) <= TOL


def test_items_are_independent():
    m = _full_model(seed=3)
    batch = ragged_batch(5, seed=9, tx=(30, 61), tm=(100, 161))
    with torch.no_grad():
        attn = m.align(_dev(batch))
        mel = m(_dev(batch))[0]
        for b in (0, 2, 4):
            one = {k: (v[b:b + 1] if torch.is_tensor(v) else v) for k, v in batch.items()}
            a1 = m.align(_dev(one))
            m1 = m(_dev(one))[0]
            da, dm = _maxdiff(a1[0], attn[b].cpu()), _maxdiff(m1[0], mel[b].cpu())
            print(f'item {b}: alone vs in the batch, max |attn diff| {da:.3g}, max |mel diff| {dm:.3g}')
            assert da <= 1e-5 and dm <= 1e-5


def test_refusals(gold):
    m, _ = case_model(gold, 'a')
    m = m.cuda()
    batch = _dev(case_batch(gold, 'a'))
    m.train()
    with torch.no_grad(), pytest.raises(_lib.FtError, match='training the teacher'):
        m(batch)
    m.eval()
    m.postnet.train()
    with torch.no_grad(), pytest.raises(_lib.FtError, match='training'):
        m.align(batch)
    m.eval()
    with pytest.raises(_lib.FtError, match='no_grad'):       # grad enabled, parameters require grad
        m(batch)
    with pytest.raises(_lib.FtError, match='generate'):
        m.generate(batch['x'])
    long = dict(batch, x=torch.ones(3, 1025, dtype=torch.int64, device='cuda'))
    with torch.no_grad(), pytest.raises(_lib.FtError, match='Tx'):
        m.align(long)
    ms, _ = case_model(gold, 'c')
    ms = ms.cuda()
    nospk = {k: v for k, v in _dev(case_batch(gold, 'c')).items() if k != 'speaker_emb'}
    with torch.no_grad(), pytest.raises(_lib.FtError, match='speaker_emb'):
        ms(nospk)
    # the C entry checks its own bounds
    ws = torch.empty(1 << 20, dtype=torch.uint8, device='cuda')
    f = torch.zeros(8, device='cuda')
    for B, Tx, S, nb in ((1, 1025, 1, ws.numel()), (1, 4, 0, ws.numel()), (1, 4, 1, 16)):
        with pytest.raises(_lib.FtError):
            _lib.call('ft_taco_attend', *(f.data_ptr(),) * 4, 256, *(f.data_ptr(),) * 9, None, B, Tx, S, ws.data_ptr(),
                      nb, H._stream())


def test_extract_durations_end_to_end(tmp_path):
    m = _full_model(seed=1)
    batches = [ragged_batch(6, seed=s, tx=(40, 81), tm=(150, 301)) for s in (21, 22)]
    stats = extract_durations(m, [_dev(b) for b in batches], tmp_path)
    assert len(stats) == 12
    for bt in batches:
        for b, item in enumerate(bt['item_id']):
            d = np.load(tmp_path / f'{item}.npy')
            assert len(d) == int(bt['x_len'][b]) and d.sum() == int(bt['mel_len'][b])
    # what extract_durations writes equals DurationExtractor.extract_batch on forward()'s attention under the same
    # torch seed (extraction mode keeps the decoder prenet's dropout; both draw the same two seeds)
    ext = DurationExtractor(silence_threshold=-11., silence_prob_shift=0.25)
    bt = batches[1]
    torch.manual_seed(5)
    stats2 = extract_durations(m, [_dev(bt)], tmp_path / 'again')
    torch.manual_seed(5)
    with torch.no_grad():
        attn = m(_dev(bt))[2]
    res = ext.extract_batch(attn.contiguous(), bt['x'].cuda(), bt['x_len'], bt['mel'].cuda(), bt['mel_len'])
    for b, item in enumerate(bt['item_id']):
        np.testing.assert_array_equal(np.load(tmp_path / 'again' / f'{item}.npy'),
                                      res.durations[b, :int(bt['x_len'][b])].cpu().numpy())
        assert stats2[item].max_duration == int(res.max_duration[b])


def _lstm_ref(xp, whh, bhh):
    T, B, G = xp.shape
    Hd = G // 4
    h = torch.zeros(B, Hd, dtype=torch.float64)
    c = torch.zeros(B, Hd, dtype=torch.float64)
    out = []
    for t in range(T):
        g = xp[t] + h @ whh.t() + bhh
        i, f, gg, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
        h = torch.sigmoid(o) * torch.tanh(c)
        out.append(h)
    return torch.stack(out)


@pytest.mark.parametrize('Hd,B', [(512, 32), (37, 5)])
def test_one_direction_lstm_long_sequence(Hd, B):
    T = 820
    g = torch.Generator().manual_seed(Hd)
    s = 1 / math.sqrt(Hd)
    xp = torch.randn(T, B, 4 * Hd, generator=g) * 0.5
    whh = (torch.rand(4 * Hd, Hd, generator=g) * 2 - 1) * s
    bhh = (torch.rand(4 * Hd, generator=g) * 2 - 1) * s
    xd, wd, bd = xp.cuda(), whh.cuda(), bhh.cuda()
    out = torch.empty(T, B, Hd, device='cuda')
    cst = torch.empty(T, B, Hd, device='cuda')
    ws, nb = H._rnn_workspace(4, B, Hd, xd.device)
    before = H.rnn_counters()
    _lib.call('ft_lstm_fwd_uni', xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), cst.data_ptr(), B, T, Hd,
              None if ws is None else ws.data_ptr(), nb, H._stream())
    torch.cuda.synchronize()
    H.check_rnn_status()
    after = H.rnn_counters()
    ref = _lstm_ref(xp.double(), whh.double(), bhh.double())
    err = (out.double().cpu() - ref).abs().amax(dim=(1, 2))
    print(f'H={Hd}: persistent launches {after[0] - before[0]}; max err per 200 steps',
          [float(err[i:i + 200].max()) for i in range(0, T, 200)])
    assert float(err.max()) <= TOL
    if Hd == 512:
        assert after[0] - before[0] == 1, 'the 512-wide one-direction LSTM should run persistent'
