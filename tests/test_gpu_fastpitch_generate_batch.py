"""GPU: FastPitch.generate_batch -- every item of a ragged batch gets what generate() gives it alone.  Mirrors
test_gpu_generate_batch.py; the length-aware attention kernel under it is tested alone in test_gpu_attn_lens.py."""
import numpy as np
import pytest
import torch

from helpers import TINY_FP, fp_state, load_npz, maxdiff

pytestmark = pytest.mark.gpu

PAD = float(np.float32(-11.5129))
KEYS = ('mel', 'mel_post', 'dur', 'pitch', 'energy')
BAR = 5e-5              # test_gpu_generate_batch.py / test_gpu_fastpitch.py (generate vs the golden fixture)


@pytest.fixture(scope='module')
def fx():
    """(fixture, model on the device, x, x_len, generate_batch of the zero-padded fixture batch) -- computed once"""
    from forwardtacotron_amd.fastpitch import FastPitch
    G = load_npz('fastpitch_generate_batch.npz')
    m = FastPitch(**TINY_FP)
    m.load_state_dict(fp_state(G, 'sd/'))
    m = m.cuda()
    x = torch.from_numpy(G['x']).cuda()
    x_len = torch.from_numpy(G['x_len'])
    out = m.generate_batch(x, x_len, alpha=float(G['alpha']))
    torch.cuda.synchronize()
    return G, m, x, x_len, {k: v.cpu() for k, v in out.items()}


def _valid(out, b, L, n):
    return {'mel': out['mel'][b:b + 1, :, :n], 'mel_post': out['mel_post'][b:b + 1, :, :n], 'dur': out['dur'][b:b + 1, :L],
            'pitch': out['pitch'][b:b + 1, :, :L], 'energy': out['energy'][b:b + 1, :, :L]}


def _check_padding(out, b, L, n):
    for k in ('mel', 'mel_post'):
        assert bool((out[k][b, :, n:] == PAD).all()), (b, k, 'padded frames must hold padding_value exactly')
    assert bool((out['dur'][b, L:] == 0).all()) and bool((out['pitch'][b, :, L:] == 0).all()) and \
        bool((out['energy'][b, :, L:] == 0).all()), (b, 'padded tokens must be exactly 0')


def test_golden(fx):
    G, m, x, x_len, out = fx
    B, Tx = x.shape
    frames = [G[f'item{b}/mel'].shape[2] for b in range(B)]
    assert out['mel_len'].dtype == torch.int64 and out['mel_len'].tolist() == frames
    Tm = max(frames)
    assert out['mel'].shape == out['mel_post'].shape == (B, TINY_FP['n_mels'], Tm)
    assert out['dur'].shape == (B, Tx) and out['pitch'].shape == out['energy'].shape == (B, 1, Tx)
    for b in range(B):
        L, n = int(x_len[b]), frames[b]
        for k, v in _valid(out, b, L, n).items():
            d = maxdiff(v, G[f'item{b}/{k}'])
            print(f'item {b} {k}: {d:.3e}')
            assert d < BAR, (b, k, d)
        _check_padding(out, b, L, n)


def test_pad_content_is_irrelevant(fx):
    G, m, x, x_len, out = fx
    g = torch.Generator().manual_seed(3)
    junk = torch.randint(1, TINY_FP['num_chars'], x.shape, generator=g)
    pad = torch.arange(x.shape[1])[None, :] >= x_len[:, None]
    x2 = torch.where(pad, junk, x.cpu()).cuda()
    assert bool((x2.cpu()[pad] != 0).all()) and x2.shape == x.shape
    out2 = m.generate_batch(x2, x_len.cuda(), alpha=float(G['alpha']))      # (x_len on the device this time)
    assert set(out2) == set(out)
    for k in out:
        assert torch.equal(out2[k].cpu(), out[k]), f'{k} depends on what the padding holds'


def test_neighbours_are_irrelevant(fx):
    G, m, x, x_len, out = fx
    alpha = float(G['alpha'])
    b, L = 2, int(x_len[2])                       # 4 tokens; in the batch of 5 it sits between a 1- and a 7-token item
    n = int(out['mel_len'][b])
    in5 = _valid(out, b, L, n)
    g = torch.Generator().manual_seed(4)
    x2 = torch.zeros(2, 9, dtype=torch.long)
    x2[0] = torch.randint(1, TINY_FP['num_chars'], (9,), generator=g)
    x2[1, :L] = x[b, :L].cpu()
    o2 = m.generate_batch(x2.cuda(), torch.tensor([9, L]), alpha=alpha)
    assert int(o2['mel_len'][1]) == n
    in2 = _valid({k: v.cpu() for k, v in o2.items()}, 1, L, n)
    alone = m.generate(x[b:b + 1, :L].contiguous(), alpha=alpha)
    assert alone['mel'].shape[2] == n
    for k in KEYS:
        a = alone[k].cpu()
        assert maxdiff(in5[k], a) < BAR and maxdiff(in2[k], a) < BAR and maxdiff(in5[k], in2[k]) < BAR, k


def test_existing_generate_differs_in_a_padded_batch(fx):
    """why the method exists: generate() runs the predictors and the postnet without any padding mask, so in the
    zero-padded batch a short item's own tokens attend to the pad rows and its convolutions read them"""
    G, m, x, x_len, out = fx
    o = m.generate(x, alpha=float(G['alpha']))
    b, L = 4, int(x_len[4])                       # 2 tokens beside 7-token neighbours
    d = maxdiff(o['pitch'][b:b + 1, :, :L].cpu(), G[f'item{b}/pitch'])
    print(f'generate() in the padded batch, item {b} pitch: {d:.3e} off the per-item result')
    assert d > BAR


def test_zero_token_inside_a_sentence_raises(fx):
    from forwardtacotron_amd._lib import FtError
    G, m, x, x_len, out = fx
    x2 = x.clone()
    x2[3, 2] = 0                                  # item 3 has 7 tokens
    for xl in (x_len, x_len.cuda()):
        with pytest.raises(FtError, match='token id 0'):
            m.generate_batch(x2, xl, alpha=float(G['alpha']))
    again = m.generate_batch(x, x_len, alpha=float(G['alpha']))             # the flag does not stick
    assert torch.equal(again['mel'].cpu(), out['mel'])


# ---- production widths: head width 64 in the predictors, 128 in the trunk -> ft_attn_fwd_lens ------------------------
X_LEN = [40, 13, 1, 27, 40]
ALPHA = 0.9


def _production(conv2_kernel, fft, dur_scale, dur_bias, seed):
    """data.FASTPITCH_MODEL with one layer per stack (seconds, not minutes) -> (cfg, model on the CPU, state, tokens)"""
    from forwardtacotron_amd import data
    from forwardtacotron_amd.fastpitch import FastPitch
    cfg = dict(data.FASTPITCH_MODEL, durpred_layers=1, pitch_layers=1, energy_layers=1, prenet_layers=1, postnet_layers=1,
               conv2_kernel=conv2_kernel, prenet_fft=fft, postnet_fft=fft)
    torch.manual_seed(0)
    m = FastPitch(**cfg)
    with torch.no_grad():                           # as tests/golden/make_golden_fastpitch_generate_batch.py
        m.dur_pred.lin.weight.mul_(dur_scale)
        m.dur_pred.lin.bias.fill_(dur_bias)
    P = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed)         # (token seed picked on the CPU so that the margins asserted below hold)
    x = torch.zeros(len(X_LEN), max(X_LEN), dtype=torch.long)
    for b, L in enumerate(X_LEN):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    return cfg, m, P, x


def _oracle_dur_hat(P, cfg, xb):
    from oracle import fp_oracle as O
    with torch.no_grad():
        return O.series_predictor(xb, None, P, 'dur_pred.', cfg['durpred_n_heads'], cfg['durpred_layers'],
                                  ALPHA).double().numpy()


def _to_grid(d, offset):
    """distance of every entry to the nearest integer + offset"""
    return np.abs((d - offset) - np.round(d - offset))


# (conv2_kernel, d_fft of the trunk, token seed): the production model, and a smaller variant whose conv2 has k = 3
@pytest.mark.parametrize('conv2_kernel,fft,seed', [(1, 1024, 0), (3, 256, 0)])
def test_production_widths_vs_oracle_per_item(conv2_kernel, fft, seed):
    from oracle import fp_oracle as O
    cfg, m, P, x = _production(conv2_kernel, fft, 3.0, 2.5, seed)
    want = []
    for b, L in enumerate(X_LEN):
        xb = x[b:b + 1, :L].clone()
        d = _oracle_dur_hat(P, cfg, xb)
        assert _to_grid(d, 0.0).min() >= 1e-3 and _to_grid(d, 0.5).min() >= 1e-3, b
        want.append(O.generate(P, xb, cfg, alpha=ALPHA))
    m = m.cuda()
    assert m.matmul_dtype == 'fp32'
    out = {k: v.cpu() for k, v in m.generate_batch(x.cuda(), torch.tensor(X_LEN), alpha=ALPHA).items()}
    assert out['mel_len'].tolist() == [w['mel'].shape[2] for w in want]
    for b, L in enumerate(X_LEN):
        n = want[b]['mel'].shape[2]
        for k, v in _valid(out, b, L, n).items():
            d = maxdiff(v, want[b][k])
            print(f'conv2 k = {conv2_kernel}, item {b} {k}: {d:.3e}')
            assert d < 1e-4, (b, k, d)              # test_gpu_generate_batch.py::test_production_widths_vs_oracle_per_item
        _check_padding(out, b, L, n)


def test_production_widths_bf16_vs_per_item_generate():
    """bf16 mode: generate_batch against bf16 generate() per item, both on the GPU (mel_len equals fp32's only if no
    duration flips).  The bar is twice the noise the EXISTING bf16 generate() shows for one item between B = 1 and the
    same item twice at B = 2 (another row count takes other GEMM tiles).  An item whose fp32 dur_hat lies within 0.05 of a
    rounding boundary (a half-integer) would be skipped; the durations of this model are kept narrow (dur_pred.lin
    scaled by 0.12 around a bias of 2.0, so every dur_hat rounds to 2) and the token seed chosen so that the fp32 oracle needs no skip."""
    cfg, m, P, x = _production(1, 1024, 0.12, 2.0, 1)
    skipped = []
    for b, L in enumerate(X_LEN):
        d = _oracle_dur_hat(P, cfg, x[b:b + 1, :L].clone())
        if _to_grid(d, 0.5).min() < 0.05 or np.trunc(d).sum() <= 0:
            print(f'item {b} skipped: fp32 dur_hat within 0.05 of a rounding boundary')
            skipped.append(b)
    assert len(skipped) == 0, 'the token seed was chosen so that no item needs skipping'
    m = m.cuda()
    m.matmul_dtype = 'bf16'
    xd = x.cuda()
    one = m.generate(xd[0:1].contiguous(), alpha=ALPHA)
    two = m.generate(xd[0:1].repeat(2, 1).contiguous(), alpha=ALPHA)
    assert one['mel'].shape[2] == two['mel'].shape[2]
    bar = {k: 2 * maxdiff(one[k].cpu(), two[k][0:1].cpu()) for k in KEYS}
    print('bf16 bar (2 x the B = 1 / B = 2 noise of generate): ' + ', '.join(f'{k} {v:.3e}' for k, v in bar.items()))
    out = {k: v.cpu() for k, v in m.generate_batch(xd, torch.tensor(X_LEN), alpha=ALPHA).items()}
    for b, L in enumerate(X_LEN):
        alone = m.generate(xd[b:b + 1, :L].contiguous(), alpha=ALPHA)
        n = alone['mel'].shape[2]
        assert int(out['mel_len'][b]) == n, b
        for k, v in _valid(out, b, L, n).items():
            d = maxdiff(v, alone[k].cpu())
            print(f'bf16 item {b} {k}: {d:.3e} (bar {bar[k]:.3e})')
            assert d <= bar[k], (b, k, d, bar[k])
        _check_padding(out, b, L, n)
