"""CPU: what of melgan.MelGAN needs no device -- the parameter tree against the stock-torch tree of tests/melgan_cpu.py
(keys, shapes, seed-identical initialisation), the checkpoint round trip, the folded and packed weights against
torch._weight_norm in float64, the polyphase identity the transposed-convolution kernel rests on, the length
arithmetic, every validation error, and the condition of the test fixture itself (an unsaturated tanh)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import melgan_cpu as R
from forwardtacotron_amd import melgan as M
from forwardtacotron_amd._lib import FtError


@pytest.fixture(scope='module')
def full_ref():
    return R.build(0, torch.float64, **R.FULL)


def test_the_126_keys_and_shapes_are_the_stock_trees():
    ref = R.build(0, **R.FULL)
    torch.manual_seed(1)
    sd, want = M.MelGAN().state_dict(), ref.state_dict()
    assert len(want) == 126 and list(sd) == list(want)
    assert all(sd[k].shape == want[k].shape and sd[k].dtype == want[k].dtype for k in want)
    for k in ('generator.1.weight_g', 'generator.4.blocks.0.2.weight_v', 'generator.4.shortcuts.0.bias',
              'generator.3.weight_g', 'generator.13.blocks.2.4.bias', 'generator.16.weight_v'):
        assert k in sd, k
    assert tuple(sd['generator.3.weight_v'].shape) == (512, 256, 16) and tuple(sd['generator.3.weight_g'].shape) == (512, 1, 1)
    assert tuple(sd['generator.16.weight_v'].shape) == (1, 32, 7)


@pytest.mark.parametrize('cfg', [R.FULL, R.NARROW], ids=['full', 'narrow'])
def test_initialisation_is_seed_identical_to_the_stock_tree(cfg):
    want = R.build(7, **cfg).state_dict()
    torch.manual_seed(7)
    got = M.MelGAN(**cfg).state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize('layout', ['bare', 'model_g'])
def test_checkpoint_round_trip_in_both_layouts(tmp_path, layout):
    state = R.build(3, **R.NARROW).state_dict()
    path = tmp_path / f'{layout}.pt'
    torch.save(state if layout == 'bare' else {'model_g': state, 'model_d': {}, 'step': 5}, path)
    torch.manual_seed(99)
    voc = M.MelGAN.from_checkpoint(path, **R.NARROW)
    got = voc.state_dict()
    assert all(torch.equal(got[k], state[k]) for k in state)
    broken = dict(state)
    del broken['generator.4.shortcuts.1.bias']
    torch.save(broken, path)
    with pytest.raises(FtError, match='shortcuts.1.bias'):
        M.MelGAN.from_checkpoint(path, **R.NARROW)


def test_folded_and_packed_weights_against_weight_norm_in_float64():
    torch.manual_seed(5)
    voc = M.MelGAN(**R.NARROW).double()
    g = voc.generator
    for conv in (g[1], g[4].blocks[1][2], g[4].blocks[1][4], g[4].shortcuts[2], g[16]):          # Conv1d [cout, cin, k]
        v, gg = conv.weight_v.detach(), conv.weight_g.detach()
        v.mul_(1.7)                                                           # (so that g != ||v||: the fold does something)
        w = torch._weight_norm(v, gg, 0)
        got = M.fold_weight_norm(v, gg)
        assert float((got - w).abs().max()) <= 4 * np.finfo(np.float64).eps * float(w.abs().max())
        cout, cin, k = w.shape
        if conv is g[16]:
            p = M.pack_conv_out(got)
            assert tuple(p.shape) == (cin, 32) and torch.equal(p[:, :7], got[0]) and not p[:, 7:].any()
            continue
        p = M.pack_conv(got).reshape(k, cin, M.padded_width(cout))
        assert all(torch.equal(p[t, :, :cout], got[:, :, t].T) for t in range(k)) and not p[:, :, cout:].any()
        b = M.pack_bias(conv.bias.detach())
        assert b.numel() == M.padded_width(cout) and torch.equal(b[:cout], conv.bias.detach()) and not b[cout:].any()
    ct = g[3]                                                                 # ConvTranspose1d [cin, cout, k]: dim 0 is cin
    v, gg = ct.weight_v.detach(), ct.weight_g.detach()
    v.mul_(0.6)
    w = torch._weight_norm(v, gg, 0)
    got = M.fold_weight_norm(v, gg)
    assert float((got - w).abs().max()) <= 4 * np.finfo(np.float64).eps * float(w.abs().max())
    p = M.pack_conv_transpose(got)
    cin, cout, k = w.shape
    assert tuple(p.shape) == (k, cin, M.padded_width(cout))
    assert all(torch.equal(p[t, :, :cout], got[:, :, t]) for t in range(k)) and not p[:, :, cout:].any()


@pytest.mark.parametrize('k,s,pad', [(16, 8, 4), (4, 2, 1)])
@pytest.mark.parametrize('L', [1, 2, 11])
def test_polyphase_identity(k, s, pad, L):
    """two taps per phase == ConvTranspose1d, in float64, every output position"""
    gen = torch.Generator().manual_seed(10 * k + L)
    cin, cout = 5, 3
    x = torch.randn(cin, L, dtype=torch.float64, generator=gen)
    w = torch.randn(cin, cout, k, dtype=torch.float64, generator=gen)
    b = torch.randn(cout, dtype=torch.float64, generator=gen)
    want = F.conv_transpose1d(x.unsqueeze(0), w, b, stride=s, padding=pad)[0]
    assert want.shape[1] == s * L
    got = torch.full_like(want, float('nan'))
    for q in range(L + 1):
        for p in range(s):
            j = s * q + p - s // 2
            if not 0 <= j < s * L:
                continue
            acc = b.clone()
            for row, tap in M.polyphase_taps(q, p, s):
                if 0 <= row < L:
                    acc = acc + w[:, :, tap].T @ x[:, row]
            got[:, j] = acc
    assert not torch.isnan(got).any()
    assert float((got - want).abs().max()) < 1e-12


def test_length_arithmetic_and_the_tail_cut():
    ref = R.build(2, **R.NARROW)
    voc = M.MelGAN(**R.NARROW)
    assert voc.hop_length == ref.hop == 256 and M.TAIL_FRAMES == 10
    for n in (1, 2, 23):
        mel = R.make_mels([n], 8, n)[1][0]
        with torch.no_grad():
            audio = ref.inference(mel.unsqueeze(0))
            full = ref.forward(torch.cat((mel, torch.full((8, 10), R.PAD_VALUE)), dim=1).unsqueeze(0))
        assert full.shape[-1] == 256 * (n + 10) and audio.numel() == 256 * n == M.wav_length(n)
        assert audio.dtype == torch.int16


def test_every_validation_error_is_raised_without_a_device():
    voc = M.MelGAN(**R.NARROW).eval()
    ok = torch.zeros(2, 8, 5)
    lens = torch.tensor([5, 3])
    with torch.no_grad():
        with pytest.raises(FtError, match='float32'):
            voc.inference_batch(ok.double(), lens)
        with pytest.raises(FtError, match=r'\[B, n_mels, Tmax\]'):
            voc.inference_batch(ok[0], lens)
        with pytest.raises(FtError, match='8 mel channels'):
            voc.inference_batch(torch.zeros(2, 9, 5), lens)
        with pytest.raises(FtError, match='empty batch'):
            voc.inference_batch(torch.zeros(0, 8, 5), torch.zeros(0, dtype=torch.int64))
        with pytest.raises(FtError, match='empty batch'):
            voc.inference_batch(torch.zeros(2, 8, 0), lens)
        for bad in (torch.tensor([5, 0]), torch.tensor([6, 1]), torch.tensor([-1, 2])):
            with pytest.raises(FtError, match='mel_len must be in'):
                voc.inference_batch(ok, bad)
        with pytest.raises(FtError, match='int64'):
            voc.inference_batch(ok, lens.to(torch.int32))
        with pytest.raises(FtError, match='int64'):
            voc.inference_batch(ok, torch.tensor([5, 3, 1]))
        with pytest.raises(FtError, match='int64'):
            voc.inference_batch(ok, [5, 3])
        with pytest.raises(FtError, match='one mel'):
            voc.inference(ok)
        with pytest.raises(FtError, match='HIP'):                      # all valid: the only thing missing is the device
            voc.inference_batch(ok, lens)
        with pytest.raises(FtError, match='HIP'):
            voc.forward(ok)
    with pytest.raises(FtError, match='no autograd'):                  # parameters require grad and grad mode is on
        voc.inference_batch(ok, lens)
    for p in voc.parameters():
        p.requires_grad_(False)
    with pytest.raises(FtError, match='no autograd'):
        voc.forward(ok.clone().requires_grad_(True))
    with pytest.raises(FtError, match='kernel = 2 stride'):
        M.MelGAN(upsamples=((16, 8, 4), (16, 8, 4), (4, 2, 1), (3, 2, 1)))
    with pytest.raises(FtError, match='multiples of 8'):
        M.MelGAN(mel_channel=80, channels=(512, 256, 128, 60, 32))


@pytest.mark.parametrize('cfg,lens', [(R.FULL, [23, 1, 2, 7]), (R.NARROW, [23, 1, 2, 7, 40])], ids=['full', 'narrow'])
def test_the_fixture_does_not_saturate_the_tanh(cfg, lens):
    """in float64 the pre-tanh RMS lies in [0.05, 1] and max |pre-tanh| < 3: a saturated tanh cannot hide an error"""
    ref = R.build(0, torch.float64, **cfg)
    _, items = R.make_mels(lens, cfg['mel_channel'], 11)
    with torch.no_grad():
        pre = torch.cat([ref.stages(m.double())[1] for m in items])
    rms, top = float(pre.pow(2).mean().sqrt()), float(pre.abs().max())
    print(f'pre-tanh RMS {rms:.3f}, max {top:.3f}')
    assert 0.05 <= rms <= 1.0 and top < 3.0
