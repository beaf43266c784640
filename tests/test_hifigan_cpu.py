"""CPU: what of hifigan.HiFiGAN needs no device -- the parameter tree against the stock-torch tree of tests/hifigan_cpu.py
(keys, counts, shapes, seed-identical initialisation), that restatement against the written definition evaluated with
plain functional calls in float64, the zero-edge identities the residual kernels rest on, from_config, the checkpoint
round trip (a SYNTHETIC file of the published layout: no published checkpoint is available), every refusal, and the
condition of the GPU tests' fixtures (an unsaturated tanh and a signal well above the end-to-end tolerance)."""
import json

import pytest
import torch
import torch.nn.functional as F

import hifigan_cpu as R
from forwardtacotron_amd import hifigan as M
from forwardtacotron_amd._lib import FtError

LENS = [23, 1, 2, 7]
COUNTS = {'full': (234, 13_936_130), 'narrow': (234, 928_514), 'rb2': (69, 1_464_322)}


@pytest.mark.parametrize('name', ['full', 'narrow', 'rb2'])
def test_state_dict_keys_counts_and_seeded_initialisation_are_the_stock_trees(name):
    cfg = R.PRESETS[name]
    want = R.build(7, **cfg).state_dict()
    torch.manual_seed(7)
    voc = {'full': M.HiFiGAN.v1, 'narrow': M.HiFiGAN.v2, 'rb2': M.HiFiGAN.v3}[name]()
    got = voc.state_dict()
    assert list(got) == list(want) and len(got) == COUNTS[name][0]
    assert sum(v.numel() for v in got.values()) == COUNTS[name][1]
    assert all(got[k].shape == want[k].shape and torch.equal(got[k], want[k]) for k in want)
    assert voc.hop_length == 256
    for k in ('conv_pre.bias', 'conv_pre.weight_g', 'conv_pre.weight_v', 'ups.0.weight_v', 'conv_post.weight_v',
              'resblocks.4.convs1.2.bias' if cfg['resblock'] == '1' else 'resblocks.4.convs.1.bias'):
        assert k in got, k
    C0 = cfg['upsample_initial_channel']
    assert tuple(got['ups.0.weight_v'].shape) == (C0, C0 // 2, 16) and tuple(got['ups.0.weight_g'].shape) == (C0, 1, 1)
    assert tuple(got['conv_post.weight_v'].shape) == (1, C0 >> len(cfg['upsample_rates']), 7)


def _definition(sd, cfg, mel):
    """the written definition with functional calls on the state dict, float64"""
    def w(p):
        v, g = sd[p + '.weight_v'].double(), sd[p + '.weight_g'].double()
        return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(g.shape)), sd[p + '.bias'].double()

    def conv(x, p, d=1):
        wt, b = w(p)
        return F.conv1d(x, wt, b, dilation=d, padding=d * (wt.shape[2] - 1) // 2)
    lr = lambda t: torch.where(t > 0, t, 0.1 * t)                                       # noqa: E731
    x = conv(mel.double().unsqueeze(0), 'conv_pre')
    nk = len(cfg['resblock_kernel_sizes'])
    for i, (u, k) in enumerate(zip(cfg['upsample_rates'], cfg['upsample_kernel_sizes'])):
        wt, b = w(f'ups.{i}')
        x = F.conv_transpose1d(lr(x), wt, b, stride=u, padding=(k - u) // 2)
        total = 0
        for j, ds in enumerate(cfg['resblock_dilation_sizes']):
            y, p = x, f'resblocks.{i * nk + j}'
            for m, d in enumerate(ds):
                if cfg['resblock'] == '1':
                    y = y + conv(lr(conv(lr(y), f'{p}.convs1.{m}', d)), f'{p}.convs2.{m}')
                else:
                    y = y + conv(lr(y), f'{p}.convs.{m}', d)
            total = total + y
        x = total / nk
    return torch.tanh(conv(torch.where(x > 0, x, 0.01 * x), 'conv_post'))[0, 0]


@pytest.mark.parametrize('name', ['narrow', 'rb2'])
def test_the_restatement_is_the_written_definition(name):
    cfg = R.PRESETS[name]
    ref = R.build(3, torch.float64, **cfg)
    for n in (1, 5):
        mel = R.make_mels([n], 80, n)[1][0]
        with torch.no_grad():
            stages, pre, wav = ref.stages(mel.double())
            want = _definition(ref.state_dict(), cfg, mel)
        assert wav.shape == want.shape == (256 * n,) and len(stages) == 1 + 2 * len(cfg['upsample_rates'])
        assert float((wav - want).abs().max()) <= 1e-13
        assert torch.equal(ref.forward(mel.double().unsqueeze(0))[0, 0], wav)


@pytest.mark.parametrize('k,d', [(3, 1), (3, 5), (5, 6), (7, 3), (7, 12), (11, 1), (11, 5)])
@pytest.mark.parametrize('L', [1, 9, 70])
def test_zero_edge_tap_identity_of_the_residual_convolution(k, d, L):
    """out[t] = b + sum over tap of W[tap] x[t + (tap - (k - 1) / 2) d], rows outside [0, L) zero -- what the kernel forms
    from a tile staged with d (k - 1) / 2 halo rows: LDS row i = row t0 - halo + i, output row r takes rows r + tap d"""
    gen = torch.Generator().manual_seed(100 * k + d + L)
    C = 4
    x = torch.randn(C, L, dtype=torch.float64, generator=gen)
    w = torch.randn(C, C, k, dtype=torch.float64, generator=gen)
    b = torch.randn(C, dtype=torch.float64, generator=gen)
    halo = d * (k - 1) // 2
    want = F.conv1d(x.unsqueeze(0), w, b, dilation=d, padding=halo)[0]
    assert want.shape == (C, L)
    tile = torch.zeros(C, L + 2 * halo, dtype=torch.float64)
    tile[:, halo:halo + L] = x
    got = b[:, None] + sum(w[:, :, tap] @ tile[:, tap * d:tap * d + L] for tap in range(k))
    assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize('k,d', [(3, 1), (3, 5), (7, 3), (11, 5)])
@pytest.mark.parametrize('L', [1, 9, 70])
def test_pair_identity_the_intermediate_is_zero_outside_the_item(k, d, L):
    """the fused pair forms the first convolution on (k - 1) / 2 rows beyond either end of its output rows; those of
    them that lie outside [0, L) must be ZERO (the second convolution pads the first one's output), not bias + taps"""
    gen = torch.Generator().manual_seed(100 * k + d + L)
    C = 4
    lr = lambda t: F.leaky_relu(t, 0.1)                                                  # noqa: E731
    x = torch.randn(C, L, dtype=torch.float64, generator=gen)
    w1, w2 = (torch.randn(C, C, k, dtype=torch.float64, generator=gen) for _ in range(2))
    b1, b2 = (torch.randn(C, dtype=torch.float64, generator=gen) for _ in range(2))
    h2 = (k - 1) // 2
    h1 = d * h2
    want = x + F.conv1d(lr(F.conv1d(lr(x).unsqueeze(0), w1, b1, dilation=d, padding=h1)), w2, b2, padding=h2)[0]
    tile = torch.zeros(C, L + 2 * (h1 + h2), dtype=torch.float64)                        # row i = item row i - h1 - h2
    tile[:, h1 + h2:h1 + h2 + L] = x
    M_ = L + 2 * h2                                                                      # mid row m = item row m - h2
    mid = b1[:, None] + sum(w1[:, :, tap] @ lr(tile[:, tap * d:tap * d + M_]) for tap in range(k))
    wrong = b2[:, None] + sum(w2[:, :, tap] @ lr(mid[:, tap:tap + L]) for tap in range(k)) + x
    mid[:, :h2] = 0
    mid[:, h2 + L:] = 0
    got = b2[:, None] + sum(w2[:, :, tap] @ lr(mid[:, tap:tap + L]) for tap in range(k)) + x
    assert float((got - want).abs().max()) < 1e-12
    assert float((wrong - want).abs().max()) > 1e-3                                      # the mask is not a no-op
    assert M.pair_is_fused(32, k, d) and not M.pair_is_fused(128, k, d) and M.pair_is_fused(64, k, d) == (k == 3)


def test_from_config_takes_a_dict_or_a_json_file(tmp_path):
    cfg = dict(R.V3, learning_rate=2e-4, segment_size=8192, num_gpus=0)                  # the published file has more keys
    a = M.HiFiGAN.from_config(cfg)
    path = tmp_path / 'config.json'
    path.write_text(json.dumps(cfg))
    b = M.HiFiGAN.from_config(path)
    for v in (a, b):
        assert v.resblock == '2' and v.upsample_rates == (8, 8, 4) and v.hop_length == 256 and len(v.state_dict()) == 69
        assert v.resblock_dilation_sizes == ((1, 2), (2, 6), (3, 12)) and v.widths == (128, 64, 32)


@pytest.mark.parametrize('layout', ['bare', 'generator'])
def test_checkpoint_round_trip_in_both_layouts_on_a_synthetic_file(tmp_path, layout):
    state = R.build(3, **R.V2).state_dict()
    path = tmp_path / f'{layout}.pt'
    torch.save(state if layout == 'bare' else {'generator': state}, path)
    torch.manual_seed(99)
    voc = M.HiFiGAN.from_checkpoint(path, config=R.V2)
    got = voc.state_dict()
    assert all(torch.equal(got[k], state[k]) for k in state)
    broken = dict(state)
    del broken['resblocks.4.convs2.1.bias']
    torch.save(broken, path)
    with pytest.raises(FtError, match='convs2.1.bias'):
        M.HiFiGAN.from_checkpoint(path, config=R.V2)
    torch.save(dict(state, extra=torch.zeros(1)), path)
    with pytest.raises(FtError, match='unknown.*extra'):
        M.HiFiGAN.from_checkpoint(path, config=R.V2)
    torch.save(state, path)
    with pytest.raises(FtError, match='does not fit the configuration'):                 # the default configuration is V1
        M.HiFiGAN.from_checkpoint(path)


def test_every_constructor_refusal():
    ok = dict(R.V2)
    M.HiFiGAN(**ok)
    M.HiFiGAN(**dict(ok, resblock=1))
    M.HiFiGAN(**dict(R.V3, resblock_kernel_sizes=(3, 5, 9), resblock_dilation_sizes=((1, 2), (2, 6), (3, 10))))     # halo 40
    for change, match in [
            (dict(resblock='3'), "'1' or '2'"),
            (dict(upsample_kernel_sizes=(16, 16, 4, 3)), 'kernel = 2 rate'),
            (dict(upsample_rates=(8, 8, 2, 3), upsample_kernel_sizes=(16, 16, 4, 6)), 'kernel = 2 rate'),
            (dict(upsample_rates=(8, 8, 4)), 'one upsample kernel size per upsample rate'),
            (dict(resblock_kernel_sizes=(3, 7, 10)), 'odd and at most 11'),
            (dict(resblock_kernel_sizes=(3, 7, 13)), 'odd and at most 11'),
            (dict(resblock_kernel_sizes=(3, 7)), 'one non-empty dilation list'),
            (dict(resblock_dilation_sizes=((1, 3, 5), (1, 3, 5), (1, 3, 9))), 'halo of at most 40'),
            (dict(resblock_dilation_sizes=((1, 3, 5), (1, 3, 0), (1, 3, 5))), 'halo of at most 40'),
            (dict(num_mels=81), 'multiples of 8'),
            (dict(num_mels=136), 'multiples of 8'),
            (dict(upsample_initial_channel=120), 'multiples of 8'),                       # 120 >> 4 = 7
            (dict(upsample_initial_channel=1024), 'multiples of 8'),                      # above 512 at conv_pre
            (dict(upsample_initial_channel=512, upsample_rates=(8, 8), upsample_kernel_sizes=(16, 16)), 'multiples of 8'),
    ]:
        with pytest.raises(FtError, match=match):
            M.HiFiGAN(**dict(ok, **change))
    with pytest.raises(FtError, match='parameter containers'):
        M.HiFiGAN(**ok).resblocks[0](torch.zeros(1, 64, 4))


def test_every_validation_error_is_raised_without_a_device():
    voc = M.HiFiGAN.v2().eval()
    ok = torch.zeros(2, 80, 5)
    lens = torch.tensor([5, 3])
    with torch.no_grad():
        with pytest.raises(FtError, match='float32'):
            voc.inference_batch(ok.double(), lens)
        with pytest.raises(FtError, match=r'\[B, n_mels, Tmax\]'):
            voc.inference_batch(ok[0], lens)
        with pytest.raises(FtError, match='80 mel channels'):
            voc.inference_batch(torch.zeros(2, 8, 5), lens)
        with pytest.raises(FtError, match='empty batch'):
            voc.inference_batch(torch.zeros(0, 80, 5), torch.zeros(0, dtype=torch.int64))
        with pytest.raises(FtError, match='empty batch'):
            voc.inference_batch(torch.zeros(2, 80, 0), lens)
        for bad in (torch.tensor([5, 0]), torch.tensor([6, 1]), torch.tensor([-1, 2])):
            with pytest.raises(FtError, match='mel_len must be in'):
                voc.inference_batch(ok, bad)
        with pytest.raises(FtError, match='int64'):
            voc.inference_batch(ok, lens.to(torch.int32))
        with pytest.raises(FtError, match='int64'):
            voc.inference_batch(ok, [5, 3])
        with pytest.raises(FtError, match='one mel'):
            voc.inference(ok)
        with pytest.raises(FtError, match='HIP'):                      # a CPU-placed model: all valid but the device
            voc.inference_batch(ok, lens)
        with pytest.raises(FtError, match='HIP'):
            voc.forward(ok)
        with pytest.raises(FtError, match='HIP'):
            voc.inference(ok[0])
    with pytest.raises(FtError, match='no autograd'):                  # parameters require grad and grad mode is on
        voc.inference_batch(ok, lens)
    for p in voc.parameters():
        p.requires_grad_(False)
    with pytest.raises(FtError, match='no autograd'):
        voc.forward(ok.clone().requires_grad_(True))


@pytest.mark.parametrize('name', ['full', 'narrow', 'rb2'])
def test_the_fixture_is_usable(name):
    """seed 0, default initialisation, the GPU tests' lengths: in float64 max |pre-tanh| < 1 (no saturated tanh hides
    an error) and the wav's standard deviation over the valid samples is at least 1e4 times the end-to-end tolerance of
    the GPU test, twice the stock fp32 CPU route's own error against float64"""
    cfg = R.PRESETS[name]
    ref64, ref32 = R.build(0, torch.float64, **cfg), R.build(0, **cfg)
    _, items = R.make_mels(LENS, 80, 11)
    with torch.no_grad():
        got = [ref64.stages(m.double()) for m in items]
        e_cpu = max(float((ref32.stages(m)[2].double() - g[2]).abs().max()) for m, g in zip(items, got))
    top = max(float(g[1].abs().max()) for g in got)
    std = float(torch.cat([g[2] for g in got]).std())
    print(f'{name}: pre-tanh max {top:.3f}, wav std {std:.3e}, stock fp32 error {e_cpu:.3e}, std / tolerance {std / (2 * e_cpu):.3g}')
    assert top < 1.0
    assert std >= 1e4 * 2 * e_cpu
