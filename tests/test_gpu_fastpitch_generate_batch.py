"""GPU: FastPitch.generate_batch -- every item of a ragged batch gets what generate() gives it alone.  The shared
contract is tests/generate_batch_contract.py; the length-aware attention kernel under it is tested alone in test_gpu_attn_lens.py."""
import numpy as np
import pytest
import torch

import generate_batch_contract as contract
from generate_batch_contract import KEYS
from helpers import TINY_FP, fp_state, load_npz, maxdiff

pytestmark = pytest.mark.gpu


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


def test_golden(fx):
    contract.check_golden(fx, TINY_FP)


def test_pad_content_is_irrelevant(fx):
    contract.check_pad_content_is_irrelevant(fx, TINY_FP)


def test_neighbours_are_irrelevant(fx):
    contract.check_neighbours_are_irrelevant(fx, TINY_FP)


def test_existing_generate_differs_in_a_padded_batch(fx):
    """why the method exists: generate() runs the predictors and the postnet without any padding mask, so in the
    zero-padded batch a short item's own tokens attend to the pad rows and its convolutions read them"""
    contract.check_existing_generate_differs_in_a_padded_batch(fx, TINY_FP)


def test_user_function_applies_per_token(fx):
    contract.check_user_function_applies_per_token(fx, TINY_FP)


def test_bad_user_function_raises_and_nothing_sticks(fx):
    contract.check_bad_user_function_raises_and_nothing_sticks(fx, TINY_FP)


def test_overlap_switch_is_bit_neutral(fx, monkeypatch):
    contract.check_overlap_switch_is_bit_neutral(fx, TINY_FP, monkeypatch)


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
        for k, v in contract.valid(out, b, L, n).items():
            d = maxdiff(v, want[b][k])
            print(f'conv2 k = {conv2_kernel}, item {b} {k}: {d:.3e}')
            assert d < 1e-4, (b, k, d)              # test_gpu_generate_batch.py::test_production_widths_vs_oracle_per_item
        contract.check_padding(out, b, L, n)


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
        for k, v in contract.valid(out, b, L, n).items():
            d = maxdiff(v, alone[k].cpu())
            print(f'bf16 item {b} {k}: {d:.3e} (bar {bar[k]:.3e})')
            assert d <= bar[k], (b, k, d, bar[k])
        contract.check_padding(out, b, L, n)
