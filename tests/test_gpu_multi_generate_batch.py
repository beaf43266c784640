"""GPU: MultiForwardTacotron.generate_batch -- every item of a ragged batch gets what generate() gives it alone with its
own speaker row.  The shared contract is tests/multi_generate_batch_contract.py."""
import pytest
import torch

import multi_generate_batch_contract as contract
from helpers import TINY_MULTI, load_npz, maxdiff, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    """(fixture, model on the device, x, x_len, speaker_emb, generate_batch of the zero-padded fixture batch) -- once"""
    from forwardtacotron_amd.multi_model import MultiForwardTacotron
    G = load_npz('multi_generate_batch.npz')
    m = MultiForwardTacotron(**TINY_MULTI)
    m.load_state_dict(sub(G, 'sd/'))
    m = m.cuda()
    assert not m.checks_tokens
    x = torch.from_numpy(G['x']).cuda()
    x_len = torch.from_numpy(G['x_len'])
    semb = torch.from_numpy(G['speaker_emb']).cuda()
    out = m.generate_batch(x, x_len, semb, alpha=float(G['alpha']))
    torch.cuda.synchronize()
    return G, m, x, x_len, semb, {k: v.cpu() for k, v in out.items()}


def test_golden(fx):
    contract.check_golden(fx, TINY_MULTI)
    assert fx[5]['mel'].data_ptr() != fx[5]['mel_post'].data_ptr() and not torch.equal(fx[5]['mel'], fx[5]['mel_post'])


def test_pad_content_is_irrelevant(fx):
    contract.check_pad_content_is_irrelevant(fx, TINY_MULTI)


def test_neighbours_are_irrelevant(fx):
    contract.check_neighbours_are_irrelevant(fx, TINY_MULTI)


def test_speaker_is_per_item(fx):
    contract.check_speaker_is_per_item(fx, TINY_MULTI)


def test_one_token_item(fx):
    contract.check_one_token_item(fx, TINY_MULTI)


def test_existing_generate_fails_or_differs_in_a_padded_batch(fx):
    contract.check_existing_generate_fails_or_differs_in_a_padded_batch(fx, TINY_MULTI)


def test_bad_speaker_rows_raise_and_nothing_sticks(fx):
    contract.check_bad_speaker_rows_raise_and_nothing_sticks(fx, TINY_MULTI)


def test_user_function_applies_per_token(fx):
    contract.check_user_function_applies_per_token(fx, TINY_MULTI)


def test_bad_user_function_raises_and_nothing_sticks(fx):
    contract.check_bad_user_function_raises_and_nothing_sticks(fx, TINY_MULTI)


def test_overlap_switch_is_bit_neutral(fx, monkeypatch):
    contract.check_overlap_switch_is_bit_neutral(fx, TINY_MULTI, monkeypatch)


def test_production_widths_vs_per_item_generate():
    """data.MULTISPEAKER_MODEL against its own generate() per item, on the same GPU (there is no CPU oracle of this
    model's generate); the bar is that of the other production-width tests"""
    from forwardtacotron_amd import data, hip
    from forwardtacotron_amd.multi_model import MultiForwardTacotron
    cfg = dict(data.MULTISPEAKER_MODEL)
    x_len = [40, 13, 2, 27, 40]
    alpha = 0.9
    torch.manual_seed(0)
    m = MultiForwardTacotron(**cfg)
    with torch.no_grad():                           # as test_gpu_generate_batch.py::test_production_widths_vs_oracle_per_item
        m.dur_pred.lin.weight.mul_(30.0)
        m.dur_pred.lin.bias.fill_(2.5)
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(5, 40, dtype=torch.long)
    for b, L in enumerate(x_len):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    semb = torch.randn(5, cfg['speaker_emb_dims'], generator=g)
    semb = (semb / semb.norm(dim=1, keepdim=True)).cuda()
    m, x = m.cuda(), x.cuda()
    out = {k: v.cpu() for k, v in m.generate_batch(x, torch.tensor(x_len), semb, alpha=alpha).items()}
    hip.check_rnn_status()
    for b, L in enumerate(x_len):
        alone = m.generate(x[b:b + 1, :L].contiguous(), semb[b:b + 1].contiguous(), alpha=alpha)
        n = alone['mel'].shape[2]
        assert int(out['mel_len'][b]) == n, b
        assert out['pitch_cond'][b, :L].tolist() == alone['pitch_cond'].reshape(-1).tolist(), b
        for k, v in contract.valid(out, b, L, n).items():
            d = maxdiff(v, alone[k].cpu())
            print(f'item {b} {k}: {d:.3e}')
            assert d < 1e-4, (b, k, d)
        contract.check_padding(out, b, L, n)
        contract.check_pitch_cond_padding(out, b, L)
