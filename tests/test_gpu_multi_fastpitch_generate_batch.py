"""GPU: MultiFastPitch.generate_batch -- every item of a ragged batch gets what generate() gives it alone with its own
speaker row.  The shared contract is tests/multi_generate_batch_contract.py; the wide-head attention kernel under the
production widths is tested alone in test_gpu_attn_lens_wide.py."""
import os

import numpy as np
import pytest
import torch

import multi_generate_batch_contract as contract
from multi_generate_batch_contract import KEYS
from helpers import ROOT, TINY_MFP, fp_state, load_npz, maxdiff

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    """(fixture, model on the device, x, x_len, speaker_emb, generate_batch of the zero-padded fixture batch) -- once"""
    from forwardtacotron_amd.multi_fastpitch import MultiFastPitch
    G = load_npz('multi_fastpitch_generate_batch.npz')
    m = MultiFastPitch(**TINY_MFP)
    m.load_state_dict(fp_state(G, 'sd/'))
    m = m.cuda()
    assert m.checks_tokens
    x = torch.from_numpy(G['x']).cuda()
    x_len = torch.from_numpy(G['x_len'])
    semb = torch.from_numpy(G['speaker_emb']).cuda()
    out = m.generate_batch(x, x_len, semb, alpha=float(G['alpha']))
    torch.cuda.synchronize()
    return G, m, x, x_len, semb, {k: v.cpu() for k, v in out.items()}


def test_golden(fx):
    contract.check_golden(fx, TINY_MFP)
    assert torch.equal(fx[5]['mel'], fx[5]['mel_post'])              # one tensor, as in generate


def test_pad_content_is_irrelevant(fx):
    contract.check_pad_content_is_irrelevant(fx, TINY_MFP)


def test_neighbours_are_irrelevant(fx):
    contract.check_neighbours_are_irrelevant(fx, TINY_MFP)


def test_speaker_is_per_item(fx):
    contract.check_speaker_is_per_item(fx, TINY_MFP)


def test_one_token_item(fx):
    contract.check_one_token_item(fx, TINY_MFP)


def test_existing_generate_fails_or_differs_in_a_padded_batch(fx):
    contract.check_existing_generate_fails_or_differs_in_a_padded_batch(fx, TINY_MFP)


def test_bad_speaker_rows_raise_and_nothing_sticks(fx):
    contract.check_bad_speaker_rows_raise_and_nothing_sticks(fx, TINY_MFP)


def test_user_function_applies_per_token(fx):
    contract.check_user_function_applies_per_token(fx, TINY_MFP)


def test_bad_user_function_raises_and_nothing_sticks(fx):
    contract.check_bad_user_function_raises_and_nothing_sticks(fx, TINY_MFP)


def test_overlap_switch_is_bit_neutral(fx, monkeypatch):
    contract.check_overlap_switch_is_bit_neutral(fx, TINY_MFP, monkeypatch)


def test_zero_token_inside_a_sentence_raises(fx):
    from forwardtacotron_amd._lib import FtError
    G, m, x, x_len, semb, out = fx
    x2 = x.clone()
    x2[3, 2] = 0                                  # item 3 has 7 tokens
    for xl in (x_len, x_len.cuda()):
        with pytest.raises(FtError, match='token id 0'):
            m.generate_batch(x2, xl, semb, alpha=float(G['alpha']))
    again = m.generate_batch(x, x_len, semb, alpha=float(G['alpha']))       # the flag does not stick
    assert torch.equal(again['mel'].cpu(), out['mel'])


# ---- production widths: head width 192 / 196 in the predictors, 256 in the trunk -------------------------------------
X_LEN = [40, 13, 2, 27, 40]
ALPHA = 0.9
MARGIN = 1e-3
FP32_SEED, BF16_SEED = 0, 0             # token / speaker seeds, picked on the CPU oracle so that the asserted margins hold
PC_BIAS = (-0.75, -1.5, 0.0)        # bf16 test: the pitch_cond head's bias, which sets the classes apart (two of them occur)


def _production(dur_scale, dur_bias, seed, pc_bias=None):
    """data.MULTI_FASTPITCH_MODEL with one layer per stack (seconds, not minutes)
    -> (cfg, model on the CPU, state, tokens, speaker rows)"""
    from forwardtacotron_amd import data
    from forwardtacotron_amd.multi_fastpitch import MultiFastPitch
    cfg = dict(data.MULTI_FASTPITCH_MODEL, durpred_layers=1, pitch_layers=1, energy_layers=1, pitch_cond_layers=1,
               prenet_layers=1, postnet_layers=1)
    torch.manual_seed(0)
    m = MultiFastPitch(**cfg)
    with torch.no_grad():
        m.dur_pred.lin.weight.mul_(dur_scale)
        m.dur_pred.lin.bias.fill_(dur_bias)
        if pc_bias is not None:
            m.pitch_cond_pred.lin.bias.copy_(torch.tensor(pc_bias))
    P = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(len(X_LEN), max(X_LEN), dtype=torch.long)
    for b, L in enumerate(X_LEN):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    semb = torch.randn(len(X_LEN), cfg['speaker_emb_dims'], generator=g)
    return cfg, m, P, x, semb / semb.norm(dim=1, keepdim=True)


def _oracle_item(P, cfg, xb, sb):
    """the CPU oracle on one item -> (pitch_cond logits [T,K], raw dur_hat [T]) as float64 arrays"""
    from oracle import fp_oracle as O
    with torch.no_grad():
        logits = O.multi_series_predictor(xb, sb, None, P, 'pitch_cond_pred.', cfg['pitch_cond_n_heads'],
                                          cfg['pitch_cond_layers'], ALPHA)
        pc = torch.argmax(logits, dim=2)
        d = O.multi_series_predictor(xb, sb, None, P, 'dur_pred.', cfg['durpred_n_heads'], cfg['durpred_layers'], ALPHA,
                                     x_cond=pc)
    return logits[0].double().numpy(), d.reshape(-1).double().numpy()


def _to_grid(d, offset):
    """distance of every entry to the nearest integer + offset"""
    return np.abs((d - offset) - np.round(d - offset))


def _logit_gap(logits):
    s = np.sort(logits, axis=-1)
    return s[..., -1] - s[..., -2]


def test_production_widths_vs_oracle_per_item():
    from oracle import fp_oracle as O
    cfg, m, P, x, semb = _production(3.0, 4.0, FP32_SEED)
    want = []
    for b, L in enumerate(X_LEN):
        xb, sb = x[b:b + 1, :L].clone(), semb[b:b + 1].clone()
        logits, d = _oracle_item(P, cfg, xb, sb)
        assert _to_grid(d, 0.0).min() >= MARGIN and _to_grid(d, 0.5).min() >= MARGIN, b
        assert _logit_gap(logits).min() >= MARGIN, b
        want.append(O.multi_generate(P, xb, sb, cfg, alpha=ALPHA))
    assert max(w['mel'].shape[2] for w in want) > 128      # the frame side spans more than one query workgroup
    m = m.cuda()
    assert m.matmul_dtype == 'fp32'
    out = {k: v.cpu() for k, v in m.generate_batch(x.cuda(), torch.tensor(X_LEN), semb.cuda(), alpha=ALPHA).items()}
    assert out['mel_len'].tolist() == [w['mel'].shape[2] for w in want]
    for b, L in enumerate(X_LEN):
        n = want[b]['mel'].shape[2]
        assert out['pitch_cond'][b, :L].tolist() == want[b]['pitch_cond'].reshape(-1).tolist(), b
        for k, v in contract.valid(out, b, L, n).items():
            d = maxdiff(v, want[b][k])
            print(f'item {b} {k}: {d:.3e}')
            assert d < 1e-4, (b, k, d)              # test_gpu_fastpitch_generate_batch.py::test_production_widths_vs_oracle_per_item
        contract.check_padding(out, b, L, n)
        contract.check_pitch_cond_padding(out, b, L)


def test_production_widths_bf16_vs_per_item_generate():
    """bf16 mode.  The wide-head kernel has no bit-equal twin in generate() (whose attention is the unfused route at these
    widths), so the yardstick is fp32 generate() per item: err(bf16 generate_batch item) <= 2 x err(bf16 generate alone)
    per key -- the same operand rounding, summed in another order.  That needs fp32 and bf16 to agree on every pitch_cond
    class and every rounded duration: the durations are kept narrow (dur_pred.lin scaled by 0.12 around a bias of 2.0),
    the pitch_cond head is biased so that its classes lie well apart, and the seed is picked on the CPU oracle so that
    no item has a dur_hat within 0.05 of a rounding boundary or a logit gap below 0.05 -- asserted, zero skipped."""
    cfg, m, P, x, semb = _production(0.12, 2.0, BF16_SEED, PC_BIAS)
    skipped = []
    for b, L in enumerate(X_LEN):
        logits, d = _oracle_item(P, cfg, x[b:b + 1, :L].clone(), semb[b:b + 1].clone())
        if _to_grid(d, 0.5).min() < 0.05 or np.trunc(d).sum() <= 0 or _logit_gap(logits).min() < 0.05:
            print(f'item {b} skipped: fp32 dur_hat or pitch_cond logits too close to a decision boundary')
            skipped.append(b)
    assert len(skipped) == 0, 'the seed was chosen so that no item needs skipping'
    m = m.cuda()
    xd, sd = x.cuda(), semb.cuda()
    ref, alone = [], []
    for mode, dst in (('fp32', ref), ('bf16', alone)):
        m.matmul_dtype = mode
        for b, L in enumerate(X_LEN):
            dst.append({k: v.cpu() for k, v in m.generate(xd[b:b + 1, :L].contiguous(), sd[b:b + 1].contiguous(),
                                                          alpha=ALPHA).items()})
    for b in range(len(X_LEN)):
        assert torch.equal(ref[b]['pitch_cond'], alone[b]['pitch_cond']), b
        assert ref[b]['mel'].shape == alone[b]['mel'].shape and \
            torch.equal((ref[b]['dur'] + 0.5).long(), (alone[b]['dur'] + 0.5).long()), b
    out = {k: v.cpu() for k, v in m.generate_batch(xd, torch.tensor(X_LEN), sd, alpha=ALPHA).items()}     # (bf16)
    worst = {k: 0.0 for k in KEYS}
    failed = []
    for b, L in enumerate(X_LEN):
        n = ref[b]['mel'].shape[2]
        assert int(out['mel_len'][b]) == n, b
        assert out['pitch_cond'][b, :L].tolist() == ref[b]['pitch_cond'].reshape(-1).tolist(), b
        for k, v in contract.valid(out, b, L, n).items():
            e_batch, e_alone = maxdiff(v, ref[b][k]), maxdiff(alone[b][k], ref[b][k])
            print(f'bf16 item {b} {k}: generate_batch {e_batch:.3e}, generate alone {e_alone:.3e} off fp32 generate, '
                  f'ratio {e_batch / max(e_alone, 1e-30):.2f}')
            worst[k] = max(worst[k], e_batch / max(e_alone, 1e-30))
            if e_batch > 2 * e_alone:
                failed.append((b, k, e_batch, e_alone))
        contract.check_padding(out, b, L, n)
        contract.check_pitch_cond_padding(out, b, L)
    print('worst ratio per key: ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    assert not failed, failed
