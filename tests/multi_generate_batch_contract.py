"""The contract of the speaker-conditioned generate_batch (MultiForwardTacotron, MultiFastPitch), on top of
generate_batch_contract.py: each item of a ragged batch gets what generate() gives it alone WITH ITS OWN SPEAKER ROW, and
`pitch_cond` -- the per-token argmax that conditions the item's dur and pitch predictors -- matches exactly.  A model's
GPU test file keeps its own module fixture

    fx = (fixture, model on the device, x, x_len, speaker_emb, generate_batch of the zero-padded fixture batch on the host)

The fixture batches (B = 5, Tx = 7, x_len [7, 2, 4, 7, 3], five different unit-norm speaker rows) hold no 1-token item:
the reference's generate() raises on one, and so does the package's.  check_one_token_item covers it."""
import pytest
import torch

import generate_batch_contract as base
from generate_batch_contract import BAR, PAD, check_padding, valid  # noqa: F401
from helpers import maxdiff

KEYS = base.KEYS


class Bound:
    """model with its speaker rows bound: what generate_batch_contract's checks call as m.generate_batch(x, x_len, ...)"""

    def __init__(self, m, semb):
        self.m, self.semb = m, semb

    def generate_batch(self, x, x_len, **kw):
        return self.m.generate_batch(x, x_len, self.semb, **kw)


def _base_fx(fx):
    G, m, x, x_len, semb, out = fx
    return G, Bound(m, semb), x, x_len, out


def _unit_rows(n, S, seed):
    s = torch.randn(n, S, generator=torch.Generator().manual_seed(seed))
    return s / s.norm(dim=1, keepdim=True)


def check_pitch_cond_padding(out, b, L):
    assert bool((out['pitch_cond'][b, L:] == 0).all()), (b, 'pitch_cond must be 0 past the length')


def check_golden(fx, cfg):
    G, m, x, x_len, semb, out = fx
    B, Tx = x.shape
    frames = [G[f'item{b}/mel'].shape[2] for b in range(B)]
    assert out['mel_len'].dtype == torch.int64 and out['mel_len'].tolist() == frames
    Tm = max(frames)
    assert out['mel'].shape == out['mel_post'].shape == (B, cfg['n_mels'], Tm)
    assert out['dur'].shape == (B, Tx) and out['pitch'].shape == out['energy'].shape == (B, 1, Tx)
    assert out['pitch_cond'].shape == (B, Tx) and out['pitch_cond'].dtype == torch.int64
    assert set(out) == {'mel', 'mel_post', 'mel_len', 'dur', 'pitch', 'energy', 'pitch_cond'}
    for b in range(B):
        L, n = int(x_len[b]), frames[b]
        assert out['pitch_cond'][b, :L].tolist() == G[f'item{b}/pitch_cond'].reshape(-1).tolist(), b
        for k, v in valid(out, b, L, n).items():
            d = maxdiff(v, G[f'item{b}/{k}'])
            print(f'item {b} {k}: {d:.3e}')
            assert d < BAR, (b, k, d)
        check_padding(out, b, L, n)
        check_pitch_cond_padding(out, b, L)


def check_pad_content_is_irrelevant(fx, cfg):
    base.check_pad_content_is_irrelevant(_base_fx(fx), cfg)


def check_neighbours_are_irrelevant(fx, cfg):
    """item 2 in another batch, at another index, beside another speaker: its speaker row moves with it"""
    G, m, x, x_len, semb, out = fx
    alpha = float(G['alpha'])
    b, L = 2, int(x_len[2])
    n = int(out['mel_len'][b])
    in5 = valid(out, b, L, n)
    g = torch.Generator().manual_seed(4)
    x2 = torch.zeros(2, 9, dtype=torch.long)
    x2[0] = torch.randint(1, cfg['num_chars'], (9,), generator=g)
    x2[1, :L] = x[b, :L].cpu()
    s2 = torch.cat([_unit_rows(1, semb.shape[1], 5), semb[b:b + 1].cpu()]).cuda()
    o2 = {k: v.cpu() for k, v in m.generate_batch(x2.cuda(), torch.tensor([9, L]), s2, alpha=alpha).items()}
    assert int(o2['mel_len'][1]) == n
    in2 = valid(o2, 1, L, n)
    alone = m.generate(x[b:b + 1, :L].contiguous(), semb[b:b + 1].contiguous(), alpha=alpha)
    assert alone['mel'].shape[2] == n
    pc = alone['pitch_cond'].reshape(-1).tolist()
    assert out['pitch_cond'][b, :L].tolist() == pc and o2['pitch_cond'][1, :L].tolist() == pc
    for k in KEYS:
        a = alone[k].cpu()
        assert maxdiff(in5[k], a) < BAR and maxdiff(in2[k], a) < BAR and maxdiff(in5[k], in2[k]) < BAR, k


def check_speaker_is_per_item(fx, cfg):
    G, m, x, x_len, semb, out = fx
    alpha = float(G['alpha'])
    B = x.shape[0]
    perm = [3, 1, 2, 0, 4]                        # items 0 and 3 (7 tokens each) trade speakers
    o2 = {k: v.cpu() for k, v in m.generate_batch(x, x_len, semb[perm].contiguous(), alpha=alpha).items()}
    for b in range(B):
        L, n = int(x_len[b]), int(out['mel_len'][b])
        if perm[b] == b:                          # nothing else moves, bit for bit
            assert int(o2['mel_len'][b]) == n
            for k, v in valid(o2, b, L, n).items():
                assert torch.equal(v, valid(out, b, L, n)[k]), (b, k)
            assert torch.equal(o2['pitch_cond'][b], out['pitch_cond'][b])
        else:                                     # and the two items are other utterances now
            assert not torch.equal(o2['pitch'][b], out['pitch'][b]) and not torch.equal(o2['energy'][b], out['energy'][b]), b
            n2 = min(n, int(o2['mel_len'][b]))
            assert not torch.equal(o2['mel'][b, :, :n2], out['mel'][b, :, :n2]), b
    o3 = {k: v.cpu() for k, v in m.generate_batch(x, x_len, semb[0:1].repeat(B, 1).contiguous(), alpha=alpha).items()}
    L, n = int(x_len[0]), int(out['mel_len'][0])
    assert int(o3['mel_len'][0]) == n
    for k, v in valid(o3, 0, L, n).items():
        assert torch.equal(v, valid(out, 0, L, n)[k]), k
    assert torch.equal(o3['pitch_cond'][0], out['pitch_cond'][0])


def check_one_token_item(fx, cfg):
    """generate() raises on a 1-token sentence (the argmax chain squeezes the time axis away); generate_batch gives the
    item the per-token result"""
    G, m, x, x_len, semb, out = fx
    alpha = float(G['alpha'])
    S = semb.shape[1]
    tok = x[0:1, 0:1].contiguous()
    sp = _unit_rows(1, S, 6).cuda()
    with pytest.raises(Exception):
        m.generate(tok, sp, alpha=alpha)
    xa = torch.zeros(2, 7, dtype=torch.long, device='cuda')
    xa[0] = x[3]
    xa[1, 0] = tok[0, 0]
    oa = {k: v.cpu() for k, v in m.generate_batch(xa, torch.tensor([7, 1]), torch.cat([semb[3:4], sp]).contiguous(),
                                                  alpha=alpha).items()}
    xb = torch.zeros(3, 4, dtype=torch.long, device='cuda')
    xb[0, 0] = tok[0, 0]
    xb[1, :4] = x[2, :4]
    xb[2, :2] = x[1, :2]
    ob = {k: v.cpu() for k, v in m.generate_batch(xb, torch.tensor([1, 4, 2]).cuda(),
                                                  torch.cat([sp, semb[2:3], semb[1:2]]).contiguous(), alpha=alpha).items()}
    n = int(oa['mel_len'][1])
    assert n >= 1 and int(ob['mel_len'][0]) == n
    from forwardtacotron_amd import hip
    with torch.no_grad(), hip.gemm_precision(m.matmul_dtype):
        logits = m.pitch_cond_pred.forward_lens(tok, torch.tensor([1]).cuda(), sp).cpu()
    assert logits.shape == (1, 1, 3)
    want = int(torch.argmax(logits[0, 0]))
    assert int(oa['pitch_cond'][1, 0]) == want and int(ob['pitch_cond'][0, 0]) == want
    va, vb = valid(oa, 1, 1, n), valid(ob, 0, 1, n)
    for k in KEYS:
        d = maxdiff(va[k], vb[k])
        print(f'1-token item in two batches, {k}: {d:.3e}')
        assert d < BAR, (k, d)
    check_padding(oa, 1, 1, n)
    check_padding(ob, 0, 1, n)
    check_pitch_cond_padding(oa, 1, 1)


def check_existing_generate_fails_or_differs_in_a_padded_batch(fx, cfg):
    """why the method exists: generate() on the padded batch with B > 1 either raises (the B = 1 argmax chain) or gives a
    short item another result"""
    G, m, x, x_len, semb, out = fx
    try:
        o = m.generate(x, semb, alpha=float(G['alpha']))
    except Exception as e:                        # noqa: BLE001  (IndexError / RuntimeError / FtError, whichever comes first)
        print(f'generate() on the padded batch raises {type(e).__name__}: {e}')
        return
    b, L = 1, int(x_len[1])
    p = o['pitch'].cpu()
    assert p.shape[0] != x.shape[0] or maxdiff(p[b:b + 1, :, :L], G[f'item{b}/pitch']) > BAR


def check_bad_speaker_rows_raise_and_nothing_sticks(fx, cfg):
    from forwardtacotron_amd._lib import FtError
    G, m, x, x_len, semb, out = fx
    alpha = float(G['alpha'])
    B, S = semb.shape
    bad = [semb[:, :S - 1].contiguous(), semb[:B - 1].contiguous(), semb[0].contiguous(), semb.reshape(B, 1, S),
           semb.double(), semb.cpu(), None]
    for t in bad:
        with pytest.raises(FtError, match='speaker_emb must be'):
            m.generate_batch(x, x_len, t, alpha=alpha)
    again = m.generate_batch(x, x_len, semb, alpha=alpha)
    assert set(again) == set(out)
    for k in out:
        assert torch.equal(again[k].cpu(), out[k]), k


def check_user_function_applies_per_token(fx, cfg):
    base.check_user_function_applies_per_token(_base_fx(fx), cfg)


def check_bad_user_function_raises_and_nothing_sticks(fx, cfg):
    base.check_bad_user_function_raises_and_nothing_sticks(_base_fx(fx), cfg)


def check_overlap_switch_is_bit_neutral(fx, cfg, monkeypatch):
    base.check_overlap_switch_is_bit_neutral(_base_fx(fx), cfg, monkeypatch)
