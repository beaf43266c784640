"""CPU: the float64 restatement of Tacotron.generate (tests/taco_gen_cpu.py) reproduces the reference's generate
(tests/golden/tacotron_generate.npz, made from models/tacotron.py), stop step included, and every fixture model is the
seed-identical initialisation of forwardtacotron_amd.tacotron.Tacotron."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import taco_gen_cpu as G
from forwardtacotron_amd.tacotron import Tacotron

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'tacotron_generate.npz')
CASES = ('a', 'b', 'c', 'c2', 'd', 'e', 'f')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def gen_case(g, name):
    """(model in eval mode, cfg, r, steps, x [1,Tx], speaker_emb or None, emb_seed or None) of a fixture case"""
    p = name + '/'
    cfg = json.loads(str(g[p + 'cfg']))
    torch.manual_seed(int(g[p + 'seed']))
    m = Tacotron(**cfg)
    m.r = int(g[p + 'r'])
    bn = {k[len(p) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + 'bn/')}
    m.load_state_dict(bn, strict=False)
    if p + 'mel_proj_scale' in g.files:
        with torch.no_grad():
            m.decoder.mel_proj.weight.mul_(float(g[p + 'mel_proj_scale']))
    semb = torch.from_numpy(g[p + 'speaker_emb']) if p + 'speaker_emb' in g.files else None
    emb_seed = int(g[p + 'emb_seed']) if p + 'emb_seed' in g.files else None
    return m.eval(), cfg, int(g[p + 'r']), int(g[p + 'steps']), torch.from_numpy(g[p + 'x']), semb, emb_seed


@pytest.mark.parametrize('name', CASES)
def test_seed_init_is_bit_identical(gold, name):
    p = name + '/'
    torch.manual_seed(int(gold[p + 'seed']))
    m = Tacotron(**json.loads(str(gold[p + 'cfg'])))
    m.r = int(gold[p + 'r'])
    sd = m.state_dict()
    assert list(sd.keys()) == [k.decode() for k in gold[p + 'sd_keys']]
    got = [hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in sd.values()]
    assert got == [s.decode() for s in gold[p + 'sd_sha256']]


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_reference_generate(gold, name):
    m, cfg, r, steps, x, semb, emb_seed = gen_case(gold, name)
    if emb_seed is not None:
        torch.manual_seed(emb_seed)
        drawn = torch.rand((1, cfg['speaker_emb_dim']))
        assert torch.equal(drawn, semb)
    P = {k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()}
    p = name + '/'
    with torch.no_grad():
        mel, lin, attn, s_out = G.generate(P, x, cfg, r, steps, semb)
    assert s_out == int(gold[p + 's_out'])
    for got, key in ((mel, 'mel_outputs'), (lin, 'linear'), (attn, 'attn_scores')):
        ref = gold[p + key]
        assert tuple(got.shape) == ref.shape, key
        assert float(np.abs(got.numpy() - ref).max()) < 1e-5, key


def test_fixture_stop_cases(gold):
    """a and f run to S; d stops mid-run; e stops at the first eligible step (s*r > 10)"""
    S = {n: -(-int(gold[n + '/steps']) // int(gold[n + '/r'])) for n in CASES}
    assert int(gold['a/s_out']) == S['a'] and int(gold['f/s_out']) == S['f']
    assert int(gold['b/s_out']) == 14 and gold['b/mel_outputs'].shape == (80, 42)
    assert 12 < int(gold['d/s_out']) < S['d']
    assert int(gold['e/s_out']) == 10 // int(gold['e/r']) + 2
