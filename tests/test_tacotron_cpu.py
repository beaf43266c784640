"""CPU: the drop-in Tacotron (forwardtacotron_amd/tacotron.py) has the reference's state_dict layout and seed-identical
initialisation (tests/golden/tacotron.npz, made from models/tacotron.py), refuses configurations the reference cannot
run, and the float64 restatement of its teacher-forced forward (tests/taco_cpu.py) reproduces the reference's outputs."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import taco_cpu as R
from forwardtacotron_amd import _lib
from forwardtacotron_amd.tacotron import Tacotron

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'tacotron.npz')
CASES = ('a', 'b', 'c', 'd')
# configs/singlespeaker.yaml of the reference (tacotron.model), num_chars = len(phonemes), n_mels = 80
FULL_CFG = dict(embed_dims=256, num_chars=135, encoder_dims=128, decoder_dims=256, n_mels=80, postnet_dims=128,
                encoder_k=16, lstm_dims=512, postnet_k=8, num_highways=4, dropout=0.5, stop_threshold=-11.,
                speaker_emb_dim=0)


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def case_model(g, name):
    """the case's model: seed-init Tacotron with the fixture's BatchNorm statistics, eval mode"""
    p = name + '/'
    cfg = json.loads(str(g[p + 'cfg']))
    torch.manual_seed(int(g[p + 'seed']))
    m = Tacotron(**cfg)
    m.r = int(g[p + 'r'])
    bn = {k[len(p) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p + 'bn/')}
    m.load_state_dict(bn, strict=False)
    return m.eval(), cfg


def case_batch(g, name):
    p = name + '/'
    return {k: torch.from_numpy(g[p + k]) for k in ('x', 'mel', 'speaker_emb', 'x_len', 'mel_len')}


@pytest.mark.parametrize('name', CASES)
def test_state_dict_layout_matches_reference(gold, name):
    m, _ = case_model(gold, name)
    sd = m.state_dict()
    keys = [k.decode() for k in gold[name + '/sd_keys']]
    assert list(sd.keys()) == keys
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [s.decode() for s in gold[name + '/sd_shapes']]
    if name == 'd':
        assert json.loads(str(gold['d/cfg'])) == FULL_CFG
        assert len(keys) == 254
        assert sum(p.numel() for p in m.parameters()) == 11167072


@pytest.mark.parametrize('name', CASES)
def test_seed_init_is_bit_identical(gold, name):
    p = name + '/'
    torch.manual_seed(int(gold[p + 'seed']))
    m = Tacotron(**json.loads(str(gold[p + 'cfg'])))
    m.r = int(gold[p + 'r'])
    got = [hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest() for v in m.state_dict().values()]
    assert got == [s.decode() for s in gold[p + 'sd_sha256']]


def test_buffers_r_and_step():
    m = Tacotron(**json.loads(str(np.load(GOLD)['a/cfg'])))
    assert m.r == 1 and m.decoder.r.dtype == torch.int32
    m.r = 7
    assert m.r == 7 and 'decoder.r' in m.state_dict()
    assert m.get_step() == 0
    m.reset_step()
    assert m.get_step() == 1
    assert float(m.stop_threshold) == -11.


@pytest.mark.parametrize('bad', [dict(decoder_dims=128), dict(encoder_dims=64), dict(n_mels=40)])
def test_unsupported_dims_refused(gold, bad):
    cfg = dict(json.loads(str(gold['a/cfg'])), **bad)
    with pytest.raises(_lib.FtError):
        Tacotron(**cfg)


def test_generate_refused(gold):
    m = Tacotron(**json.loads(str(gold['a/cfg'])))
    with pytest.raises(_lib.FtError, match='generate'):
        m.generate(torch.zeros(1, 5, dtype=torch.int64))


def test_forward_refuses_cpu_tensors(gold):
    m, _ = case_model(gold, 'a')
    with torch.no_grad(), pytest.raises(_lib.FtError):
        m(case_batch(gold, 'a'))


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_reference(gold, name):
    m, cfg = case_model(gold, name)
    P = {k: v.double() if v.is_floating_point() else v for k, v in m.state_dict().items()}
    p = name + '/'
    with torch.no_grad():
        mel, lin, attn = R.forward(P, case_batch(gold, name), cfg, int(gold[p + 'r']))
    for got, key in ((mel, 'mel_outputs'), (lin, 'linear'), (attn, 'attn_scores')):
        ref = gold[p + key]
        assert got.shape == ref.shape, key
        assert float(np.abs(got.numpy() - ref).max()) < 1e-5, key
