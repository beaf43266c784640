"""GPU: Tacotron.generate (forwardtacotron_amd/tacotron.py, ft_taco_gen_steps) against the reference's generate
(tests/golden/tacotron_generate.npz), against the teacher-forced forward() over its own output at length, and its
invariances: chunking, prefixes, stop arithmetic, the reference's API and its refusals."""
import numpy as np
import pytest
import torch

from forwardtacotron_amd import _lib
from forwardtacotron_amd import hip as H
from forwardtacotron_amd import tacotron as T
from test_tacotron_generate_cpu import CASES, GOLD, gen_case

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _model(gold, name, threshold=None):
    m, cfg, r, steps, x, semb, emb_seed = gen_case(gold, name)
    m = m.cuda()
    if threshold is not None:
        m.stop_threshold.fill_(threshold)
    return m, cfg, r, steps, x.cuda(), semb, emb_seed


def _gen(m, x, steps, semb=None):
    with torch.no_grad():
        out = m.generate(x, semb, steps=steps)
    H.check_rnn_status()
    return out


def _same(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('name', CASES)
def test_generate_matches_reference_fixture(gold, name):
    m, cfg, r, steps, x, semb, emb_seed = _model(gold, name)
    if emb_seed is not None:
        torch.manual_seed(emb_seed)
        semb_arg = None
    else:
        semb_arg = semb.cuda() if semb is not None else None
    out = _gen(m, x, steps, semb_arg)
    p = name + '/'
    assert out[2].shape[0] == int(gold[p + 's_out'])
    for got, key in zip(out, ('mel_outputs', 'linear', 'attn_scores')):
        assert isinstance(got, np.ndarray) and got.shape == gold[p + key].shape, key
        d = float(np.abs(got.astype(np.float64) - gold[p + key]).max())
        assert d <= TOL, (key, d)


def test_long_horizon_matches_teacher_forced_forward(gold):
    """900 free-running steps of the full-size model; the same frames teacher-forced through forward() must give the
    same frames, linear and attention: every step is checked at length without feedback amplification"""
    m, cfg, r, _, x, _, _ = _model(gold, 'f', threshold=-1e9)
    mel, lin, attn = _gen(m, x, 900)
    assert mel.shape == (80, 900) and attn.shape == (900, x.shape[1])
    m.eval()
    with torch.no_grad():
        fm, fl, fa = m({'x': x, 'mel': torch.from_numpy(mel)[None].cuda()})
    torch.cuda.synchronize()
    for got, ref, key in ((fm[0], mel, 'mel'), (fl[0], lin, 'linear'), (fa[0], attn, 'attn')):
        d = float((got.double().cpu() - torch.from_numpy(ref).double()).abs().max())
        assert d <= TOL, (key, d)


def test_chunking_does_not_change_outputs(gold, monkeypatch):
    m, _, _, steps, x, _, _ = _model(gold, 'a')
    outs = []
    for k in (1, 5, 64):
        monkeypatch.setattr(T, 'GEN_CHUNK', k)
        outs.append(_gen(m, x, steps))
    assert _same(outs[0], outs[1]) and _same(outs[0], outs[2])


@pytest.mark.parametrize('name', ['e', 'd'])
def test_stop_at_chunk_boundaries_gives_no_stop_prefix(gold, monkeypatch, name):
    m, _, r, steps, x, _, _ = _model(gold, name)
    s_out = int(gold[name + '/s_out'])
    thr = float(m.stop_threshold)
    m.stop_threshold.fill_(-1e9)
    full = _gen(m, x, steps)
    m.stop_threshold.fill_(thr)
    for k in (s_out - 1, s_out, s_out + 1):
        monkeypatch.setattr(T, 'GEN_CHUNK', k)
        mel, _, attn = _gen(m, x, steps)
        assert attn.shape[0] == s_out, k
        assert np.array_equal(mel, full[0][:, :s_out * r]) and np.array_equal(attn, full[2][:s_out]), k


def test_prefix_property(gold):
    m, _, r, _, x, _, _ = _model(gold, 'b', threshold=-1e9)
    short = _gen(m, x, 20)
    long = _gen(m, x, 40)
    n = short[0].shape[1]
    assert n == 21 and long[0].shape[1] == 42
    assert np.array_equal(short[0], long[0][:, :n]) and np.array_equal(short[2], long[2][:short[2].shape[0]])


@pytest.mark.parametrize('r', [1, 2, 3])
def test_stop_arithmetic(gold, r):
    m, _, _, _, x, _, _ = _model(gold, 'a', threshold=1e3)
    m.r = r
    assert _gen(m, x, 48)[2].shape[0] == 10 // r + 2
    assert _gen(m, x, 5)[2].shape[0] == -(-5 // r)             # steps before the stop point: runs to S
    m.stop_threshold.fill_(-1e9)
    mel, lin, attn = _gen(m, x, 47)
    S = -(-47 // r)
    assert attn.shape[0] == S and mel.shape == (80, S * r) and lin.shape == (80, S * r)


def test_api_behaviour(gold):
    m, cfg, r, steps, x, _, _ = _model(gold, 'a')
    m.train()
    assert all(p.requires_grad for p in m.parameters())
    out = m.generate(x, steps=torch.tensor(steps - 20) + 20)      # grad enabled, 0-d tensor steps (the trainer's call)
    assert m.training and all(mod.training for mod in m.modules())
    assert [o.shape for o in out] == [(80, steps), (80, steps), (steps, x.shape[1])]
    assert all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in out)
    assert _same(out, m.generate(x.cpu(), steps=steps))             # host-side x, and a second call
    # align / forward are unchanged by a generate in between
    mel = torch.randn(1, 80, 30, device='cuda')
    m.eval()
    with torch.no_grad():
        before = m({'x': x, 'mel': mel})
        m.generate(x, steps=17)
        m.eval()
        after = m({'x': x, 'mel': mel})
        align = m.align({'x': x, 'mel': mel})
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and torch.equal(align, before[2])


def test_default_speaker_emb_is_seeded_torch_rand(gold):
    m, cfg, r, steps, x, _, _ = _model(gold, 'c')
    torch.manual_seed(123)
    drawn = _gen(m, x, steps)
    torch.manual_seed(123)
    semb = torch.rand((1, cfg['speaker_emb_dim']))
    explicit = _gen(m, x, steps, semb)
    assert _same(drawn, explicit)


def test_refusals(gold):
    m, _, _, _, x, _, _ = _model(gold, 'a')
    with pytest.raises(_lib.FtError, match='generate'):
        m.cpu().generate(x.cpu(), steps=10)
    m.cuda()
    with pytest.raises(_lib.FtError, match='generate'):
        m.generate(x.repeat(2, 1), steps=10)
    for steps in (0, -3, torch.tensor(0)):
        with pytest.raises(_lib.FtError, match='generate'):
            m.generate(x, steps=steps)
    with pytest.raises(_lib.FtError, match='generate'):
        m.generate(torch.ones(1, 1025, dtype=torch.int64, device='cuda'), steps=10)
    ms, cfg, _, _, xs, _, _ = _model(gold, 'c')
    for bad in (torch.rand(1, cfg['speaker_emb_dim'] + 1), torch.rand(2, cfg['speaker_emb_dim'])):
        with pytest.raises(_lib.FtError, match='generate'):
            ms.generate(xs, bad, steps=10)
    # the C entry checks its own bounds
    assert _lib.query('ft_taco_gen_workspace', 1025, 40, 1) == 0
    assert _lib.query('ft_taco_gen_workspace', 8, 40, 21) == 0
    assert _lib.query('ft_taco_gen_workspace', 8, 0, 1) == 0
    nb = _lib.query('ft_taco_gen_workspace', 8, 40, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device='cuda')
    f = torch.zeros(4096, device='cuda')
    fp = f.data_ptr()
    for Tx, L, r, S, s0, n, size in ((1025, 40, 1, 4, 0, 1, nb), (8, 0, 1, 4, 0, 1, nb), (8, 40, 21, 4, 0, 1, nb),
                                     (8, 40, 1, 4, 3, 2, nb), (8, 40, 1, 4, -1, 1, nb), (8, 40, 1, 4, 0, 1, nb - 1)):
        with pytest.raises(_lib.FtError, match='taco_gen_steps'):
            _lib.call('ft_taco_gen_steps', *(fp,) * 7, 384, *(fp,) * 20, 0.0, *(fp,) * 5, Tx, L, r, S, s0, n,
                      ws.data_ptr(), size, H._stream())
