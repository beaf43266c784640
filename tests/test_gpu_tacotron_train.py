"""GPU: Tacotron.forward_train and its backward against (1) the reference's recorded float32 training step
(tests/golden/tacotron_train.npz, made by tests/golden/make_golden_tacotron_train.py) and (2) float64 autograd through
the training-mode restatement tests/taco_train_cpu.py, which tests/test_tacotron_train_cpu.py ties to the reference.

Bound (tests/test_gpu_full_parity.py:213-218): an array passes when its max error against float64 is at most
max(4 * e_stock, 1e-4 * |x64|inf); e_stock is the error of the same restatement run by stock torch in float32 on the host
(for the fixture cases: the recorded reference values' own distance from float64), |x64|inf the array's OWN scale.  The
teacher's gradients are small (|g|inf of decoder.attn_net.L.weight is 4.9e-5 at the tiny config): a criterion relative
to max(1, |g|inf) would pass an all-zero attention gradient, this one does not.  Every figure is printed (-s).

The masks of the ten random sites are rebuilt on the host from model.last_seeds (tests/dropout_cpu.py)."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import taco_train_cpu as TT  # noqa: E402
from make_golden_tacotron import FULL as FULL_CFG, TINY, make_batch  # noqa: E402
from make_golden_tacotron_train import sample, sd_sha256  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, 'golden', 'tacotron_train.npz')
TINY_CASES = {
    'tiny-r3': dict(cfg=TINY, r=3, seed=1, x_len=[9, 12, 6], mel_len=[20, 27, 14]),
    'tiny-spk16-r2': dict(cfg=dict(TINY, speaker_emb_dim=16), r=2, seed=2, x_len=[7, 11, 10], mel_len=[25, 16, 30]),
    'tiny-r1-long': dict(cfg=TINY, r=1, seed=3, x_len=[33, 70, 40], mel_len=[120, 90, 100]),
}
FULL_CASE = dict(cfg=FULL_CFG, r=2, seed=1, x_len=[40, 33, 37, 21], mel_len=[99, 80, 91, 60])


def _model(cfg, r, seed):
    from forwardtacotron_amd.tacotron import Tacotron
    torch.manual_seed(seed)
    m = Tacotron(**cfg)
    m.r = r
    return m.cuda().train()


def _batch(np_batch):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in np_batch.items() if k in ('x', 'mel', 'speaker_emb')}


def _is_param(k, v):
    return v.is_floating_point() and 'running_' not in k and v.dim() > 0 and k != 'stop_threshold'


def _losses(m1, m2, mel, kind, l1):
    if kind == 'l1':
        return l1(m1, mel) + l1(m2, mel)
    g = torch.Generator().manual_seed(4242)                    # a fixed random linear functional of the outputs
    w1 = torch.randn(m1.shape, generator=g, dtype=torch.float64) / m1[0].numel()
    w2 = torch.randn(m2.shape, generator=g, dtype=torch.float64) / m2[0].numel()
    return (m1 * w1.to(m1.device, m1.dtype)).sum() + (m2 * w2.to(m2.device, m2.dtype)).sum()


TIE = 16 * 2.0 ** -23        # a max-pool pair closer than 16 float32 spacings is a tie no float32 forward can resolve


class _Pool:
    """Stands in for torch.maximum while the restatement runs (its only use there is the CBHG max-pool, call 0 the
    encoder's, call 1 the postnet's).  It records the NEAR-TIES of a float64 run -- pairs z[t], z[t-1] that differ, but by
    less than TIE * max(1, |z|) -- and, given some of them as `flips`, lets the other neighbour win there (the smaller
    value is raised by twice the gap, which moves the forward by less than 4e-6 * TIE)."""

    def __init__(self, flips=()):
        self.flips, self.call, self.ties, self.orig = set(flips), 0, [], torch.maximum

    def __call__(self, a, b):
        call, self.call = self.call, self.call + 1
        if a.dtype == torch.float64:
            d = (a - b).abs().detach()
            near = (d > 0) & (d < TIE * self.orig(a.abs(), b.abs()).clamp(min=1.0)) & torch.isfinite(b)
            for i in near.nonzero().tolist():
                tie = (call, *i)
                self.ties.append(tie)
                if tie in self.flips:
                    bump = torch.zeros_like(a)
                    bump[tuple(i)] = 2 * float(d[tuple(i)])
                    a, b = (a, b + bump) if float(a.detach()[tuple(i)]) > float(b.detach()[tuple(i)]) else (a + bump, b)
        return self.orig(a, b)

    def __enter__(self):
        torch.maximum = self
        return self

    def __exit__(self, *exc):
        torch.maximum = self.orig


def _restate(sd, batch, cfg, r, masks, dt, kinds, flips=()):
    """-> dict(mel_outputs, linear, attn_scores, stats, loss/<kind>, grad/<kind>/<param>, ties) of the restatement in dt;
    flips: near-ties of the max-pools (see _Pool) to resolve the other way"""
    with _Pool(flips) as pool:
        out = _restate_run(sd, batch, cfg, r, masks, dt, kinds)
    out['ties'] = pool.ties
    return out


def _restate_run(sd, batch, cfg, r, masks, dt, kinds):
    P = {k: (v.detach().cpu().to(dt).requires_grad_(True) if _is_param(k, v) else v.detach().cpu().clone())
         for k, v in sd.items()}
    for k in P:
        if 'running_' in k:
            P[k] = P[k].to(dt)
    m1, m2, attn, stats = TT.forward(P, batch, cfg, r, masks)
    out = dict(mel_outputs=m1.detach(), linear=m2.detach(), attn_scores=attn.detach(), stats=stats)
    mel = batch['mel'].to(dt)
    names = [k for k, v in P.items() if v.requires_grad]
    for i, kind in enumerate(kinds):
        loss = _losses(m1, m2, mel, kind, torch.nn.functional.l1_loss)
        gs = torch.autograd.grad(loss, [P[k] for k in names], retain_graph=i + 1 < len(kinds), allow_unused=True)
        out['loss/' + kind] = loss.detach()
        for k, g in zip(names, gs):
            out['grad/%s/%s' % (kind, k)] = g if g is not None else torch.zeros_like(P[k])
    return out


def _gpu_step(m, batch, kind):
    from forwardtacotron_amd.tacotron import l1_loss
    m.zero_grad(set_to_none=True)
    m1, m2, attn = m.forward_train(batch)
    assert not attn.requires_grad and m1.requires_grad and m2.requires_grad
    loss = _losses(m1, m2, batch['mel'].cuda(), kind, l1_loss)
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in m.named_parameters()}
    return dict(mel_outputs=m1.detach().cpu(), linear=m2.detach().cpu(), attn_scores=attn.cpu(),
                loss=loss.detach().cpu(), grads=grads)


def _masks(m, cfg, batch, r):
    B, Tx = batch['x'].shape
    S = math.ceil(batch['mel'].shape[2] / r)
    shapes = TT.site_shapes(cfg, B, Tx, S, r, cfg['lstm_dims'], cfg['postnet_dims'])
    return TT.masks_from_seeds(m.last_seeds, m._site_p(), shapes)


def _compare(what, pairs, enforce=True):
    """pairs: (name, gpu, x64, stock); prints and asserts max(4 e_stock, 1e-4 |x64|inf) for each (enforce=False: returns
    the arrays that miss instead of asserting)"""
    bad, worst = [], (0.0, None)
    for name, got, ref, stock in pairs:
        assert got is not None, (what, name, 'no gradient')
        got, ref, stock = got.double(), ref.double(), stock.double()
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert torch.isfinite(got).all(), (what, name)
        scale = float(ref.abs().max())
        err, e32 = float((got - ref).abs().max()), float((stock - ref).abs().max())
        bound = max(4 * e32, 1e-4 * scale)
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float('inf'))
        worst = max(worst, (ratio, name))
        if err > bound:
            bad.append((name, scale, e32, err))
            print('%s %-60s |x64|inf %.2e  stock %.2e  gpu %.2e  gpu / bound %.2f' % (what, name, scale, e32, err, ratio))
    print('%s: %d arrays, worst gpu / bound %.3f (%s)' % (what, len(pairs), worst[0], worst[1]))
    assert not (bad and enforce), (what, bad)
    return bad


def _check_against_restatement(m, c, batch, kinds):
    cfg, r = c['cfg'], c['r']
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    runs = {}
    for kind in kinds:
        m.load_state_dict(sd0)
        seeds = getattr(m, '_test_seeds', None)
        m._forced_seeds = seeds
        runs[kind] = _gpu_step(m, batch, kind)
        m._test_seeds = dict(m.last_seeds)                       # the second loss runs on the first one's masks
    masks = _masks(m, cfg, batch, r)
    r64 = _restate(sd0, batch, cfg, r, masks, torch.float64, kinds)
    r32 = _restate(sd0, batch, cfg, r, masks, torch.float32, kinds)
    # A max-pool pair that float64 separates by less than TIE is a tie for every float32 forward: which neighbour gets
    # the gradient is decided by rounding, and the float64 gradient with the OTHER neighbour is as right as r64's.  The
    # device must match ONE resolution of these ties in ALL arrays (r64's own is tried first); there are few such pairs
    # (none at the tiny configs, one at the full width), and a tie wider than TIE gets no such allowance.
    ties = sorted(set(r64['ties']))
    print('%s: max-pool near-ties below %.1e in float64: %s' % (c.get('name', ''), TIE, ties))
    assert len(ties) <= 3, ties
    refs = [((), r64)]
    for n in range(1, 2 ** len(ties)):
        flips = tuple(t for i, t in enumerate(ties) if n >> i & 1)
        refs.append((flips, _restate(sd0, batch, cfg, r, masks, torch.float64, kinds, flips)))
    sd1 = m.state_dict()
    for kind in kinds:
        g = runs[kind]
        for i, (flips, ref) in enumerate(refs):
            pairs = [(k, g[k], ref[k], r32[k]) for k in ('mel_outputs', 'linear', 'attn_scores')]
            pairs.append(('loss', g['loss'].reshape(1), ref['loss/' + kind].reshape(1), r32['loss/' + kind].reshape(1)))
            pairs += [('grad ' + k, g['grads'][k], ref['grad/%s/%s' % (kind, k)], r32['grad/%s/%s' % (kind, k)])
                      for k in g['grads']]
            what = '%s %s%s' % (c.get('name', ''), kind, ' [ties resolved the other way: %s]' % (flips,) if flips else '')
            if not _compare(what, pairs, enforce=i + 1 == len(refs)):
                break
    _compare('%s BN statistics' % c.get('name', ''),
             [(k, sd1[k].cpu(), r64['stats'][k], r32['stats'][k]) for k in r64['stats']])
    for k, v in sd1.items():
        if k.endswith('num_batches_tracked') or k == 'step':
            assert int(v.reshape(-1)[0]) == int(sd0[k].reshape(-1)[0]) + 1, k
    return runs, r64


@pytest.mark.parametrize('name', list(TINY_CASES))
def test_tiny_cases_match_float64_restatement(name):
    c = dict(TINY_CASES[name], name=name)
    m = _model(c['cfg'], c['r'], c['seed'])
    batch = _batch(make_batch(c['x_len'], c['mel_len'], c['r'], c['cfg']['speaker_emb_dim'], 40 + len(name)))
    runs, _ = _check_against_restatement(m, c, batch, ['l1'])
    assert all(v is not None for v in m.last_seeds.values()) and len(m.last_seeds) == 10
    gm = runs['l1']['grads']['decoder.mel_proj.weight'].view(80, 20, -1)
    assert not bool(gm[:, c['r']:].any()) and bool(gm[:, :c['r']].any())      # exact zeros in the dropped rows


def test_full_width_case_matches_float64_restatement_under_both_losses():
    """the reference's singlespeaker config, B = 4, r = 2, all ten sites on, the L1 loss and a linear functional.

    With these masks the float64 restatement has ONE max-pool near-tie (postnet bank, k = 4, filter 27, item 1, frame 45:
    z[t] and z[t-1] 5.55e-7 apart at values of order 1, the next closest pair 2.7e-6).  The device's float32 forward,
    1.4e-6 from float64, takes the other neighbour: against r64's own resolution 112 of 171 gradients miss (median
    2.15e-4 of own scale, postnet.conv1d_bank.3.conv.weight 4.88e-2, all of it in filter 27) -- and the float64
    restatement with that one pair resolved the other way differs from r64 by exactly these figures (median 2.15e-4, 112
    arrays over 1e-4, 4.88e-2 on the same weight).  _check_against_restatement therefore admits either resolution of
    a pair closer than TIE, one resolution for all arrays."""
    c = dict(FULL_CASE, name='full')
    m = _model(c['cfg'], c['r'], c['seed'])
    batch = _batch(make_batch(c['x_len'], c['mel_len'], c['r'], 0, 107))
    _check_against_restatement(m, c, batch, ['l1', 'linear'])


@pytest.mark.parametrize('name', ['b', 'c'])
def test_fixture_cases_match_the_reference_training_step(name):
    z = np.load(GOLDEN)
    p = name + '/'
    cfg, r, seed = json.loads(str(z[p + 'cfg'])), int(z[p + 'r']), int(z[p + 'seed'])
    m = _model(cfg, 1, seed)
    assert sd_sha256({k: v.cpu() for k, v in m.state_dict().items()}) == str(z[p + 'sd_sha256'])   # seed-identical init
    m.r = r                                                          # (the recorded hash is of the r = 1 state_dict)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    sites = [s.decode() for s in z[p + 'sites']]
    seeds = {s: int(v) for s, v in zip(sites, z[p + 'site_seeds'])}
    assert m._site_p() == {s: float(v) for s, v in zip(sites, z[p + 'site_p'])}
    m._forced_seeds = seeds
    batch = _batch({k: z[p + k] for k in ('x', 'mel', 'speaker_emb')})
    g = _gpu_step(m, batch, 'l1')
    assert m.last_seeds == seeds
    r64 = _restate(sd0, batch, cfg, r, _masks(m, cfg, batch, r), torch.float64, ['l1'])
    rec = lambda k: torch.from_numpy(z[p + k])
    pairs = [(k, g[k], r64[k], rec(k)) for k in ('mel_outputs', 'linear', 'attn_scores')]
    pairs.append(('loss', g['loss'].reshape(1), r64['loss/l1'].reshape(1), rec('loss').reshape(1)))
    for k, gv in g['grads'].items():
        pairs.append(('grad ' + k, torch.from_numpy(sample(gv)), torch.from_numpy(sample(r64['grad/l1/' + k])),
                      rec('grad/' + k)))
    sd1 = m.state_dict()
    for k in r64['stats']:
        pairs.append((k, sd1[k].cpu(), r64['stats'][k], rec('bn/' + k)))
    _compare('fixture ' + name, pairs)
    for k, v in sd1.items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(z[p + 'bn/' + k]) == 1, k
    assert int(sd1['step']) == int(z[p + 'step']) == 1


def _tiny():
    c = TINY_CASES['tiny-r3']
    batch = _batch(make_batch(c['x_len'], c['mel_len'], c['r'], 0, 9))
    return c, _model(c['cfg'], c['r'], c['seed']), batch


def test_manual_seed_reproduces_outputs_and_gradients_bit_for_bit():
    c, m, batch = _tiny()
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    runs = []
    for seed in (7, 7, 8):
        m.load_state_dict(sd0)
        torch.manual_seed(seed)
        runs.append((_gpu_step(m, batch, 'l1'), dict(m.last_seeds)))
    (a, sa), (b, sb), (d, sd) = runs
    assert sa == sb and sa != sd
    for k in ('mel_outputs', 'linear', 'attn_scores', 'loss'):
        assert torch.equal(a[k], b[k]), k
    for k in a['grads']:
        assert torch.equal(a['grads'][k], b['grads'][k]), k
    assert not torch.equal(a['mel_outputs'], d['mel_outputs'])


def test_all_sites_off_runs_and_matches():
    """zoneout 0 and every dropout p = 0: no seed is drawn (the reference cannot run this, the restatement can)"""
    c, m, batch = _tiny()
    m.zoneout = 0.0
    m.encoder.pre_net.p = m.decoder.prenet.p = 0.0
    m.encoder.cbhg.dropout = m.postnet.dropout = 0.0
    state = torch.random.get_rng_state()
    _check_against_restatement(m, dict(c, name='sites off'), batch, ['l1'])
    assert torch.equal(state, torch.random.get_rng_state())
    assert m.last_seeds == dict.fromkeys(m.SITES)


def test_adam_step_with_the_reference_loop():
    """optimizer.zero_grad(); loss.backward(); clip_grad_norm_; optimizer.step() with torch.optim.Adam on the device
    tensors: every parameter changes, and where the gradient is at least 1e-2 of its tensor's scale -- there the
    gradient bound 1e-4 |g|inf is a relative error of 1e-2, i.e. lr * 1e-2 = 1e-5 of Adam's first step of lr * g / |g| --
    the stepped parameters match the float64 restatement's step to 1e-5"""
    from forwardtacotron_amd.tacotron import l1_loss
    lr, clip = 1e-3, 1.0
    c, m, batch = _tiny()
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    opt.zero_grad()
    m1, m2, _ = m.forward_train(batch)
    loss = l1_loss(m1, batch['mel'].cuda()) + l1_loss(m2, batch['mel'].cuda())
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), clip)
    opt.step()
    torch.cuda.synchronize()
    r64 = _restate(sd0, batch, c['cfg'], c['r'], _masks(m, c['cfg'], batch, c['r']), torch.float64, ['l1'])
    names = [k for k, _ in m.named_parameters()]
    P = [sd0[k].double().requires_grad_(True) for k in names]
    for p_, k in zip(P, names):
        p_.grad = r64['grad/l1/' + k].clone()
    opt64 = torch.optim.Adam(P, lr=lr)
    torch.nn.utils.clip_grad_norm_(P, clip)
    opt64.step()
    worst = (0.0, None)
    for (k, p_gpu), p64 in zip(m.named_parameters(), P):
        g = r64['grad/l1/' + k]
        if k != 'decoder.mel_proj.weight':
            assert not torch.equal(p_gpu.detach().cpu(), sd0[k]), k
        live = g.abs() >= 1e-2 * g.abs().max()
        assert bool(live.any()), k
        d = float((p_gpu.detach().cpu().double() - p64.detach()).abs()[live].max())
        worst = max(worst, (d, k))
        assert d <= 1e-5, (k, d)
    assert bool((m.decoder.mel_proj.weight.detach().cpu() != sd0['decoder.mel_proj.weight']).any())
    print('post-Adam max |gpu - float64| over live elements: %.2e (%s)' % worst)


def test_forward_and_align_still_refuse_training_and_grad():
    from forwardtacotron_amd.tacotron import FtError
    c, m, batch = _tiny()
    with pytest.raises(FtError, match='training the teacher'):
        m(batch)
    with pytest.raises(FtError, match='training the teacher'):
        m.align(batch)
    m.eval()
    with pytest.raises(FtError, match='no_grad'):
        m(batch)
    with pytest.raises(FtError, match='no_grad'):
        m.align(batch)
