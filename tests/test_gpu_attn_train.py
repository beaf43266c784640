"""GPU: the fused training attention of csrc/ft_attn.hip alone -- ft_attn_fwd_kernel, ft_attn_delta_kernel,
ft_attn_bwd_dq_kernel and ft_attn_bwd_dkv_kernel through hip.attn_fwd / hip.attn_bwd, the backward fed with the kernel's
own att and lse2 as mha_bwd feeds it.

Yardsticks (tests/attn_cpu.py, proven in tests/test_attn_cpu.py): reference() is exact float64 attention on the
bf16-rounded q / k / v with the host's dropout mask; emulate() is the same with the kernels' rounding points.  Bar, per
(item, head) slab and per output (att, lse2, dq, dk, dv) over all T query rows -- padded queries attend to the valid
keys, as in torch:

    |kernel - reference| <= 4 E + 16 * 2^-24 * max(1, max|ref|),     E = max |emulate - reference| over the slab.

The 4 is the room the project gives a kernel over a yardstick for summation order and v_exp_f32
(test_fp32_error_against_the_unfused_route), the floor is the one of tests/test_gpu_taco_kernels.py.  Every comparison
prints error / bar and error / E per slab, and the distance to the emulation itself (not asserted).  T = 200 gives two 128-row workgroups and four 64-key blocks in all three
kernels; the cases and their inputs are attn_cpu.CASES."""
import pytest
import torch

import attn_cpu as A

pytestmark = pytest.mark.gpu

_cache = {}


def _dev(t):
    return None if t is None else t.cuda()


def _run(qkv, datt, key_pad, nh, scale, p, seed):
    """-> att, lse2, dqkv on the host; the backward gets the forward's own att and lse2"""
    from forwardtacotron_amd import hip
    qkv, datt, key_pad = _dev(qkv), _dev(datt), _dev(key_pad)
    att, lse2 = hip.attn_fwd(qkv, key_pad, nh, scale, p, seed)
    dqkv = hip.attn_bwd(qkv, att, datt, key_pad, lse2, nh, scale, p, seed)
    return att.cpu(), lse2.cpu(), dqkv.cpu()


def _run_case(c):
    return _run(c['qkv'], c['datt'], c['key_pad'], c['nh'], c['scale'], c['p'], c['seed'])


def _outputs(att, lse2, dqkv):
    dq, dk, dv = dqkv.split(dqkv.shape[-1] // 3, dim=-1)
    return dict(att=att, lse2=lse2, dq=dq, dk=dk, dv=dv)


@pytest.fixture(scope='module')
def case():
    """case(name) -> (inputs, kernel outputs, reference, {output: (bar, E, emulation)}) -- each computed once per module"""
    def get(name):
        if name not in _cache:
            c = A.make_case(name)
            ref = A.reference(*A.args(c))
            emu = A.emulate(*A.args(c))
            bars = {o: A.slab_bar(o, emu[o], ref[o], c['nh']) + (emu[o],) for o in A.OUTPUTS}
            _cache[name] = (c, _outputs(*_run_case(c)), ref, bars)
        return _cache[name]
    return get


def _hold(name, c, got, ref, bars):
    """every slab of every output inside its bar; prints error / bar and error / E"""
    worst = {}
    for o in A.OUTPUTS:
        bar, E, emu = bars[o]
        assert got[o].shape == ref[o].shape and not bool(torch.isnan(got[o]).any()), o
        err = A.slab_err(o, got[o], ref[o], c['nh'])
        for b in range(err.shape[0]):
            for h in range(err.shape[1]):
                e, t, ee = float(err[b, h]), float(bar[b, h]), float(E[b, h])
                print(f'{name} {o:4s} item {b} head {h}: {e:.3e} off float64, bar {t:.3e} ({e / t:.2f}), '
                      f'E {ee:.3e} ({e / ee if ee > 0 else float("nan"):.2f})')
        worst[o] = (float((err / bar).max()), float((err / E)[E > 0].max()) if bool((E > 0).any()) else float('nan'),
                    float(A.slab_err(o, got[o], emu, c['nh']).max()))
    print(f'{name} worst error / bar: ' + ', '.join(f'{o} {worst[o][0]:.3f}' for o in A.OUTPUTS))
    print(f'{name} worst error / E: ' + ', '.join(f'{o} {worst[o][1]:.3f}' for o in A.OUTPUTS))
    print(f'{name} off the emulation (not asserted): ' + ', '.join(f'{o} {worst[o][2]:.1e}' for o in A.OUTPUTS))
    for o in A.OUTPUTS:
        bar = bars[o][0]
        err = A.slab_err(o, got[o], ref[o], c['nh'])
        assert bool((err <= bar).all()), (name, o, (err / bar).tolist())


def _padded_keys_get_no_gradient(c, got):
    if c['key_pad'] is not None:
        pad = c['key_pad'].bool()
        for o in ('dk', 'dv'):
            assert bool((got[o][pad] == 0).all()), o


EDGES = [n for n in A.CASES if n.startswith('edges')]
HEADS = [n for n in A.CASES if n.startswith('heads')]
SMALL = [n for n in A.CASES if n.startswith('small')]
BYTES = [n for n in A.CASES if n.startswith('bytes')]


@pytest.mark.parametrize('name', EDGES)
def test_lengths_on_the_block_and_workgroup_edges(case, name):
    """suffix lengths 1 / 63 / 64 / 65 / 128 / 129 / 200 in one batch: each item is held by its own slabs"""
    c, got, ref, bars = case(name)
    _hold(name, c, got, ref, bars)
    _padded_keys_get_no_gradient(c, got)


@pytest.mark.parametrize('name', EDGES)
def test_single_key_leaves_rounding_only(case, name):
    """L = 1: the float64 dq and dk are exactly 0.  The kernels leave O(2^-9 |dO| |v|) there -- delta is formed from the
    fp32 datt, dP from the bf16-rounded one -- which emulate() reproduces, so the residue sits inside the bar."""
    c, got, ref, bars = case(name)
    for o in ('dq', 'dk'):
        assert float(ref[o][0].abs().max()) == 0.0
        res = float(got[o][0].abs().max())
        bar, E, _ = bars[o]
        print(f'{name} {o} of the single-key item: kernel {res:.3e}, emulation {float(E[0].max()):.3e}, '
              f'bar {float(bar[0].min()):.3e}')
        assert bool((A.slab_err(o, got[o], ref[o], c['nh'])[0] <= bar[0]).all())


@pytest.mark.parametrize('name', HEADS)
def test_head_addressing(case, name):
    """nh 1 and 3: h * HD, dmodel and the per-head delta / lse2 / mask index"""
    c, got, ref, bars = case(name)
    _hold(name, c, got, ref, bars)
    _padded_keys_get_no_gradient(c, got)


@pytest.mark.parametrize('name', SMALL)
def test_small_and_odd_lengths(case, name):
    c, got, ref, bars = case(name)
    _hold(name, c, got, ref, bars)
    _padded_keys_get_no_gradient(c, got)
    if c['T'] == 1 and c['p'] > 0:                      # one probability per row: dropped entirely, or doubled
        d = c['nh'] * c['hd']
        v = c['qkv'][:, :, 2 * d:].bfloat16().float()
        keep = torch.as_tensor(c['keep']).float().reshape(c['B'], 1, c['nh'], 1).expand(-1, -1, -1, c['hd'])
        assert set(keep.unique().tolist()) <= {0.0, 2.0}
        assert torch.equal(got['att'], keep.reshape(c['B'], 1, d) * v)


@pytest.mark.parametrize('name', BYTES)
def test_byte_masks_that_are_no_suffix(case, name):
    """keys 0..63 masked (every row starts the online softmax at m = -inf), keys 64..127 masked, every second key
    masked, only key 199 valid"""
    c, got, ref, bars = case(name)
    _hold(name, c, got, ref, bars)
    _padded_keys_get_no_gradient(c, got)


# ---------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------
GUARD = 1024                                            # floats: 4096 bytes in front and behind


def _carve(n):
    big = torch.full((GUARD + n + GUARD,), float('nan'), device='cuda')
    return big, big[GUARD:GUARD + n]


def _guards_intact(big, n, what):
    bits = big.view(torch.int32)
    nan = torch.full((1,), float('nan'), device='cuda').view(torch.int32)
    assert bool((bits[:GUARD] == nan).all()) and bool((bits[GUARD + n:] == nan).all()), what


@pytest.mark.parametrize('name', ['edges-hd64-p0.1', 'heads-nh3-hd128'])
def test_outputs_stay_inside_their_buffers(case, name):
    """att, lse2 and dqkv carved out of NaN allocations with 4096-byte guard bands, a workspace of 0xFF bytes: the
    results are the wrapper's bit for bit, no NaN is left inside, no guard word changes"""
    from forwardtacotron_amd import _lib, hip
    c, got, _, _ = case(name)
    B, T, nh, hd = c['B'], c['T'], c['nh'], c['hd']
    d = nh * hd
    qkv, datt, kp = c['qkv'].cuda(), c['datt'].cuda(), _dev(c['key_pad'])
    seed = int(c['seed']) & 0xFFFFFFFFFFFFFFFF
    att_big, att = _carve(B * T * d)
    lse_big, lse2 = _carve(B * nh * T)
    dq_big, dqkv = _carve(B * T * 3 * d)
    nws = int(_lib.query('ft_attn_workspace', B, T, nh))
    ws_big = torch.full((4096 + nws + 4096,), 255, dtype=torch.uint8, device='cuda')
    ws = ws_big[4096:4096 + nws]
    _lib.call('ft_attn_fwd', qkv.data_ptr(), hip._p(kp), att.data_ptr(), lse2.data_ptr(), B, T, nh, hd, float(c['scale']),
              float(c['p']), seed, hip._stream())
    _lib.call('ft_attn_bwd', qkv.data_ptr(), att.data_ptr(), datt.data_ptr(), hip._p(kp), lse2.data_ptr(), dqkv.data_ptr(),
              B, T, nh, hd, float(c['scale']), float(c['p']), seed, ws.data_ptr(), nws, hip._stream())
    torch.cuda.synchronize()
    for big, view, what in ((att_big, att, 'att'), (lse_big, lse2, 'lse2'), (dq_big, dqkv, 'dqkv')):
        _guards_intact(big, view.numel(), what)
        assert not bool(torch.isnan(view).any()), what
    assert bool((ws_big[:4096] == 255).all()) and bool((ws_big[4096 + nws:] == 255).all())
    assert torch.equal(att.cpu().reshape(B, T, d), got['att'])
    assert torch.equal(lse2.cpu().reshape(B, nh, T), got['lse2'])
    assert torch.equal(dqkv.cpu().reshape(B, T, 3 * d), torch.cat([got['dq'], got['dk'], got['dv']], dim=-1))


# ---------------------------------------------------------------------------------------------------
# isolation and reproducibility
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['edges-hd64-p0.0', 'edges-hd128-p0.0'])
def test_an_item_alone_equals_the_item_in_the_batch(case, name):
    c, got, _, _ = case(name)
    for b in range(c['B']):
        att, lse2, dqkv = _run(c['qkv'][b:b + 1], c['datt'][b:b + 1], c['key_pad'][b:b + 1], c['nh'], c['scale'], 0.0, 0)
        alone = _outputs(att, lse2, dqkv)
        for o in A.OUTPUTS:
            assert torch.equal(alone[o][0], got[o][b]), (b, o)


@pytest.mark.parametrize('name', ['edges-hd64-p0.1', 'edges-hd128-p0.1'])
def test_neighbours_are_irrelevant_under_dropout(case, name):
    """the item keeps its batch slot (the mask index holds the item); every neighbour and every other length changes,
    one neighbour has all its keys padded (NaN there, as in torch: not asserted)"""
    c, got, _, _ = case(name)
    b = 3
    g = torch.Generator().manual_seed(77)
    qkv = torch.randn(c['qkv'].shape, generator=g)
    datt = torch.randn(c['datt'].shape, generator=g)
    qkv[b], datt[b] = c['qkv'][b], c['datt'][b]
    lens = [200, 0, 130, A.EDGE_LENS[b], 1, 77, 64]
    att, lse2, dqkv = _run(qkv, datt, A._suffix(lens, c['T']), c['nh'], c['scale'], c['p'], c['seed'])
    other = _outputs(att, lse2, dqkv)
    for o in A.OUTPUTS:
        assert torch.equal(other[o][b], got[o][b]), o
        for i in range(c['B']):
            if lens[i] > 0:
                assert not bool(torch.isnan(other[o][i]).any()), (o, i)


@pytest.mark.parametrize('name', ['edges-hd128-p0.1', 'heads-nh3-hd64'])
def test_forward_and_backward_run_twice_are_bit_equal(case, name):
    from forwardtacotron_amd import hip
    c, got, _, _ = case(name)
    qkv, datt, kp = c['qkv'].cuda(), c['datt'].cuda(), _dev(c['key_pad'])
    fwd = [hip.attn_fwd(qkv, kp, c['nh'], c['scale'], c['p'], c['seed']) for _ in range(2)]
    assert torch.equal(fwd[0][0], fwd[1][0]) and torch.equal(fwd[0][1], fwd[1][1])
    att, lse2 = fwd[0]
    bwd = [hip.attn_bwd(qkv, att, datt, kp, lse2, c['nh'], c['scale'], c['p'], c['seed']) for _ in range(2)]
    assert torch.equal(bwd[0], bwd[1])
    again = _outputs(att.cpu(), lse2.cpu(), bwd[0].cpu())
    for o in A.OUTPUTS:
        assert torch.equal(again[o], got[o]), o
