"""tests/rnn_cpu.py (the float64 restatement the GPU recurrence matrix compares with) against torch.nn.GRU / torch.nn.LSTM
and autograd in float64 -- both directions and one, padded and packed (pack_padded_sequence) -- on the (B, T) shapes
tests/test_gpu_rnn_forms.py runs, at widths cut for the CPU; and the margin of the GPU bounds: the same recurrences in
plain fp32 stay within a quarter of them on every shape of the matrix.  No GPU."""
import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import rnn_cpu as R


def close(a, b, what=''):
    a, b = R.f64(a), R.f64(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.all(np.isfinite(a)), what
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9, err_msg=what)


def torch_module(G, H, nd, whh, bhh):
    """nn.GRU / nn.LSTM in float64 whose input IS the x projection: W_ih of direction d selects the direction's G*H
    columns of the xp row, b_ih = 0"""
    m = (torch.nn.GRU if G == 3 else torch.nn.LSTM)(nd * G * H, H, bidirectional=nd == 2).double()
    with torch.no_grad():
        for d, sfx in enumerate(['', '_reverse'][:nd]):
            wih = torch.zeros(G * H, nd * G * H, dtype=torch.float64)
            wih[:, d * G * H:(d + 1) * G * H] = torch.eye(G * H, dtype=torch.float64)
            getattr(m, 'weight_ih_l0' + sfx).copy_(wih)
            getattr(m, 'bias_ih_l0' + sfx).zero_()
            getattr(m, 'weight_hh_l0' + sfx).copy_(torch.from_numpy(R.f64(whh[d])))
            getattr(m, 'bias_hh_l0' + sfx).copy_(torch.from_numpy(R.f64(bhh[d])))
    return m


def torch_run(G, inp):
    """-> module (with .grad), out [T,B,nd*H], h_n, c_n, d loss / d xp for loss = sum(out * dout)"""
    T, B, H, nd, lens = inp['T'], inp['B'], inp['H'], inp['nd'], inp['lens']
    m = torch_module(G, H, nd, inp['whh'], inp['bhh'])
    x = torch.from_numpy(R.f64(inp['xp'])).requires_grad_(True)
    if lens is None:
        out, hc = m(x)
    else:
        po, hc = m(pack_padded_sequence(x, torch.from_numpy(lens), enforce_sorted=False))
        out, _ = pad_packed_sequence(po, total_length=T)
    (out * torch.from_numpy(R.f64(inp['dout']))).sum().backward()
    h_n, c_n = (hc, None) if G == 3 else hc
    return m, out.detach(), h_n.detach(), None if c_n is None else c_n.detach(), x.grad


def last_state(state, lens, B, T, H, nd):
    """[nd, B, H]: the state after an item's last step (t = L - 1 forward, t = 0 reverse)"""
    L = R.clamp_lens(lens, B, T)
    rows = np.arange(B)
    return np.stack([state[L - 1 if d == 0 else np.zeros_like(L), rows, d * H:(d + 1) * H] for d in range(nd)])


CPU_WIDTHS = (16, 48)        # the matrix's widths cut for the CPU: one power of two, one that is not
CPU_CASES = [(G, B, T, H, nd, packed) for G in (3, 4) for (B, T, packed) in R.BT for H in CPU_WIDTHS for nd in (2, 1)
             if nd == 2 or (H == 16 and not packed)]


@pytest.mark.parametrize('G,B,T,H,nd,packed', CPU_CASES)
def test_forward_and_backward_equal_torch(G, B, T, H, nd, packed):
    inp = R.rnn_inputs(G, B, T, H, nd, seed=1, packed=packed)
    m, out_t, h_n, c_n, dx_t = torch_run(G, inp)
    out, cst, gates = R.rnn_fwd(G, inp['xp'], inp['whh'], inp['bhh'], H, inp['lens'])
    close(out, out_t, 'out')
    close(last_state(out, inp['lens'], B, T, H, nd), h_n, 'h_n')
    if G == 4:
        close(last_state(cst, inp['lens'], B, T, H, nd), c_n, 'c_n')
    act = R.active_mask(inp['lens'], B, T)
    assert np.all(out[~act] == 0) and (cst is None or np.all(cst[~act] == 0))
    # the saved activations reproduce the states they belong to
    for d in range(nd):
        sg = gates[:, :, d]
        if G == 4:
            close(out[..., d * H:(d + 1) * H][act], (sg[..., 3 * H:] * np.tanh(cst[..., d * H:(d + 1) * H]))[act], 'o tanh c')
        assert np.all((sg[..., :2 * H][act] > 0) & (sg[..., :2 * H][act] < 1))

    dxp, dhp = R.rnn_bwd(G, inp['dout'], out, cst, gates, inp['whh'], H, inp['lens'])
    close(dxp, dx_t, 'dxp / dg: d loss / d xp')
    assert np.all(dxp[~act] == 0) and np.all(dhp[~act] == 0)
    K = G * H
    L = R.clamp_lens(inp['lens'], B, T)
    for d, sfx in enumerate(['', '_reverse'][:nd]):
        dh = dhp[..., d * K:(d + 1) * K]
        if G == 4:
            assert np.array_equal(dh, dxp[..., d * K:(d + 1) * K])
        else:   # the n gate's hidden pre-activation sits behind the r gate
            r = gates[:, :, d, :H]
            close(dh[..., 2 * H:], dxp[..., d * K + 2 * H:(d + 1) * K] * r, 'dhp n = dn * r')
            assert np.array_equal(dh[..., :2 * H], dxp[..., d * K:d * K + 2 * H])
        # dhp position by position, through the two gradients that are sums over it: b_hh and W_hh (against h_prev)
        close(dh.sum((0, 1)), getattr(m, 'bias_hh_l0' + sfx).grad, 'sum dhp = d b_hh')
        hprev = np.zeros((T, B, H))
        hs = out[..., d * H:(d + 1) * H]
        if d == 0:
            hprev[1:] = hs[:-1]
        else:
            hprev[:-1] = hs[1:]
            hprev[np.clip(L - 1, 0, None), np.arange(B)] = 0        # the reverse direction starts at t = L - 1
        close(np.einsum('tbk,tbh->kh', dh, hprev), getattr(m, 'weight_hh_l0' + sfx).grad, 'dhp^T h_prev = d W_hh')


@pytest.mark.parametrize('G', [3, 4])
def test_entry_points_by_name(G):
    inp = R.rnn_inputs(G, 5, 9, 16, 2, seed=2, packed=True)
    w, b = inp['whh'], inp['bhh']
    ref = R.reference(inp)
    if G == 3:
        assert np.array_equal(R.gru_fwd_lens(inp['xp'], w[0], w[1], b[0], b[1], inp['lens'], 16), ref['out'])
        out, gates = R.gru_fwd(inp['xp'], w[0], w[1], b[0], b[1], 16)
        full = R.rnn_fwd(3, inp['xp'], w, b, 16)
        assert np.array_equal(out, full[0]) and np.array_equal(gates, full[2])
        dxp, dhp = R.gru_bwd(inp['dout'], out, gates, w[0], w[1], 16)
        want = R.rnn_bwd(3, inp['dout'], out, None, gates, w, 16)
        assert np.array_equal(dxp, want[0]) and np.array_equal(dhp, want[1])
    else:
        raw, cst, gates = R.lstm_fwd(inp['xp'], w[0], w[1], b[0], b[1], inp['lens'], 16)
        assert np.array_equal(raw, ref['out']) and np.array_equal(cst, ref['cst'])
        assert np.array_equal(R.lstm_bwd(inp['dout'], raw, cst, gates, w[0], w[1], inp['lens'], 16), ref['dxp'])
        one = R.rnn_inputs(4, 5, 9, 16, 1, seed=2)
        o, c = R.lstm_fwd_uni(one['xp'], one['whh'][0], one['bhh'][0], 16)
        _, out_t, _, _, _ = torch_run(4, one)
        close(o, out_t, 'lstm_fwd_uni')
        assert o.shape == c.shape == (9, 5, 16)


@pytest.mark.parametrize('G', [3, 4])
def test_zero_length_item_is_never_active(G):
    """clamp_len maps a length of 0 (or below) to 'never active': the item's rows are exactly zero everywhere and the
    other items are what they are without it (torch refuses such a batch, so the comparison is with the batch less the item)"""
    B, T, H = 5, 9, 16
    inp = R.rnn_inputs(G, B, T, H, 2, seed=3, packed=True, zero_len=True)
    z = int(np.flatnonzero(inp['lens'] == 0)[0])
    ref = R.reference(inp)
    for k in ('out', 'cst', 'gates', 'dxp', 'dhp'):
        if ref[k] is not None:
            assert np.all(ref[k][:, z] == 0), k
    keep = [b for b in range(B) if b != z]
    out, cst, gates = R.rnn_fwd(G, inp['xp'][:, keep], inp['whh'], inp['bhh'], H, inp['lens'][keep])
    dxp, dhp = R.rnn_bwd(G, inp['dout'][:, keep], out, cst, gates, inp['whh'], H, inp['lens'][keep])
    close(ref['out'][:, keep], out); close(ref['dxp'][:, keep], dxp); close(ref['dhp'][:, keep], dhp)
    neg = inp['lens'].copy()
    neg[z] = -3
    assert np.array_equal(R.rnn_fwd(G, inp['xp'], inp['whh'], inp['bhh'], H, neg)[0], ref['out'])


def test_inputs_follow_the_width():
    assert R.whh_scale(128) == 0.3 and R.whh_scale(256) == 0.1 and abs(R.whh_scale(512) - 1.6 / 512 ** 0.5) < 1e-15
    for packed in (False, True):
        inp = R.rnn_inputs(4, 21, 12, 16, 2, seed=0, packed=packed)
        assert inp['xp'].dtype == np.float32 and inp['dout'].dtype == np.float32
        assert np.unique(inp['dout']).size > inp['dout'].size // 2, 'dout must be random, never constant'
        if packed:
            assert inp['lens'][0] == 12 and inp['lens'][-1] == 1 and inp['lens'].min() >= 1 and inp['lens'].max() <= 12
    assert R.rnn_inputs(4, 21, 12, 16, 2, seed=0, packed=True, zero_len=True)['lens'].min() == 0


def margin_errors(G, B, T, H, nd, packed):
    inp = R.rnn_inputs(G, B, T, H, nd, 0, packed, packed)        # the GPU matrix's own inputs: a packed case holds an
    ref = R.reference64(G, B, T, H, nd, 0, packed, packed)       # item of length 0
    f32 = R.reference(inp, np.float32)
    err = {}
    for k, v in ref.items():
        if v is None:
            continue
        assert f32[k].dtype == np.float32
        bound = R.FWD_TOL if k in ('out', 'cst', 'gates') else R.GRAD_TOL * max(1.0, float(np.abs(v).max()))
        err[k] = (float(np.abs(f32[k].astype(np.float64) - v).max()), bound)
    return err


@pytest.mark.parametrize('G,H', R.WIDTHS)
def test_plain_fp32_uses_at_most_a_quarter_of_the_gpu_bounds(G, H):
    """The GPU matrix holds every kernel form to 2e-5 (forward) and 1e-4 * max(1, max |ref|) (gradients) against this
    restatement in float64.  The same recurrences evaluated in plain fp32 on the matrix's own inputs must stay within a
    quarter of those bounds, on every (B, T) the width runs with: the bounds then leave an honest fp32 kernel room, and a
    later change of shapes or weight scales cannot quietly turn them meaningless (a chaotic recurrence would)."""
    for (B, T, packed) in R.BT:
        for k, (e, bound) in margin_errors(G, B, T, H, 2, packed).items():
            assert e <= bound / 4, (G, H, B, T, packed, k, e, bound)
    if (G, H) == (4, 512):
        for (Hu, B, T) in R.UNI:
            for k, (e, bound) in margin_errors(4, B, T, Hu, 1, False).items():
                assert e <= bound / 4, ('uni', Hu, B, T, k, e, bound)
