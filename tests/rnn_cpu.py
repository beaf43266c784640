"""Plain numpy restatement of the recurrence primitives (hip.gru_fwd / gru_fwd_lens / gru_bwd / lstm_fwd / lstm_bwd and
ft_lstm_fwd_uni), in float64 by default, on the buffers and layouts the kernels use (csrc/ft_rnn.hip, ops.py):

    xp    [T, B, ND*G*H]   x W_ih^T + b_ih, a row laid out [direction][gate][unit]; gates r, z, n (GRU) | i, f, g, o (LSTM)
    whh   ND x [G*H, H],  bhh  ND x [G*H]          (per direction)
    out / raw, cst  [T, B, ND*H]   hidden / LSTM cell states, zero at t >= lens[b]
    gates [T, B, ND, 4H]   saved activations: r, z, n, W_hn h + b_hn (GRU) | i, f, g, o (LSTM); written at active positions
    dxp, dhp [T, B, ND*G*H]   gradients wrt the input / hidden pre-activations (GRU n gate: dhp = dn * r); LSTM: one dg
    time: direction 0 runs t = 0 .. L-1, direction 1 runs t = L-1 .. 0 with L = lens[b] (T without lens); a length is
    clamped to [0, T] (clamp_len), so a zero-length item is never active.

tests/test_rnn_cpu.py checks this file against torch.nn.GRU / torch.nn.LSTM and autograd in float64; the GPU matrix
(tests/test_gpu_rnn_forms.py) compares every kernel form with it.  dtype=np.float32 evaluates the same recurrences in
plain fp32: the yardstick for how much of the GPU tests' bounds an honest fp32 implementation uses."""
import functools

import numpy as np

FWD_TOL = 2e-5              # forward outputs against float64 (the bound tests/test_gpu_rnn.py holds the kernels to)
GRAD_TOL = 1e-4             # gradients: GRAD_TOL * max(1, max |reference|)


def f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, 'detach') else a, dtype=np.float64)


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def whh_scale(H):
    """standard deviation of the recurrent weights: see tests/test_gpu_rnn.py::_params (0.3 makes a recurrence wider
    than 128 chaotic, so the scale follows the width there)"""
    return 0.3 if H <= 128 else 1.6 / H ** 0.5


def packed_lens(B, T, rng, zero_len=False):
    """random lengths in [1, T] with one item at T and one at 1 (B >= 2), optionally one of length 0"""
    lens = rng.integers(1, T + 1, size=B).astype(np.int64)
    lens[0] = T
    if B > 1:
        lens[B - 1] = 1
    if zero_len and B > 2:
        lens[B // 2] = 0
    return lens


@functools.lru_cache(maxsize=None)
def rnn_inputs(G, B, T, H, nd=2, seed=0, packed=False, zero_len=False):
    """float32 inputs of one case, from a seed: xp, whh[nd], bhh[nd], dout (random, never constant), lens or None.
    Cached and shared: do not write to the arrays."""
    rng = np.random.default_rng([seed, G, B, T, H, nd])
    f = np.float32
    d = dict(G=G, B=B, T=T, H=H, nd=nd)
    d['xp'] = (rng.standard_normal((T, B, nd * G * H)) * 0.5).astype(f)
    d['whh'] = [(rng.standard_normal((G * H, H)) * whh_scale(H)).astype(f) for _ in range(nd)]
    d['bhh'] = [(rng.standard_normal(G * H) * 0.1).astype(f) for _ in range(nd)]
    d['dout'] = rng.standard_normal((T, B, nd * H)).astype(f)
    d['lens'] = packed_lens(B, T, rng, zero_len) if packed else None
    for k in ('xp', 'dout'):
        d[k].setflags(write=False)
    return d


def clamp_lens(lens, B, T):
    if lens is None:
        return np.full(B, T, dtype=np.int64)
    return np.clip(np.asarray(lens, dtype=np.int64), 0, T)


def _time_index(d, s, L):
    """time step that launch index s of direction d works on, per item (clipped into range for inactive items)"""
    t = np.full_like(L, s) if d == 0 else L - 1 - s
    return np.clip(t, 0, None)


def rnn_fwd(G, xp, whh, bhh, H, lens=None, dtype=np.float64):
    """-> out [T,B,ND*H], cst (LSTM; None for the GRU), gates [T,B,ND,4H] (zero where never written)"""
    T, B, W = xp.shape
    nd = W // (G * H)
    assert W == nd * G * H and len(whh) >= nd
    xp = np.asarray(xp, dtype=dtype)
    L = clamp_lens(lens, B, T)
    out = np.zeros((T, B, nd * H), dtype=dtype)
    cst = np.zeros((T, B, nd * H), dtype=dtype) if G == 4 else None
    gates = np.zeros((T, B, nd, 4 * H), dtype=dtype)
    rows = np.arange(B)
    for d in range(nd):
        w = np.asarray(whh[d], dtype=dtype).T                    # [H, G*H]
        b = np.asarray(bhh[d], dtype=dtype)
        h = np.zeros((B, H), dtype=dtype)
        c = np.zeros((B, H), dtype=dtype)
        for s in range(T):
            act = s < L
            if not act.any():
                break
            t = _time_index(d, s, L)
            x = xp[t, rows, d * G * H:(d + 1) * G * H]
            hp = h @ w + b
            if G == 3:
                r = sigmoid(x[:, :H] + hp[:, :H])
                z = sigmoid(x[:, H:2 * H] + hp[:, H:2 * H])
                n = np.tanh(x[:, 2 * H:] + r * hp[:, 2 * H:])
                hn = (1 - z) * n + z * h
                sg = np.concatenate([r, z, n, hp[:, 2 * H:]], axis=1)
            else:
                i = sigmoid(x[:, :H] + hp[:, :H])
                f = sigmoid(x[:, H:2 * H] + hp[:, H:2 * H])
                g = np.tanh(x[:, 2 * H:3 * H] + hp[:, 2 * H:3 * H])
                o = sigmoid(x[:, 3 * H:] + hp[:, 3 * H:])
                cn = f * c + i * g
                hn = o * np.tanh(cn)
                sg = np.concatenate([i, f, g, o], axis=1)
                c = np.where(act[:, None], cn, c)
                cst[t[act], rows[act], d * H:(d + 1) * H] = cn[act]
            h = np.where(act[:, None], hn, h)
            out[t[act], rows[act], d * H:(d + 1) * H] = hn[act]
            gates[t[act], rows[act], d] = sg[act]
    return out, cst, gates


def rnn_bwd(G, dout, out, cst, gates, whh, H, lens=None, dtype=np.float64):
    """BPTT from the saved forward state -> dxp, dhp [T,B,2*G*H] (LSTM: dhp is dxp).  whh are the UNtransposed
    [G*H, H] matrices (the kernels take their transposes)."""
    T, B, W = out.shape
    nd = W // H
    K = G * H
    dout, out, gates = (np.asarray(a, dtype=dtype) for a in (dout, out, gates))
    if G == 4:
        cst = np.asarray(cst, dtype=dtype)
    L = clamp_lens(lens, B, T)
    dxp = np.zeros((T, B, nd * K), dtype=dtype)
    dhp = np.zeros((T, B, nd * K), dtype=dtype)
    rows = np.arange(B)
    for d in range(nd):
        w = np.asarray(whh[d], dtype=dtype)                      # [G*H, H]: d(h_prev) = d(hidden pre-activation) @ W_hh
        carry = np.zeros((B, H), dtype=dtype)
        last = np.zeros((B, K), dtype=dtype)                     # d(hidden pre-activation) of the step done before
        for s in range(T):
            act = s < L
            if not act.any():
                break
            t = np.clip(L - 1 - s, 0, None) if d == 0 else np.full_like(L, s)
            tprev = t - 1 if d == 0 else t + 1
            has_prev = (tprev >= 0) & (tprev < L)
            tp = np.clip(tprev, 0, T - 1)
            sg = gates[t, rows, d]
            dh = dout[t, rows, d * H:(d + 1) * H] + last @ w
            state = out if G == 3 else cst
            prev = np.where(has_prev[:, None], state[tp, rows, d * H:(d + 1) * H], 0)
            if G == 3:
                r, z, n, hn = (sg[:, j * H:(j + 1) * H] for j in range(4))
                dh = dh + carry
                dz = dh * (prev - n) * z * (1 - z)
                dn = dh * (1 - z) * (1 - n * n)
                dr = dn * hn * r * (1 - r)
                dx = np.concatenate([dr, dz, dn], axis=1)
                dhh = np.concatenate([dr, dz, dn * r], axis=1)
                ncarry = dh * z
            else:
                i, f, g, o = (sg[:, j * H:(j + 1) * H] for j in range(4))
                tc = np.tanh(cst[t, rows, d * H:(d + 1) * H])
                dc = dh * o * (1 - tc * tc) + carry
                dx = np.concatenate([dc * g * i * (1 - i), dc * prev * f * (1 - f), dc * i * (1 - g * g),
                                     dh * tc * o * (1 - o)], axis=1)
                dhh = dx
                ncarry = dc * f
            carry = np.where(act[:, None], ncarry, carry)
            last = np.where(act[:, None], dhh, last)
            dxp[t[act], rows[act], d * K:(d + 1) * K] = dx[act]
            dhp[t[act], rows[act], d * K:(d + 1) * K] = dhh[act]
    return dxp, dhp


# ---- the entry points, by name -------------------------------------------------------------------------------------
def gru_fwd(xp, whh_f, whh_r, bhh_f, bhh_r, H, dtype=np.float64):
    out, _, gates = rnn_fwd(3, xp, [whh_f, whh_r], [bhh_f, bhh_r], H, None, dtype)
    return out, gates


def gru_fwd_lens(xp, whh_f, whh_r, bhh_f, bhh_r, lens, H, dtype=np.float64):
    return rnn_fwd(3, xp, [whh_f, whh_r], [bhh_f, bhh_r], H, lens, dtype)[0]


def gru_bwd(dout, out, gates, whh_f, whh_r, H, dtype=np.float64):
    return rnn_bwd(3, dout, out, None, gates, [whh_f, whh_r], H, None, dtype)


def lstm_fwd(xp, whh_f, whh_r, bhh_f, bhh_r, lens, H, dtype=np.float64):
    return rnn_fwd(4, xp, [whh_f, whh_r], [bhh_f, bhh_r], H, lens, dtype)


def lstm_bwd(dout, raw, cst, gates, whh_f, whh_r, lens, H, dtype=np.float64):
    """-> dg [T, B, 8H]"""
    return rnn_bwd(4, dout, raw, cst, gates, [whh_f, whh_r], H, lens, dtype)[0]


def lstm_fwd_uni(xp, whh, bhh, H, dtype=np.float64):
    """one direction, zero initial states: xp [T,B,4H] -> out, cst [T,B,H]"""
    out, cst, _ = rnn_fwd(4, xp, [whh], [bhh], H, None, dtype)
    return out, cst


def reference(inp, dtype=np.float64):
    """every output of one case (rnn_inputs) in `dtype`: out, cst, gates, and for nd = 2 dxp, dhp"""
    G, H = inp['G'], inp['H']
    out, cst, gates = rnn_fwd(G, inp['xp'], inp['whh'], inp['bhh'], H, inp['lens'], dtype)
    res = dict(out=out, cst=cst, gates=gates)
    if inp['nd'] == 2:
        res['dxp'], res['dhp'] = rnn_bwd(G, inp['dout'], out, cst, gates, inp['whh'], H, inp['lens'], dtype)
    return res


_ref_cache = {}


def reference64(G, B, T, H, nd=2, seed=0, packed=False, zero_len=False):
    """the float64 reference of a case, computed once and shared: do not write to it"""
    key = (G, B, T, H, nd, seed, packed, zero_len)
    if key not in _ref_cache:
        _ref_cache[key] = reference(rnn_inputs(*key))
    return _ref_cache[key]


def active_mask(lens, B, T):
    """[T, B] bool: t < clamp(lens[b])"""
    return np.arange(T)[:, None] < clamp_lens(lens, B, T)[None, :]


# ---- the shapes of the GPU matrix (tests/test_gpu_rnn_forms.py), shared with the CPU check of the margins -----------
# (G, H) of the width cases, and the (B, T, packed) combinations they run with
WIDTHS = [(3, 16), (3, 48), (3, 64), (3, 128), (3, 256), (3, 272), (3, 512), (3, 704),
          (4, 16), (4, 64), (4, 128), (4, 256), (4, 512), (4, 528)]
BT = [(5, 9, False), (21, 9, False), (33, 9, False), (5, 2, False), (21, 2, False), (33, 2, False), (5, 1, False),
      (21, 12, True), (33, 12, True), (5, 12, True)]
UNI = [(512, 9, 9), (512, 40, 2), (512, 3, 9)]      # ft_lstm_fwd_uni: (H, B, T); rows_per_wg(1, B) = 8 | 8 | 16
