"""The pYIN definition of DESIGN.md section 7 in numpy, twice: pyin64 -- float64, the whole pipeline, with the tables
before their rounding -- and the three stage functions in fp32 (dt=np.float32), which follow the operation orders the
kernels of csrc/ft_pitch.hip follow: p_i is summed over the thresholds in ascending order as (E * C) * bp, the Viterbi
recursion is single adds, subtracts and maxima in the stated order, so its score is reproduced bit for bit.  The one
place that is float64 in both is the parabolic shift and the bin of a candidate, formed from the (fp32 or float64) dn:
three-term differences of fp32 numbers cancel.  Tables and sizes come from forwardtacotron_amd.pitch.pyin_tables, which
tests/test_pyin_cpu.py holds to scipy."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of fp32
FLT_MIN = float(np.finfo(np.float32).tiny)
DENORM = 2.0 ** -149
N_THR = 100


def tables(tb, dt):
    """the tables in dt: float32 -> the rounded ones the kernels get, float64 -> the ones before the rounding"""
    if dt == np.float32:
        t = {k: tb[k] for k in ('thr', 'bp', 'bpc', 'E', 'C', 'logtri', 'lognorm', 'freqs')}
        t.update({k: np.float32(tb[k]) for k in ('ls', 'lw', 'LZ', 'lN')})
        return t
    t = {k: tb['t64'][k] for k in ('thr', 'bp', 'bpc', 'E', 'C', 'logtri', 'lognorm', 'freqs')}
    t.update(ls=np.log(0.99), lw=np.log(0.01), LZ=np.log(FLT_MIN), lN=-np.log(float(tb['N'])))
    return t


def rounded_tables64(tb):
    """the ROUNDED tables held in float64: float64 arithmetic on exactly the numbers the kernels read"""
    t = tables(tb, np.float32)
    return {k: (np.asarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else np.float64(v)) for k, v in t.items()}


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def frames_of(x, fl, hop):
    """[1 + len // hop, fl]: frame t is fl samples from t * hop of x zero-padded by fl // 2 on both sides"""
    T = 1 + len(x) // hop
    pad = np.zeros(len(x) + 2 * (fl // 2) + fl, dtype=x.dtype)
    pad[fl // 2:fl // 2 + len(x)] = x
    return pad[np.arange(T)[:, None] * hop + np.arange(fl)[None, :]]


def cmnd(x, tb, dt=np.float32):
    """-> (d [T, pmax + 1], dn [T, P]) in dt"""
    fr = frames_of(np.asarray(x).astype(dt), tb['frame_length'], tb['hop_length'])
    W, pmin, pmax = tb['W'], tb['pmin'], tb['pmax']
    d = np.empty((fr.shape[0], pmax + 1), dtype=dt)
    for tau in range(pmax + 1):
        df = fr[:, :W] - fr[:, tau:tau + W]
        d[:, tau] = (df * df).sum(axis=1, dtype=dt)
    c = np.cumsum(d[:, 1:], axis=1, dtype=dt) / np.arange(1, pmax + 1).astype(dt)
    dn = d[:, pmin:] / np.maximum(c[:, pmin - 1:], dt(FLT_MIN))
    return d, dn.astype(dt)


def cmnd_bound(dn64, tb):
    """A-priori bound on |dn_fp32 - dn64| for ANY summation order, from the same fp32 samples.  Every term of d is
    non-negative, so |d_32 - d_64| <= e d_64 with e = (W + 2) u (one rounding of the difference, one of the square and
    add, W adds).  The prefix sum over tau non-negative terms adds at most tau - 1 roundings, the division by tau one,
    the final division one: dn_32 / dn_64 <= (1 + e)(1 + u) / ((1 - e)(1 - u)^(tau + 1)), and the lower side deviates
    less.  Valid where c(tau) stays clear of the FLT_MIN floor."""
    e = (tb['W'] + 2) * U
    tau = np.arange(tb['pmin'], tb['pmax'] + 1, dtype=np.float64)
    rel = (1 + e) * (1 + U) / ((1 - e) * (1 - U) ** (tau + 1)) - 1
    return np.abs(dn64) * rel[None, :]


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
def observe_frame(h, tb, dt=np.float32, t=None):
    """one row of dn (dtype dt) -> everything stage 2 defines, as a dict"""
    t = tables(tb, dt) if t is None else t
    P, N, pmin = tb['P'], tb['N'], tb['pmin']
    h = np.asarray(h, dtype=dt)
    tr = np.zeros(P, dtype=bool)
    tr[1:-1] = (h[1:-1] < h[:-2]) & (h[1:-1] <= h[2:])
    tr[0] = h[0] < h[1]
    tr[-1] = h[-1] < h[-2]
    idx = np.flatnonzero(tr)
    hh = h[idx]
    below = hh[:, None] < t['thr'][None, :]
    pos = np.cumsum(below, axis=0) - below
    n = below.sum(axis=0)
    p = np.zeros(len(idx), dtype=dt)
    for k in range(N_THR):
        term = (t['E'][pos[:, k]] * t['C'][n[k]]) * t['bp'][k]
        p = np.where(below[:, k], p + term, p).astype(dt)
    g, m = -1, 0
    if len(idx):
        g = int(np.argmin(hh))                                    # the first, i.e. lowest, trough of minimal height
        m = N_THR - int(below[g].sum())
        p[g] = p[g] + dt(0.01) * t['bpc'][m]
    # candidates: the shift and the bin in float64 from dn
    cand = np.flatnonzero(p > 0)
    ci = idx[cand]
    h64 = h.astype(np.float64)
    shift = np.zeros(len(ci))
    for j, i in enumerate(ci):
        if 0 < i < P - 1:
            a = h64[i - 1] + h64[i + 1] - 2.0 * h64[i]
            b = (h64[i + 1] - h64[i - 1]) / 2.0
            if abs(b) < abs(a):
                shift[j] = -b / a
    f0 = tb['sr'] / ((pmin + ci).astype(np.float64) + shift)
    v = 120.0 * np.log2(f0 / tb['fmin']) + 0.5
    bins = np.floor(v).astype(np.int64)
    bins = np.where(v < 0, 0, bins)
    keep = v < N
    obs = np.zeros(N, dtype=dt)
    for j in np.flatnonzero(keep):                                 # ascending i: the larger i wins a shared bin
        obs[bins[j]] = p[cand[j]]
    vp = dt(min(max(obs.sum(dtype=dt), dt(0)), dt(1)))
    lo_v = np.where(obs > 0, np.log(np.maximum(obs, dt(FLT_MIN))), t['LZ']).astype(dt)
    lo_u = np.log(np.maximum((dt(1) - vp) / dt(N), dt(FLT_MIN))).astype(dt)
    return dict(troughs=idx, below=below, pos=pos, n=n, p=p, g=(int(idx[g]) if g >= 0 else -1), m=m, cand=ci, v=v, bins=bins,
                keep=keep, obs=obs, vp=vp, lo_v=lo_v, lo_u=lo_u)


def observe(dn, tb, dt=np.float32, t=None):
    """dn [T, P] -> (lo_v [T, N], lo_u [T], vp [T], the per-frame dicts)"""
    rows = [observe_frame(h, tb, dt, t) for h in dn]
    return (np.stack([r['lo_v'] for r in rows]), np.array([r['lo_u'] for r in rows], dtype=dt),
            np.array([r['vp'] for r in rows], dtype=dt), rows)


def prob_bound(p64, nterms=N_THR):
    """A-priori bound on |p_fp32 - p64| where p64 is formed in float64 from the ROUNDED tables: a sum of at most 100
    non-negative products of three factors (two roundings each, at most 100 adds), then one product and one add for the
    no-trough term: (nterms + 4) u p, plus a denormal's spacing per term for products that underflow."""
    return (nterms + 4) * U * np.abs(p64) + (nterms + 4) * DENORM


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def _band_max(a, logtri, half):
    """max over k in the band of a[k] + logtri[s - k + half], the lowest k on ties -> (best [N], k [N])"""
    N = len(a)
    pad = np.full(N + 2 * half, -np.inf, dtype=a.dtype)
    pad[half:half + N] = a
    win = np.lib.stride_tricks.sliding_window_view(pad, 2 * half + 1) + logtri[None, :]
    arg = np.argmax(win, axis=1)
    return win[np.arange(N), arg], np.arange(N) - half + arg


def viterbi(lo_v, lo_u, tb, dt=np.float32, t=None):
    """lo_v [T, N], lo_u [T] -> dict(state [T], score, maxima [T], pitch [T]); every operation one add, subtract or
    maximum in dt, in the order of include/fwdtaco_hip.h"""
    t = tables(tb, dt) if t is None else t
    N, half = tb['N'], tb['half']
    lo_v, lo_u = np.asarray(lo_v, dtype=dt), np.asarray(lo_u, dtype=dt)
    T = lo_v.shape[0]
    ls, lw, LZ, lN, ln, lt = dt(t['ls']), dt(t['lw']), dt(t['LZ']), dt(t['lN']), t['lognorm'], t['logtri']
    dv = LZ + lo_v[0]
    du = np.full(N, lN + lo_u[0], dtype=dt)
    mx = max(dv.max(), du.max())
    dv, du = dv - mx, du - mx
    maxima = [mx]
    score = dt(mx)
    back = np.zeros((T, 2 * N), dtype=np.int64)
    for s in range(1, T):
        pv, pu = dv + ls, du + lw
        f1 = pu > pv
        bv, kv = _band_max(np.where(f1, pu, pv) - ln, lt, half)
        qv, qu = dv + lw, du + ls
        f2 = qu > qv
        bu, ku = _band_max(np.where(f2, qu, qv) - ln, lt, half)
        back[s, :N] = kv + np.where(f1[kv], N, 0)
        back[s, N:] = ku + np.where(f2[ku], N, 0)
        nv, nu = bv + lo_v[s], bu + lo_u[s]
        mx = max(nv.max(), nu.max())
        dv, du = nv - mx, nu - mx
        maxima.append(mx)
        score = dt(score + mx)
    state = np.zeros(T, dtype=np.int64)
    state[T - 1] = int(np.argmax(np.concatenate([dv, du])))       # the lowest maximal final state
    for s in range(T - 1, 0, -1):
        state[s - 1] = back[s, state[s]]
    pitch = np.where(state < N, t['freqs'][state % N], 0).astype(dt)
    return dict(state=state, score=score, maxima=np.array(maxima, dtype=dt), pitch=pitch)


def path_is_valid(state, tb):
    """every step stays inside the transition band (a switch of voicing is always legal)"""
    s = np.asarray(state) % tb['N']
    return bool(((np.asarray(state) >= 0) & (np.asarray(state) < 2 * tb['N'])).all() and
                (np.abs(np.diff(s)) <= tb['half']).all())


def path_value(state, lo_v, lo_u, maxima, tb, dt=np.float32, t=None):
    """the normalised log score of `state` itself, accumulated in the recursion's operation order with the optimum's
    normalisers: exactly 0 iff the path attains the optimum (its score is then sum(maxima) + 0)"""
    t = tables(tb, dt) if t is None else t
    N, half = tb['N'], tb['half']
    ls, lw, LZ, lN = dt(t['ls']), dt(t['lw']), dt(t['LZ']), dt(t['lN'])
    s0 = int(state[0])
    v = (LZ + dt(lo_v[0, s0]) if s0 < N else lN + dt(lo_u[0])) - dt(maxima[0])
    for s in range(1, len(state)):
        a, c = int(state[s - 1]), int(state[s])
        same = (a < N) == (c < N)
        v = v + (ls if same else lw)
        v = v - t['lognorm'][a % N]
        v = v + t['logtri'][c % N - a % N + half]
        v = v + (dt(lo_v[s, c]) if c < N else dt(lo_u[s]))
        v = dt(v - dt(maxima[s]))
    return v


# ---- the whole pipeline -----------------------------------------------------------------------------------------------
def pyin(x, tb, dt):
    _, dn = cmnd(x, tb, dt)
    lo_v, lo_u, vp, rows = observe(dn, tb, dt)
    out = viterbi(lo_v, lo_u, tb, dt)
    out.update(dn=dn, lo_v=lo_v, lo_u=lo_u, vp=vp, rows=rows)
    return out


def pyin64(x, tb):
    """the definition in float64 with the unrounded tables -> dict(pitch [T] in Hz, 0 = unvoiced; vp; state; dn; ...)"""
    return pyin(np.asarray(x, dtype=np.float64), tb, np.float64)


def pyin32(x, tb):
    """the fp32 stage functions chained"""
    return pyin(np.asarray(x, dtype=np.float32), tb, np.float32)


# ---- signals ----------------------------------------------------------------------------------------------------------
def tone(f0, n=6000, sr=22050, seed=1):
    ts = np.arange(n) / sr
    x = 0.3 * sum(np.sin(2 * np.pi * k * f0 * ts) / k for k in range(1, 5))
    return (x + 1e-3 * np.random.RandomState(seed).randn(n)).astype(np.float32)


def noise(n=6000, seed=1, amp=0.1):
    return (amp * np.random.RandomState(seed).randn(n)).astype(np.float32)


def vibrato(sr=22050, seed=0):
    n = int(0.6 * sr)
    ts = np.arange(n) / sr
    f0 = 180.0 * 2.0 ** (0.3 * np.sin(2 * np.pi * 2.5 * ts))
    ph = 2 * np.pi * np.cumsum(f0) / sr
    x = 0.3 * sum(np.sin(k * ph) / k for k in range(1, 6))
    rs = np.random.RandomState(seed)
    a, b = int(0.25 * sr), int(0.40 * sr)
    x[a:b] = 0.05 * rs.randn(b - a)
    return (x + 0.002 * rs.randn(n)).astype(np.float32)


# the settings, wav lengths and items of tests/test_gpu_pitch.py (here, so that tests/test_pyin_cpu.py can confirm on the
# CPU what that test relies on, on the same signals)
SETTINGS = {'A': dict(sample_rate=22050, fmin=30, fmax=600, frame_length=2048, hop_length=256),
            'B': dict(sample_rate=8000, fmin=100, fmax=800, frame_length=256, hop_length=64),
            'C': dict(sample_rate=22050, fmin=30, fmax=600, frame_length=2048, hop_length=128)}
LENGTHS = {'A': [0, 1, 255, 256, 257, 2047, 2048, 2049, 6000], 'B': [0, 1, 63, 64, 65, 255, 256, 257, 750]}


def item(name, n):
    """a voiced signal of n samples at the setting's rate: four harmonics of 150 .. 189 Hz and a little noise"""
    ts = np.arange(n) / SETTINGS[name]['sample_rate']
    f0 = 150.0 + n % 40
    x = 0.3 * sum(np.sin(2 * np.pi * k * f0 * ts) / k for k in range(1, 5)) if n else np.zeros(0)
    return (x + 0.01 * np.random.RandomState(7 + n).randn(n)).astype(np.float32)


def cents(f, f0):
    return 1200.0 * np.log2(np.asarray(f, dtype=np.float64) / f0)
