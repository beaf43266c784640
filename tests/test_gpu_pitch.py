"""GPU: pYIN of a ragged batch (pitch.LibrosaPitchExtractor; ft_pyin_cmnd, ft_pyin_observe, ft_pyin_viterbi of
csrc/ft_pitch.hip), stage by stage against the restatements of tests/pyin_cpu.py, and end to end.

Settings: A = the shipped config (22050 Hz, 30-600 Hz, frame 2048, hop 256: P = 700 periods, N = 519 bins, 2N = 1038
states > the Viterbi's 1024 threads, a band of 51) and B = 8000 Hz, 100-800 Hz, frame 256, hop 64 (periods 10..80, N =
361, a band of 31, fewer states than threads); for the Viterbi also C = A at hop 128 (a band of 31 with 1038 states:
the any-band kernel with states beyond its 1024 threads, where A runs the kernel specialised for its band of 51).  Wav
lengths [0, 1, 255, 256, 257, 2047, 2048, 2049, 6000] for A and the
same points scaled to hop 64 / frame 256 for B: an empty item, fewer samples than the padding, one sample either side
of a frame boundary and of the frame length; batched in mixed order, so the four-frame run of a difference-kernel
workgroup crosses the end of an item.

What is exact and what is bounded:
  stage 1  dn against float64 from the same fp32 samples, inside the a-priori bound pyin_cpu.cmnd_bound (any summation
           order); zero frames exactly 0.
  stage 2  fed the kernel's own dn: troughs, below(i, k), pos(i, k), n(k), g, m and the candidate periods equal the fp32
           restatement exactly (the kernel's test outputs prob, info and pos; crafted rows with a trough at every other
           period take pos across the waves of the workgroup, which E's underflow from pos 52 on hides from p_i); p_i
           and vp inside
           the a-priori bound of a 100-term non-negative fp32 sum of three-factor products (pyin_cpu.prob_bound); a
           candidate's bin equals the float64 bin from the same dn, a neighbouring bin only where the unrounded value is
           within 1e-3 of the boundary and on at most 1 % of the candidates; lo_v and lo_u after exp: the stored fp32
           logarithm may be off by 4 of its own ulps, i.e. |exp(lo) / x - 1| <= 4 max(ulp(lo), 2^-24) (a 4-ulp bound on
           exp(lo) itself cannot be met by any fp32 logarithm: half an ulp of lo = -46 is already 32 ulps of its exp).
  stage 3  fed arbitrary fp32 observations: score bit-equal to the fp32 restatement, the path valid, the path's own score
           accumulated along it equal to the optimum bit for bit, pitch exactly freqs[state mod N] or 0.
  end to end  the tone / zeros / noise assertions of tests/test_pyin_cpu.py; bits independent of batch, padding,
           poisoned buffers and neighbours."""
import os

import numpy as np
import pytest
import torch

import pyin_cpu as R
from poison import poison as _poison

pytestmark = pytest.mark.gpu

SETTINGS, LENGTHS = R.SETTINGS, R.LENGTHS                       # A, B and, for the Viterbi, C; the lengths of A and B
ORDER = [[8, 0, 7, 1, 3], [2, 6, 4, 5]]                         # two batches of indices into LENGTHS, mixed

_ext, _items, _runs = {}, {}, {}


def ext(name):
    from forwardtacotron_amd.pitch import LibrosaPitchExtractor
    if name not in _ext:
        _ext[name] = LibrosaPitchExtractor(**SETTINGS[name])
    return _ext[name]


def item(name, n):
    if (name, n) not in _items:
        _items[(name, n)] = R.item(name, n)
    return _items[(name, n)]


def stages(name, lens, debug=True):
    """every intermediate of the three launches for the items of these lengths, as numpy"""
    e = ext(name)
    wav, dlens, Lmax = e._gather([item(name, n) for n in lens])
    out = e.stages(wav, dlens, Lmax, debug=debug)
    return {k: v.cpu().numpy() for k, v in out.items()}


def run(name, j):
    if (name, j) not in _runs:
        _runs[(name, j)] = stages(name, [LENGTHS[name][i] for i in ORDER[j]])
    return _runs[(name, j)]


@pytest.fixture(scope='module', params=['A', 'B'])
def name(request):
    return request.param


# ---- stage 1 ----------------------------------------------------------------------------------------------------------
def test_stage1_difference_function_within_the_a_priori_bound(name):
    tb = ext(name).tables
    worst = 0.0
    for j in range(len(ORDER)):
        out = run(name, j)
        lens = [LENGTHS[name][i] for i in ORDER[j]]
        assert out['dn'].shape == (len(lens), 1 + max(lens) // tb['hop_length'], tb['P']) and out['dn'].dtype == np.float32
        for b, n in enumerate(lens):
            T = 1 + n // tb['hop_length']
            assert out['frames'][b] == T
            assert not out['dn'][b, T:].any()                              # exactly 0 past the item's frames
            _, dn64 = R.cmnd(item(name, n), tb, np.float64)
            got = out['dn'][b, :T].astype(np.float64)
            assert np.isfinite(got).all()
            assert not got[dn64 == 0].any()                                # zero (parts of) frames: exactly 0
            bnd = R.cmnd_bound(dn64, tb)
            sel = bnd > 0
            if sel.any():
                worst = max(worst, float((np.abs(got - dn64)[sel] / bnd[sel]).max()))
            if n == 0:
                assert not got.any()
    print(f'stage 1 {name}: worst |gpu - fp64| / bound = {worst:.3f}')
    assert worst <= 1.0


# ---- stage 2 ----------------------------------------------------------------------------------------------------------
def _log_close(lo, x):
    """exp(lo) against x > 0: the stored logarithm within 4 of its ulps"""
    lo = np.asarray(lo, dtype=np.float32)
    tol = 4 * np.maximum(np.spacing(np.abs(lo)).astype(np.float64), R.U)
    return np.abs(np.exp(lo.astype(np.float64)) / x - 1.0) <= np.expm1(tol)


def check_observe_frame(tb, t64r, h, prob, info, pos, lo_v, lo_u, vp, stats):
    """one frame of ft_pyin_observe against the restatements from the same fp32 dn row h"""
    N, LZ = tb['N'], np.float32(tb['LZ'])
    r32 = R.observe_frame(h, tb, np.float32)
    r64 = R.observe_frame(h.astype(np.float64), tb, np.float64, t64r)
    assert np.array_equal(np.flatnonzero(prob != -1), r32['troughs'])
    assert np.array_equal(info[2:], r32['n']) and info[0] == r32['g'] and info[1] == r32['m']
    notr = np.ones(len(prob), dtype=bool)
    notr[r32['troughs']] = False
    assert (pos[notr] == -1).all()
    assert np.array_equal(pos[r32['troughs']] >= 0, r32['below'])              # below(i, k), every trough and threshold
    assert np.array_equal(pos[r32['troughs']], np.where(r32['below'], r32['pos'], -1))      # pos(i, k)
    stats['maxpos'] = max(stats.get('maxpos', 0), int(pos.max()))
    assert np.array_equal(np.flatnonzero(prob > 0), r32['cand'])
    pg = prob[r32['troughs']].astype(np.float64)
    assert np.array_equal(r64['troughs'], r32['troughs'])
    bnd = R.prob_bound(r64['p'])
    err = np.abs(pg - r64['p'])
    if len(err):
        stats['p'] = max(stats['p'], float((err / bnd).max()))
    assert (err <= bnd).all()
    # bins: float64 from the same dn, over the kernel's candidates
    at = np.searchsorted(r64['cand'], r32['cand'])
    assert np.array_equal(r64['cand'][at], r32['cand'])
    v, bins, keep = r64['v'][at], r64['bins'][at].copy(), r64['keep'][at]
    pc = prob[r32['cand']]

    def expected(bins):
        obs = np.zeros(N, dtype=np.float32)
        for j in np.flatnonzero(keep):
            obs[bins[j]] = pc[j]
        return obs
    obs = expected(bins)
    got_nz = lo_v != LZ
    stats['cands'] += len(bins)

    def wrong(obs):
        """bins whose lo_v contradicts obs: LZ under a p clear of the FLT_MIN floor, or not LZ where no candidate sits (a
        p at or below the floor gives log(FLT_MIN), which the device's logf may round one ulp off the table's LZ)"""
        return int((~got_nz & (obs > np.float32(1.0001 * R.FLT_MIN))).sum() + (got_nz & (obs == 0)).sum())
    if wrong(obs):
        for j in np.flatnonzero(np.abs(v - np.round(v)) < 1e-3):               # at the boundary between two bins
            alt = bins.copy()
            alt[j] = int(np.round(v[j])) - (1 if v[j] >= np.round(v[j]) else 0)
            if 0 <= alt[j] < N and wrong(expected(alt)) < wrong(expected(bins)):
                bins = alt
                stats['offbin'] += 1
        obs = expected(bins)
        assert wrong(obs) == 0
    nz = obs > 0
    assert _log_close(lo_v[nz], np.maximum(obs[nz].astype(np.float64), R.FLT_MIN)).all()
    assert (lo_v[~nz] == LZ).all()
    s64 = float(obs.astype(np.float64).sum())
    vp64 = min(max(s64, 0.0), 1.0)
    assert abs(float(vp) - vp64) <= (N + 104) * R.U * s64 + R.U
    assert _log_close(lo_u, max((1.0 - float(vp)) / N, R.FLT_MIN))


def test_stage2_observations_from_the_kernels_own_dn(name):
    tb = ext(name).tables
    t64r = R.rounded_tables64(tb)
    stats = dict(p=0.0, cands=0, offbin=0)
    for j in range(len(ORDER)):
        out = run(name, j)
        for b in range(out['dn'].shape[0]):
            T = int(out['frames'][b])
            for t in range(out['dn'].shape[1]):
                if t < T:
                    check_observe_frame(tb, t64r, out['dn'][b, t], out['prob'][b, t], out['info'][b, t], out['pos'][b, t],
                                        out['lo_v'][b, t], out['lo_u'][b, t], out['vp'][b, t], stats)
                else:                                                       # past the item: a frame of dn = 0
                    assert (out['lo_v'][b, t] == np.float32(tb['LZ'])).all() and out['vp'][b, t] == 0
                    assert (out['prob'][b, t] == -1).all() and out['info'][b, t, 0] == -1 and not out['info'][b, t, 1:].any()
                    assert (out['pos'][b, t] == -1).all()
    print(f'stage 2 {name}: worst |p - p64| / bound = {stats["p"]:.3f}; {stats["offbin"]} of {stats["cands"]} candidates '
          f'in a neighbouring bin')
    assert stats["cands"] > 20 and stats['offbin'] <= 0.01 * stats['cands']


def test_stage2_crafted_rows(name):
    from forwardtacotron_amd import hip as H
    e = ext(name)
    tb = e.tables
    P, N = tb['P'], tb['N']
    rows = np.ones((7, P), dtype=np.float32)
    rows[0, P - 40], rows[0, P - 38] = 0.05, 0.06            # A: two troughs that share a bin; the larger period wins
    rows[1, P // 3], rows[1, P // 2] = 0.125, 0.125          # equal heights: g is the lower one
    rows[2, 0] = 0.02                                        # period pmin: above fmax, its bin is beyond N - 1
    rows[2, P // 2] = 0.3
    rows[3, P - 1] = 0.04                                    # a trough at the last period: no shift
    rows[4] = np.linspace(1.0, 2.0, P)                       # one trough, at i = 0, at height 1: below no threshold
    rows[5, 1::2] = np.linspace(0.004, 0.996, len(rows[5, 1::2]))      # a trough at every other period, rising: P // 2 of
    rows[6, 1::2] = np.linspace(0.996, 0.004, len(rows[6, 1::2]))      # them, more than a wave holds (A: 350, pos to 349)
    dn = torch.from_numpy(rows[None]).to(e.device)
    frames = torch.tensor([7], dtype=torch.int64, device=e.device)
    out = {k: v.cpu().numpy() for k, v in H.pyin_observe(dn, frames, tb, e._dev, debug=True).items()}
    stats = dict(p=0.0, cands=0, offbin=0)
    t64r = R.rounded_tables64(tb)
    for t in range(7):
        check_observe_frame(tb, t64r, rows[t], out['prob'][0, t], out['info'][0, t], out['pos'][0, t], out['lo_v'][0, t],
                            out['lo_u'][0, t], out['vp'][0, t], stats)
    assert stats['offbin'] == 0
    assert stats['maxpos'] == P // 2 - 1                     # counts that cross the waves of the workgroup
    r = [R.observe_frame(rows[t], tb, np.float32) for t in range(7)]
    if name == 'A':
        assert len(r[0]['cand']) == 2 and r[0]['bins'][0] == r[0]['bins'][1]
        b = r[0]['bins'][0]
        assert np.exp(out['lo_v'][0, 0, b]) == pytest.approx(float(out['prob'][0, 0, P - 38]), rel=1e-5)
        assert (out['lo_v'][0, 0] != np.float32(tb['LZ'])).sum() == 1
        assert not r[2]['keep'][0] and r[2]['keep'][1] and (out['lo_v'][0, 2] != np.float32(tb['LZ'])).sum() == 1
        assert out['vp'][0, 4] == 0                          # its only candidate is beyond the top bin
    assert out['info'][0, 1, 0] == P // 3 and r[1]['g'] == P // 3
    assert out['info'][0, 4, 0] == 0 and out['info'][0, 4, 1] == 100


# ---- stage 3 ----------------------------------------------------------------------------------------------------------
def _observations(name, kind, T, frames):
    e = ext(name)
    tb = e.tables
    N, LZ = tb['N'], tb['LZ']
    rs = np.random.RandomState(100 * T + len(kind))
    if kind == 'random':
        return (rs.uniform(LZ, 0, (3, T, N)).astype(np.float32), rs.uniform(LZ, 0, (3, T)).astype(np.float32))
    if kind == 'equal':
        return np.full((3, T, N), -1.0, dtype=np.float32), np.full((3, T), -1.0, dtype=np.float32)
    out = stages(name, [tb['hop_length'] * (f - 1) + 3 for f in frames], debug=False)
    assert out['frames'].tolist() == list(frames)
    return out['lo_v'], out['lo_u']


@pytest.mark.parametrize('T', [1, 2, 3, 40])
@pytest.mark.parametrize('kind', ['random', 'equal', 'own'])
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_stage3_viterbi_score_path_and_pitch(name, kind, T):
    from forwardtacotron_amd import hip as H
    e = ext(name)
    tb = e.tables
    N = tb['N']
    frames = [T, max(1, T // 2), max(1, T - 1)]
    lo_v, lo_u = _observations(name, kind, T, frames)
    out = H.pyin_viterbi(torch.from_numpy(lo_v).to(e.device), torch.from_numpy(lo_u).to(e.device),
                         torch.tensor(frames, dtype=torch.int64, device=e.device), tb, e._dev, alloc=_poison)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    for b, Tb in enumerate(frames):
        ref = R.viterbi(lo_v[b, :Tb], lo_u[b, :Tb], tb, np.float32)
        assert out['score'][b].tobytes() == np.float32(ref['score']).tobytes(), (b, out['score'][b], ref['score'])
        st = out['state'][b, :Tb]
        assert R.path_is_valid(st, tb)
        assert R.path_value(st, lo_v[b], lo_u[b], ref['maxima'], tb, np.float32) == 0.0
        want = np.where(st < N, tb['freqs'][st % N], np.float32(0))
        assert out['pitch'][b, :Tb].tobytes() == want.astype(np.float32).tobytes()
        assert (out['state'][b, Tb:] == -1).all() and not out['pitch'][b, Tb:].any()


# ---- end to end -------------------------------------------------------------------------------------------------------
def _inside(n, tb):
    t = np.arange(1 + n // tb['hop_length'])
    return (t * tb['hop_length'] >= tb['frame_length'] // 2) & (t * tb['hop_length'] + tb['frame_length'] // 2 <= n)


def test_tones_zeros_and_noise_through_extract_batch_and_call():
    e = ext('A')
    tb = e.tables
    f0s = [40, 55, 110, 220, 440, 587]
    wavs = [R.tone(f) for f in f0s] + [np.zeros(3000, dtype=np.float32), R.noise()]
    res = e.extract_batch(wavs)
    pitch, plen, vp = (res[k].cpu().numpy() for k in ('pitch', 'pitch_len', 'voiced_prob'))
    assert plen.tolist() == [24] * 6 + [12, 24] and plen.dtype == np.int64
    sel = _inside(6000, tb)
    for b, f0 in enumerate(f0s):
        assert (pitch[b, :24][sel] > 0).all()
        c = np.abs(R.cents(pitch[b, :24][sel], f0))
        print(f'tone {f0} Hz on the GPU: worst {c.max():.2f} cents, voiced probability >= {vp[b, :24][sel].min():.4f}')
        assert c.max() <= 10.0
    assert not pitch[6].any() and not vp[6].any()
    print(f'noise on the GPU: largest voiced probability {vp[7].max():.4f}')
    assert not pitch[7].any()
    for b, w in enumerate(wavs):                                            # __call__: the same bits, numpy in -> numpy out
        one = e(w)
        assert isinstance(one, np.ndarray) and one.dtype == np.float32 and one.shape == (plen[b],)
        assert one.tobytes() == pitch[b, :plen[b]].tobytes()
    dev = e(torch.from_numpy(wavs[3]).to(e.device))
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.cpu().numpy().tobytes() == pitch[3, :24].tobytes()


def _bits(res, b, T):
    return res['pitch'][b, :T].cpu().numpy().tobytes() + res['voiced_prob'][b, :T].cpu().numpy().tobytes()


def test_an_item_gives_the_same_bits_alone_and_at_every_position_of_a_batch(name):
    e = ext(name)
    hop = e.tables['hop_length']
    lens = LENGTHS[name]
    alone = {}
    for n in lens:
        r = e.extract_batch([item(name, n)])
        assert r['pitch_len'].tolist() == [1 + n // hop] and r['pitch'].shape == (1, 1 + n // hop)
        alone[n] = _bits(r, 0, 1 + n // hop)
    for order in (lens, lens[::-1], [lens[i] for i in ORDER[0]]):
        r = e.extract_batch([item(name, n) for n in order])
        pitch, vp = r['pitch'].cpu().numpy(), r['voiced_prob'].cpu().numpy()
        for b, n in enumerate(order):
            T = 1 + n // hop
            assert r['pitch_len'][b] == T and _bits(r, b, T) == alone[n], (order, n)
            assert not pitch[b, T:].any() and not vp[b, T:].any()           # defined past the item: 0


def test_nan_padding_poisoned_buffers_and_a_nan_item_change_no_bit(name, monkeypatch):
    from forwardtacotron_amd import pitch as Pm
    e = ext(name)
    hop = e.tables['hop_length']
    lens = [LENGTHS[name][i] for i in ORDER[0]]
    L = max(lens)
    clean = e.extract_batch([item(name, n) for n in lens])
    want = [_bits(clean, b, 1 + n // hop) for b, n in enumerate(lens)]
    host = np.full((len(lens), L), np.nan, dtype=np.float32)               # NaN beyond every wav_len
    for b, n in enumerate(lens):
        host[b, :n] = item(name, n)
    monkeypatch.setattr(Pm, '_empty', _poison)                             # every buffer and workspace NaN-poisoned
    wl = torch.tensor(lens, dtype=torch.int64)
    r = e.extract_batch(torch.from_numpy(host).to(e.device), wl)
    assert [_bits(r, b, 1 + n // hop) for b, n in enumerate(lens)] == want
    rd = e.extract_batch(torch.from_numpy(host).to(e.device), wl.to(e.device))     # wav_len on the device: the same bits
    assert [_bits(rd, b, 1 + n // hop) for b, n in enumerate(lens)] == want
    assert rd['pitch_len'].tolist() == [1 + n // hop for n in lens]
    host[0, :] = np.nan                                                    # a NaN item: it finishes, the others keep their bits
    host[0, 100] = np.inf
    r = e.extract_batch(torch.from_numpy(host).to(e.device), wl)
    torch.cuda.synchronize()
    assert [_bits(r, b, 1 + n // hop) for b, n in enumerate(lens)][1:] == want[1:]
    st = r['pitch'][0].cpu().numpy()
    assert np.isfinite(st).all()


def test_pitch_len_is_the_mel_len_of_preprocess_batch():
    from forwardtacotron_amd.audio import DSP
    e = ext('A')
    dsp = DSP(num_mels=80, sample_rate=22050, hop_length=256, win_length=1024, n_fft=1024, fmin=0, fmax=8000,
              trim_start_end_silence=True, peak_norm=True)
    wavs = [np.concatenate([np.zeros(700, np.float32), R.tone(220, 5000), np.zeros(300, np.float32)]), R.tone(110, 3333),
            R.tone(440, 2048)]
    out = dsp.preprocess_batch(wavs)
    res = e.extract_batch(out['wav'], out['wav_len'])
    assert torch.equal(res['pitch_len'], out['mel_len'])
    assert torch.equal(res['pitch_len'], 1 + out['wav_len'] // 256)
    assert res['pitch'].shape == (3, 1 + out['wav'].shape[1] // 256) and res['pitch'].is_cuda


def test_write_raw_pitch_feeds_the_token_values(tmp_path):
    from forwardtacotron_amd.pitch import write_raw_pitch
    from forwardtacotron_amd.pitch_energy import TokenValues, _raw_pitch
    e = ext('A')
    tb = e.tables
    x = R.tone(220)
    res = e.extract_batch([x, R.tone(110, 3000)])
    paths = write_raw_pitch(res, ['a_01', 'b_02'], tmp_path / 'raw_pitch')
    assert [os.path.basename(p) for p in paths] == ['a_01.npy', 'b_02.npy']
    track = np.load(paths[0], allow_pickle=False)
    assert track.dtype == np.float32 and track.shape == (24,) and np.load(paths[1]).shape == (12,)
    assert track.tobytes() == res['pitch'][0, :24].cpu().numpy().tobytes()
    pitch, plen = _raw_pitch(tmp_path / 'raw_pitch', ['a_01'])
    dur = torch.tensor([[4, 16, 4]], dtype=torch.int64, device=e.device)      # the middle token: the 16 frames inside
    mel = torch.from_numpy(np.random.RandomState(3).uniform(-8, 0, (1, 80, 24)).astype(np.float32)).to(e.device)
    tv = TokenValues.extract_batch(mel, torch.tensor([24]), pitch.to(e.device), plen, dur, torch.tensor([3]), 30.0, 600.0)
    got = tv.pitch[0].cpu().numpy()
    ref = R.pyin64(x, tb)
    f64 = np.where(ref['state'] < tb['N'], tb['freqs'].astype(np.float64)[ref['state'] % tb['N']], 0.0)

    def mean(v):
        v = v[(v != 0) & (v >= 30.0) & (v <= 600.0)]
        return np.float32(v.mean()) if len(v) else np.float32(0)
    assert got[1] == mean(f64[4:20])                                          # the float64 path's token mean
    assert got[0] == mean(track[:4].astype(np.float64)) and got[2] == mean(track[20:].astype(np.float64))


def test_config_errors():
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd.pitch import LibrosaPitchExtractor, new_pitch_extractor_from_config
    cfg = {'preprocessing': {'pitch_extractor': 'librosa', 'pitch_min_freq': 30, 'pitch_max_freq': 600,
                             'pitch_frame_length': 2048}, 'dsp': {'sample_rate': 22050, 'hop_length': 256}}
    e = new_pitch_extractor_from_config(cfg)
    assert isinstance(e, LibrosaPitchExtractor) and (e.tables['P'], e.tables['N']) == (700, 519)
    cfg['preprocessing']['pitch_extractor'] = 'pyworld'
    with pytest.raises(_lib.FtError, match='DIO'):
        new_pitch_extractor_from_config(cfg)
    cfg['preprocessing']['pitch_extractor'] = 'yin'
    with pytest.raises(ValueError, match='Invalid pitch extractor type: yin'):
        new_pitch_extractor_from_config(cfg)
    for bad in (dict(frame_length=2047), dict(frame_length=2), dict(frame_length=64), dict(fmin=0), dict(fmax=30),
                dict(fmin=1, fmax=11000)):
        with pytest.raises(_lib.FtError):
            LibrosaPitchExtractor(**{**SETTINGS['A'], **bad})
    with pytest.raises(_lib.FtError):
        e.extract_batch(torch.zeros(2, 100, device='cuda'), torch.tensor([5, 101]))        # a host wav_len beyond L
    with pytest.raises(_lib.FtError):
        e.extract_batch(torch.zeros(2, 100, device='cuda'))                                 # a padded batch without wav_len
