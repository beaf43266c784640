"""CPU: the pYIN host tables (forwardtacotron_amd.pitch.pyin_tables) against scipy, the float64 definition
(tests/pyin_cpu.py pyin64) against ground truth, and the fp32 stage functions chained against pyin64.

Ground truth: harmonic tones 0.3 sum_{k=1..4} sin(2 pi k f0 t) / k + 1e-3 noise, 6000 samples at 22050 Hz; on the frames
that lie wholly inside the signal every frame must be voiced and within 10 cents -- the width of one pitch bin -- of f0.
Zeros and white noise must come out unvoiced on every frame."""
import numpy as np
import pytest
import scipy.signal
import scipy.stats

import pyin_cpu as R
from forwardtacotron_amd import _lib
from forwardtacotron_amd.pitch import (cmnd_lds_bytes, new_pitch_extractor_from_config, pyin_tables,
                                       viterbi_lds_rows)

SHIPPED = dict(sr=22050, fmin=30, fmax=600, frame_length=2048, hop_length=256)
SMALL = dict(sr=8000, fmin=100, fmax=800, frame_length=256, hop_length=64)


@pytest.fixture(scope='module')
def tb():
    return pyin_tables(**SHIPPED)


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 1e-300)))


# ---- 1. the tables ------------------------------------------------------------------------------------------------------
def test_sizes_of_the_shipped_and_the_small_setting(tb):
    assert (tb['pmin'], tb['pmax'], tb['P'], tb['N'], tb['band'], tb['half'], tb['W']) == (36, 735, 700, 519, 51, 25, 1024)
    s = pyin_tables(**SMALL)
    assert (s['pmin'], s['pmax'], s['N'], s['band']) == (10, 80, 361, 31)
    assert 2 * tb['N'] == 1038 > 1024 > 2 * s['N']
    for t in (tb, s):
        assert _lib.query('ft_pyin_cmnd_lds', t['frame_length'], t['hop_length'], t['pmin'], t['pmax']) == \
            cmnd_lds_bytes(t['frame_length'], t['hop_length'], t['pmax'])
    for N, half in ((519, 25), (361, 15), (519, 15), (1024, 1786), (1024, 1787), (1024, 2048), (1, 0), (1025, 5), (8, 2049)):
        want = viterbi_lds_rows(N, half) if N <= 1024 and half <= 2048 else 0
        assert _lib.query('ft_pyin_viterbi_rows', N, half) == want, (N, half)
    assert viterbi_lds_rows(519, 25) == 26 and viterbi_lds_rows(1024, 1786) == 1 and viterbi_lds_rows(1024, 1787) == 0


def test_tables_match_scipy_before_the_rounding(tb):
    t64 = tb['t64']
    edges = np.linspace(0, 1, 101)
    np.testing.assert_array_equal(t64['thr'], np.arange(1, 101) / 100)
    bp = np.diff(scipy.stats.beta.cdf(edges, 2, 18))
    # scipy's differences of two cdf values near 1 cancel: a few ulps of the cdf (of 1), not of the difference
    print('bp: worst |table - scipy| in ulps of 1:', np.max(np.abs(t64['bp'] - bp)) / np.spacing(1.0))
    assert np.max(np.abs(t64['bp'] - bp)) <= 8 * np.spacing(1.0)
    # the tail, which that absolute bound does not see (bp[99] is 1.9e-35): differences of the survival function, which
    # do not cancel there (sf falls by a fifth and more per step from k = 30 on); 1e-12 relative leaves room for scipy's sf
    sf = scipy.stats.beta.sf(edges, 2, 18)
    rel = np.abs(t64['bp'] - (sf[:-1] - sf[1:]))[30:] / t64['bp'][30:]
    print('bp: worst relative |table - scipy sf differences| from k = 30 on:', rel.max())
    assert (t64['bp'] > 0).all() and rel.max() <= 1e-12
    assert t64['bpc'][0] == 0 and t64['bpc'][100] == 1 and len(t64['bpc']) == 101
    assert np.max(np.abs(t64['bpc'] - scipy.stats.beta.cdf(edges, 2, 18))) <= 4 * np.spacing(1.0)
    assert np.max(np.abs(t64['bpc'][1:] - np.cumsum(t64['bp']))) <= 4 * np.spacing(1.0)
    for n in (1, 2, 3, 7, 40, tb['nE'] - 1):
        pos = np.arange(n)
        want = scipy.stats.boltzmann.pmf(pos, 2, n)
        got = t64['E'][pos] * t64['C'][n]
        assert _ulps(got, want) <= 8, (n, _ulps(got, want))
    want = scipy.signal.get_window('triangle', tb['band'], fftbins=False)
    assert _ulps(t64['tri'], want) <= 4
    np.testing.assert_allclose(t64['freqs'], 30 * 2.0 ** (np.arange(519) / 120), rtol=1e-15)
    # rounded once
    for k in ('thr', 'bp', 'bpc', 'E', 'C', 'logtri', 'lognorm', 'freqs'):
        assert tb[k].dtype == np.float32
        np.testing.assert_array_equal(tb[k], t64[k].astype(np.float32))
    assert tb['LZ'] == float(np.float32(np.log(R.FLT_MIN))) and tb['lN'] == float(np.float32(-np.log(519)))


@pytest.mark.parametrize('setting', [SHIPPED, SMALL])
def test_every_row_of_the_implied_transition_matrix_sums_to_one(setting):
    t = pyin_tables(**setting)
    N, half, tri, norm = t['N'], t['half'], t['t64']['tri'], t['t64']['norm']
    local = np.zeros((N, N))
    for k in range(N):
        lo, hi = max(0, k - half), min(N - 1, k + half)
        local[k, lo:hi + 1] = tri[lo - k + half:hi - k + half + 1] / norm[k]
    full = np.kron(np.array([[.99, .01], [.01, .99]]), local)
    assert np.max(np.abs(full.sum(axis=1) - 1)) <= 1e-12


def test_argument_checks():
    with pytest.raises(_lib.FtError, match='LDS plan'):          # N = 1024 with a band of 3881 bins: no back-pointer row fits
        pyin_tables(sr=1000, fmin=1, fmax=369, frame_length=1024, hop_length=900)
    for bad in (dict(frame_length=2047), dict(frame_length=2), dict(fmin=0), dict(fmin=-1.0), dict(fmax=30), dict(fmax=20),
                dict(frame_length=64),                       # pmax < pmin + 2
                dict(fmin=1, fmax=11000, frame_length=2048),   # 2N beyond the Viterbi kernel's plan
                dict(frame_length=4096, fmin=8)):              # more periods than the observation kernel holds
        with pytest.raises(_lib.FtError):
            pyin_tables(**{**SHIPPED, **bad})
    cfg = {'preprocessing': {'pitch_extractor': 'pyworld', 'pitch_min_freq': 30, 'pitch_max_freq': 600,
                             'pitch_frame_length': 2048}, 'dsp': {'sample_rate': 22050, 'hop_length': 256}}
    with pytest.raises(_lib.FtError, match='DIO'):
        new_pitch_extractor_from_config(cfg)
    cfg['preprocessing']['pitch_extractor'] = 'crepe'
    with pytest.raises(ValueError, match=r'Invalid pitch extractor type: crepe, choices: \[librosa, pyworld\]\.'):
        new_pitch_extractor_from_config(cfg)


# ---- 2. the definition against ground truth ----------------------------------------------------------------------------
def inside(n, tb):
    """the frames that lie wholly inside an n-sample signal"""
    hop, fl = tb['hop_length'], tb['frame_length']
    t = np.arange(1 + n // hop)
    return (t * hop >= fl // 2) & (t * hop + fl // 2 <= n)


@pytest.mark.parametrize('f0', [40, 55, 110, 220, 440, 587])
def test_pyin64_finds_a_harmonic_tone_within_one_bin(tb, f0):
    out = R.pyin64(R.tone(f0), tb)
    sel = inside(6000, tb)
    assert sel.sum() == 16 and len(sel) == 24
    assert (out['pitch'][sel] > 0).all()
    c = np.abs(R.cents(out['pitch'][sel], f0))
    print(f'tone {f0} Hz: worst {c.max():.2f} cents, voiced probability >= {out["vp"][sel].min():.4f}')
    assert c.max() <= 10.0


def test_pyin64_calls_zeros_and_noise_unvoiced(tb):
    out = R.pyin64(np.zeros(3000, dtype=np.float32), tb)
    assert len(out['pitch']) == 12 and not out['pitch'].any() and not out['vp'].any() and not out['dn'].any()
    out = R.pyin64(R.noise(), tb)
    print(f'noise: largest voiced probability {out["vp"].max():.4f}')
    assert not out['pitch'].any()


# ---- 3. fp32 against float64 -----------------------------------------------------------------------------------------
def test_fp32_stage_functions_chained_agree_with_pyin64_on_the_vibrato_signal(tb):
    x = R.vibrato()
    a, b = R.pyin64(x, tb), R.pyin32(x, tb)
    T = len(a['pitch'])
    assert T == 52 == len(b['pitch'])
    print(f'vibrato: max |dn32 - dn64| = {np.abs(b["dn"].astype(np.float64) - a["dn"]).max():.2e}')
    assert (np.abs(b['dn'].astype(np.float64) - a['dn']) <= R.cmnd_bound(a['dn'], tb)).all()
    same = a['pitch'] == b['pitch'].astype(np.float64)                 # the bin of an unvoiced state means nothing
    same |= (a['state'] < tb['N']) & (a['state'] == b['state'])
    print(f'vibrato: the same f0 on {same.sum()} of {T} frames')
    assert same.sum() >= 0.95 * T
    va = a['state'] < tb['N']
    change = np.flatnonzero(np.diff(va.astype(int)) != 0)              # voicing changes between t and t + 1
    for t in np.flatnonzero(~same):
        vb = b['state'][t] < tb['N']
        if va[t] == vb:
            assert va[t] and abs(int(a['state'][t]) - int(b['state'][t])) <= 1, t
        else:
            assert any(abs(t - c) <= 2 or abs(t - (c + 1)) <= 2 for c in change), t
    # the candidate bins of the fp32 restatement against float64 from the SAME dn: inside the cap the GPU test relies on
    tot = off = 0
    for h in b['dn']:
        r32 = R.observe_frame(h, tb, np.float32)
        r64 = R.observe_frame(h.astype(np.float64), tb, np.float64, R.rounded_tables64(tb))
        at = np.searchsorted(r64['cand'], r32['cand'])              # fp32's candidates are float64's, less those whose
        assert np.array_equal(r64['cand'][at], r32['cand'])         # p underflows in fp32 (E[pos] beyond pos = 51)
        tot += len(r32['cand'])
        off += int((r32['bins'] != r64['bins'][at]).sum())
    assert off <= 0.01 * tot


@pytest.mark.parametrize('name', ['A', 'B'])
def test_fp32_bins_against_float64_on_the_items_of_the_gpu_test(name):
    """what tests/test_gpu_pitch.py relies on for its 1 % cap, on its own signals and seeds: from the same fp32 dn, the
    fp32 restatement's candidates are float64's (less those whose p underflows) and sit in float64's bins"""
    cfg = R.SETTINGS[name]
    t = pyin_tables(cfg['sample_rate'], cfg['fmin'], cfg['fmax'], cfg['frame_length'], cfg['hop_length'])
    t64r = R.rounded_tables64(t)
    tot = off = 0
    for n in R.LENGTHS[name]:
        for h in R.cmnd(R.item(name, n), t, np.float32)[1]:
            r32 = R.observe_frame(h, t, np.float32)
            r64 = R.observe_frame(h.astype(np.float64), t, np.float64, t64r)
            at = np.searchsorted(r64['cand'], r32['cand'])
            assert np.array_equal(r64['cand'][at], r32['cand'])
            tot += len(r32['cand'])
            off += int((r32['bins'] != r64['bins'][at]).sum())
    print(f'setting {name}: {off} of {tot} candidates in another bin')
    assert tot > 20 and off <= 0.01 * tot
