"""GPU: the audio front end (forwardtacotron_amd/audio.py; ft_wav_trim_peak / ft_wav_pack / ft_mel_project and the DFT
GEMM between them) against the float64 restatement tests/mel_cpu.py.

Exact: the trim bounds and every length (tests/test_mel_cpu.py asserts that no frame of the test items lies within 3 dB
of the threshold), the scaled wav (bit-equal to numpy float32: one IEEE division, one multiplication), the padding, and
an item alone against the same item inside a batch.
Log-mel tolerance: the error of an fp32 CPU route (frames x DFT matrices in numpy float32, mel_cpu.wav_to_mel_fp32)
against float64 is computed on the same inputs; the device may be at most MARGIN = 8 times that, in the log domain and,
relative to the item's largest value, in the linear domain.  The margin covers the library's fp32 GEMM being a
three-term bf16 split rather than an IEEE fma chain (the STFT test of the vocoder allows 2e-5 of scale for the same
reason).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import mel_cpu as R
from poison import poison as _poison

pytestmark = pytest.mark.gpu

MARGIN = 8.0
PAD32 = np.float32(R.PAD)


def _dsp(**over):
    from forwardtacotron_amd.audio import DSP
    return DSP.from_config({'dsp': dict(R.CFG, **over)})


@pytest.fixture(scope='module')
def items():
    return R.items()


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_mel(name, got_log, ref_log, z, cfg, pad_mode='constant'):
    """device log-mel against float64, bounded by MARGIN x the fp32 CPU route's own error on the same wav"""
    e_ref = np.abs(R.wav_to_mel_fp32(z, cfg, pad_mode=pad_mode) - ref_log).max()
    e_dev = np.abs(got_log.astype(np.float64) - ref_log).max()
    print(f'{name}: log-mel error {e_dev:.3e}, fp32 CPU route {e_ref:.3e}, ratio {e_dev / e_ref:.2f}')
    assert e_dev <= MARGIN * e_ref, (name, e_dev, e_ref)


def test_trim_bounds_and_lengths_equal_the_oracle(items):
    dsp = _dsp()
    out = _host(dsp.preprocess_batch(items))
    hop = R.CFG['hop_length']
    Lmax = max(len(y) for y in items)
    assert out['mel'].shape == (4, 80, 1 + Lmax // hop) and out['wav'].shape == (4, Lmax)
    for k in ('mel_len', 'trim_start', 'trim_end', 'wav_len'):
        assert out[k].dtype == np.int64 and out[k].shape == (4,)
    for b, (y, want) in enumerate(zip(items, R.TRIM_BOUNDS)):
        r = R.preprocess(y)
        assert (r['trim_start'], r['trim_end']) == want
        assert (int(out['trim_start'][b]), int(out['trim_end'][b])) == want, b
        assert int(out['mel_len'][b]) == 1 + (want[1] - want[0]) // hop == r['mel_len']
        assert int(out['wav_len'][b]) == want[1] - want[0]
        assert out['peak'][b] == np.abs(y[want[0]:want[1]]).max()
    # trim_silence returns the cut wav itself, numpy in -> numpy out and device in -> device out
    t = dsp.trim_silence(items[1])
    assert isinstance(t, np.ndarray) and t.tobytes() == items[1][slice(*R.TRIM_BOUNDS[1])].tobytes()
    td = dsp.trim_silence(torch.from_numpy(items[1]).cuda())
    assert td.is_cuda and td.cpu().numpy().tobytes() == t.tobytes()
    # all-zero input: every frame is at 0 dB of itself, nothing is cut; a click keeps its four frames
    z = np.zeros(5000, np.float32)
    click = np.zeros(10000, np.float32)
    click[5000] = 1.0
    o = _host(dsp.preprocess_batch([z, click]))
    assert (int(o['trim_start'][0]), int(o['trim_end'][0])) == (0, 5000) and int(o['mel_len'][0]) == 1 + 5000 // hop
    assert (int(o['trim_start'][1]), int(o['trim_end'][1])) == R.trim_bounds(click, 60) == (8 * 512, 12 * 512)


def test_scaled_wav_is_bit_equal_to_numpy_float32(items):
    out = _host(_dsp(peak_norm=True).preprocess_batch(items))
    cfg = dict(R.CFG, peak_norm=True)
    for b, y in enumerate(items):
        r = R.preprocess(y, cfg)
        n = len(r['wav'])
        assert out['peak'][b] == np.float32(r['peak'])
        assert out['wav'][b, :n].tobytes() == r['wav'].tobytes(), b
        assert not out['wav'][b, n:].any()
    # peak_norm off: an item above 1 is scaled, the others are passed through untouched
    loud = [items[0], items[1] * np.float32(3.0), items[2]]
    out = _host(_dsp().preprocess_batch(loud))
    for b, y in enumerate(loud):
        r = R.preprocess(y)
        n = len(r['wav'])
        assert (r['peak'] > 1.0) == (b == 1)
        assert out['wav'][b, :n].tobytes() == r['wav'].tobytes(), b
        if b != 1:
            assert out['wav'][b, :n].tobytes() == y[r['trim_start']:r['trim_end']].tobytes()


@pytest.mark.parametrize('peak_norm', [False, True])
def test_log_mel_within_the_fp32_route_margin(items, peak_norm):
    cfg = dict(R.CFG, peak_norm=peak_norm)
    dsp = _dsp(peak_norm=peak_norm)
    out = _host(dsp.preprocess_batch(items))
    for b, y in enumerate(items):
        r = R.preprocess(y, cfg)
        ml = r['mel_len']
        assert out['mel'][b, :, :ml].shape == r['mel'].shape
        _check_mel(f'item {b} peak_norm={peak_norm}', out['mel'][b, :, :ml], r['mel'], r['wav'], cfg)
        # linear domain, relative to the item's largest value
        lin_ref = R.wav_to_mel(r['wav'], cfg, normalize=False)
        lin = dsp.wav_to_mel(r['wav'], normalize=False)
        e_ref = np.abs(R.wav_to_mel_fp32(r['wav'], cfg, normalize=False) - lin_ref).max() / lin_ref.max()
        e_dev = np.abs(lin.astype(np.float64) - lin_ref).max() / lin_ref.max()
        print(f'item {b} peak_norm={peak_norm}: linear error {e_dev:.3e} of the maximum, fp32 CPU route {e_ref:.3e}, '
              f'ratio {e_dev / e_ref:.2f}')
        assert e_dev <= MARGIN * e_ref, (b, e_dev, e_ref)


def test_all_zero_item_under_peak_norm_is_nan_like_numpy(items):
    """0 / 0: the reference's `y /= peak` gives NaN for a silent file; so does the device, for that item only"""
    z = np.zeros(3000, np.float32)
    out = _host(_dsp(peak_norm=True).preprocess_batch([items[3], z]))
    with np.errstate(invalid='ignore'):
        r = R.preprocess(z, dict(R.CFG, peak_norm=True))
    assert np.isnan(r['wav']).all() and (r['trim_start'], r['trim_end']) == (0, 3000)
    assert (int(out['trim_start'][1]), int(out['trim_end'][1]), float(out['peak'][1])) == (0, 3000, 0.0)
    assert np.isnan(out['wav'][1, :3000]).all() and not out['wav'][1, 3000:].any()
    ml = int(out['mel_len'][1])
    assert ml == 1 + 3000 // 256 and np.isnan(out['mel'][1, :, :ml]).all() and (out['mel'][1, :, ml:] == PAD32).all()
    assert np.isfinite(out['mel'][0]).all() and np.isfinite(out['wav'][0]).all()
    quiet = _host(_dsp().preprocess_batch([z]))                     # peak_norm off: nothing is divided
    assert not quiet['wav'].any()                                   # every mel value is the clip's log, to the two logs' rounding
    assert np.abs(quiet['mel'][0] - np.log(1e-5)).max() <= 5 * float(np.spacing(np.float32(8)))


def test_item_alone_equals_item_in_batch_and_padding_is_exact(items, monkeypatch):
    from forwardtacotron_amd import audio
    monkeypatch.setattr(audio, '_empty', _poison)             # every buffer starts as NaN / junk
    dsp = _dsp(peak_norm=True)
    batch = _host(dsp.preprocess_batch(items))
    assert np.isfinite(batch['mel']).all() and np.isfinite(batch['wav']).all()
    for b, y in enumerate(items):
        one = _host(dsp.preprocess(y))
        ml, wl = int(one['mel_len'][0]), int(one['wav_len'][0])
        for k in ('mel_len', 'trim_start', 'trim_end', 'wav_len', 'peak'):
            assert one[k][0] == batch[k][b], (k, b)
        assert ml == R.preprocess(y)['mel_len'] and 0 < ml <= one['mel'].shape[2]
        assert one['mel'][0, :, :ml].tobytes() == batch['mel'][b, :, :ml].tobytes(), b
        assert one['wav'][0, :wl].tobytes() == batch['wav'][b, :wl].tobytes(), b
        for m in (one['mel'][0], batch['mel'][b]):
            assert m.dtype == np.float32 and (m[:, ml:] == PAD32).all() and (m[:, :ml] != PAD32).any()
    assert any(int(batch['mel_len'][b]) < batch['mel'].shape[2] for b in range(4))      # there is padding to check
    from forwardtacotron_amd.audio import split_items
    per_item = split_items(dsp.preprocess_batch(items))
    for b, it in enumerate(per_item):
        assert it['mel'].shape == (80, int(batch['mel_len'][b])) and it['wav'].shape == (int(batch['wav_len'][b]),)
        assert it['mel'].tobytes() == np.ascontiguousarray(batch['mel'][b, :, :it['mel_len']]).tobytes()


def test_wav_to_mel_forms(items):
    dsp = _dsp()
    y = items[2]
    T = 1 + len(y) // R.CFG['hop_length']
    # numpy in -> numpy out, device in -> device out, same bits; no trimming, no scaling
    m_np = dsp.wav_to_mel(y)
    m_dev = dsp.wav_to_mel(torch.from_numpy(y).cuda())
    assert isinstance(m_np, np.ndarray) and m_np.dtype == np.float32 and m_np.shape == (80, T)
    assert torch.is_tensor(m_dev) and m_dev.is_cuda and m_dev.cpu().numpy().tobytes() == m_np.tobytes()
    _check_mel('wav_to_mel', m_np, R.wav_to_mel(y), y, R.CFG)
    # normalize=False is the linear mel; normalize() of it is the log-mel
    lin = dsp.wav_to_mel(y, normalize=False)
    lin_ref = R.wav_to_mel(y, normalize=False)
    e_ref = np.abs(R.wav_to_mel_fp32(y, normalize=False) - lin_ref).max() / lin_ref.max()
    e_dev = np.abs(lin - lin_ref).max() / lin_ref.max()
    print(f'linear mel: error {e_dev:.3e} of the maximum, fp32 CPU route {e_ref:.3e}, ratio {e_dev / e_ref:.2f}')
    assert lin.shape == (80, T) and e_dev <= MARGIN * e_ref
    # numpy's log of the device's linear mel against the device's logf of the same fp32 value: the two differ by their
    # rounding only, at most 1 ulp (the device library's logf) + 4 ulp (numpy's vectorised float32 log), of values
    # in (-16, -8] for these signals, where an ulp is 9.5e-7
    assert np.abs(m_np).max() < 16
    np.testing.assert_allclose(dsp.normalize(lin), m_np, rtol=0, atol=5 * float(np.spacing(np.float32(8))))
    np.testing.assert_allclose(dsp.denormalize(dsp.normalize(lin)), np.maximum(lin, 1e-5), rtol=1e-6)
    # reflect padding (older librosa): edge frames differ from the zero-padded ones, all match the oracle
    refl = _dsp(pad_mode='reflect')
    m_r = refl.wav_to_mel(y)
    ref_r = R.wav_to_mel(y, pad_mode='reflect')
    _check_mel('reflect', m_r, ref_r, y, R.CFG, 'reflect')
    assert m_r[:, 2:-2].tobytes() == m_np[:, 2:-2].tobytes() and np.abs(m_r[:, 0] - m_np[:, 0]).max() > 1e-3
    out = _host(refl.preprocess_batch(items))
    for b, yb in enumerate(items):
        r = R.preprocess(yb, R.CFG, pad_mode='reflect')
        _check_mel(f'reflect item {b}', out['mel'][b, :, :r['mel_len']], r['mel'], r['wav'], R.CFG, 'reflect')
    from forwardtacotron_amd import _lib
    with pytest.raises(_lib.FtError, match='reflect'):
        refl.wav_to_mel(y[:512])


def test_odd_lengths_and_a_wav_shorter_than_a_hop():
    rng = np.random.default_rng(5)
    dsp = _dsp(trim_start_end_silence=False)
    wavs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (12345, 255, 777, 1, 256, 1023)]
    assert max(np.abs(y).max() for y in wavs) < 1.0                 # no item is scaled (peak_norm is off)
    out = _host(dsp.preprocess_batch(wavs))
    assert out['mel'].shape == (6, 80, 1 + 12345 // 256)
    for b, y in enumerate(wavs):
        ml = 1 + len(y) // 256
        assert int(out['mel_len'][b]) == ml and int(out['wav_len'][b]) == len(y)
        assert (int(out['trim_start'][b]), int(out['trim_end'][b])) == (0, len(y))
        assert out['wav'][b, :len(y)].tobytes() == y.tobytes() and not out['wav'][b, len(y):].any()
        assert (out['mel'][b, :, ml:] == PAD32).all()
        _check_mel(f'length {len(y)}', out['mel'][b, :, :ml], R.wav_to_mel(y), y, R.CFG)
        single = dsp.wav_to_mel(y)
        assert single.shape == (80, ml) and single.tobytes() == np.ascontiguousarray(out['mel'][b, :, :ml]).tobytes()
    assert dsp.wav_to_mel(wavs[1]).shape == (80, 1)
    trimmed = _host(_dsp().preprocess_batch(wavs))                 # white noise: every frame is loud, nothing is cut
    for b, y in enumerate(wavs):
        assert (int(trimmed['trim_start'][b]), int(trimmed['trim_end'][b])) == R.trim_bounds(y, 60) == (0, len(y))


def test_round_trip_through_griffinlim(items):
    dsp = _dsp()
    mel = dsp.wav_to_mel(torch.from_numpy(items[3]).cuda())
    wav = dsp.griffinlim(mel, n_iter=4, seed=0)
    assert wav.is_cuda and wav.shape == (R.CFG['hop_length'] * (mel.shape[1] - 1),)
    again = dsp.wav_to_mel(wav)
    assert again.shape == mel.shape and torch.isfinite(again).all() and torch.isfinite(wav).all()
    wav_np = dsp.griffinlim(mel.cpu().numpy(), n_iter=2, seed=0)
    assert isinstance(wav_np, np.ndarray) and wav_np.shape == tuple(wav.shape)
