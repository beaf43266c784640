"""GPU: sample-rate conversion of a ragged batch (audio.DSP.resample_batch, ft_resample_poly_ragged of
csrc/ft_resample.hip) against the float64 restatement (tests/resample_cpu.py, itself held to scipy.signal.resample_poly
by tests/test_resample_cpu.py), and against itself: an item's samples are bit-identical alone and inside any batch, and
NaN padding, a NaN or Inf item or NaN-poisoned buffers change no bit of any item.

Ratios up/down: 147/320 (48 kHz -> 22.05 kHz), 1/2, 441/320 (upsampling), 160/441, 2/1 and the identity -- the kernel's
LDS route -- and 147/640 (48 kHz -> 11.025 kHz) and 1/64, which the kernel serves on its second route (operands read
through the cache: table and input window do not fit the LDS budget); ft_resample_route says which, and is asserted.

Lengths [0, 1, 2, 7, 319, 320, 321, 1500, 2049] -- empty, head and tail inside one filter, a window shorter than the
filter -- and per ratio the three input lengths that give 1023, 1024 and 1025 outputs: a tile is 1024 consecutive outputs
of one item, owned by one workgroup, so every ratio also has items of more than one tile and a last tile that is one
output long.  One test has 2,300 items: more workgroups than the chip holds at once (at most 8 per CU, 2,048).

Accuracy is the a-priori bound of one rounding of h, the products and a sequential fp32 sum, per sample:
|y_gpu - y_64| <= (T_n + 2) 2^-24 sum_k |h| |x[k]| (resample_cpu.bound); not a measured tolerance.  Every comparison
prints its worst ratio to the bound before it asserts.  Everything else is exact."""
import numpy as np
import pytest
import torch

import resample_cpu as R
from poison import poison as _poison

pytestmark = pytest.mark.gpu

SETTING = dict(num_mels=80, sample_rate=22050, hop_length=256, win_length=1024, n_fft=1024, fmin=0, fmax=8000)
RATIOS = {'147/320': (147, 320), '1/2': (1, 2), '441/320': (441, 320), '160/441': (160, 441), '2/1': (2, 1),
          'identity': (1, 1), '147/640': (147, 640), '1/64': (1, 64)}
ROUTE = {'147/320': 1, '1/2': 1, '441/320': 1, '160/441': 1, '2/1': 1, 'identity': 2, '147/640': 0, '1/64': 0}


def tile(up):
    """outputs per workgroup (include/fwdtaco_hip.h: ft_resample_tile; asserted against the library in the first test)"""
    return 1024


def _tile_lengths(up, down):
    """the smallest input lengths that give at least tile - 1, tile and tile + 1 outputs (exactly that many wherever the
    ratio can: 2/1 gives even counts only)"""
    return [((t - 1) * down) // up + 1 for t in (tile(up) - 1, tile(up), tile(up) + 1)]


def _batches(up, down):
    a, b, c = _tile_lengths(up, down)
    return [[319, 0, 2049, 1, 320], [2, 321, 7, 1500, b], [a, c, 1, 2049, 0]]


_items, _refs, _state = {}, {}, {}


def item(n):
    if n not in _items:
        _items[n] = R.signal(n, 1000 + n)
    return _items[n]


def ref(up, down, n):
    """(y64, S, T_n) of item(n), computed once and shared"""
    key = (up, down, n)
    if key not in _refs:
        _refs[key] = R.resample(item(n), up, down)
    return _refs[key]


@pytest.fixture(scope='module')
def dsp():
    from forwardtacotron_amd.audio import DSP
    if 'dsp' not in _state:
        _state['dsp'] = DSP(**SETTING)
    return _state['dsp']


@pytest.fixture(scope='module', params=list(RATIOS))
def ratio(request):
    return (request.param,) + RATIOS[request.param]


def run(dsp, lens, up, down):
    """resample_batch of the items of these lengths -> (wav [B, ld] numpy, wav_len list)"""
    out = dsp.resample_batch([item(n) for n in lens], down, up)
    return out['wav'].cpu().numpy(), out['wav_len'].cpu().tolist()


def worst_ratio(y, y64, S, T_n):
    """max |y - y64| / bound over the samples; asserts that a sample whose bound is 0 is exact"""
    err, bnd = np.abs(y.astype(np.float64) - y64), R.bound(S, T_n)
    assert (err[bnd == 0] == 0).all()
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


# ---- 1. the float64 restatement, lengths, padding ----------------------------------------------------------------
def test_matches_the_float64_restatement_within_the_a_priori_bound(dsp, ratio):
    from forwardtacotron_amd import _lib
    name, up, down = ratio
    assert _lib.query('ft_resample_route', up, down, 10 * max(up, down)) == ROUTE[name]
    assert _lib.query('ft_resample_tile', up, down, 10 * max(up, down)) == tile(up)
    worst = 0.0
    for lens in _batches(up, down):
        wav, wav_len = run(dsp, lens, up, down)
        assert wav.dtype == np.float32 and wav.shape[0] == len(lens) and wav.shape[1] % 4 == 0
        assert wav.shape[1] >= R.out_len(max(lens), up, down)
        for b, n in enumerate(lens):
            n_out = R.out_len(n, up, down)
            assert wav_len[b] == n_out                              # ceil(len * up / down), exactly
            assert not wav[b, n_out:].any()                         # exactly 0.0 past it (an empty item: the whole row)
            if n_out:
                y64, S, T_n = ref(up, down, n)
                r = worst_ratio(wav[b, :n_out], y64, S, T_n)
                worst = max(worst, r)
                assert r <= 1.0, (name, n, r)
    print(f'resample {name}: worst |gpu - fp64| / bound = {worst:.3f}')


# ---- 2. batch composition ----------------------------------------------------------------------------------------
def test_an_item_gives_the_same_bits_alone_and_at_every_position_of_a_batch(dsp, ratio):
    name, up, down = ratio
    for lens in _batches(up, down):
        alone = {}
        for n in set(lens) - {0}:
            wav, wav_len = run(dsp, [n], up, down)                  # B = 1, Lmax = its own length
            alone[n] = wav[0, :wav_len[0]]
        for shift in range(len(lens)):                              # every item visits position 0, the middle and the last
            order = lens[shift:] + lens[:shift]
            if max(order) == 0:
                continue
            wav, wav_len = run(dsp, order, up, down)
            for b, n in enumerate(order):
                if n:
                    np.testing.assert_array_equal(wav[b, :wav_len[b]], alone[n], err_msg=f'{name} len {n} at {b}')
                else:
                    assert wav_len[b] == 0 and not wav[b].any()


def test_more_tiles_than_resident_workgroups_give_the_same_bits(dsp, ratio):
    """the chip holds at most 8 workgroups per CU (2,048) at once: with 2,300 items (2,300 .. 11,500 tiles) the grid is
    dispatched in several waves, and every item still equals the item alone"""
    name, up, down = ratio
    cycle = [7, 321, 1, 2049, 0, 319, 2]
    lens = [cycle[i % len(cycle)] for i in range(2300)]
    wav, wav_len = run(dsp, lens, up, down)
    wav_len = np.asarray(wav_len)
    for n in cycle:
        rows = wav[np.asarray(lens) == n]
        n_out = R.out_len(n, up, down)
        assert (wav_len[np.asarray(lens) == n] == n_out).all()
        if n:
            alone, alone_len = run(dsp, [n], up, down)
            assert alone_len == [n_out]
            assert (rows[:, :n_out].view(np.uint32) == alone[0, :n_out].view(np.uint32)[None, :]).all(), (name, n)
        assert not rows[:, n_out:].any()


# ---- 3. nothing leaks --------------------------------------------------------------------------------------------
def test_nan_padding_nan_and_inf_items_and_poisoned_buffers_change_no_bit(dsp, ratio, monkeypatch):
    from forwardtacotron_amd import audio
    name, up, down = ratio
    lens = _batches(up, down)[2]                                    # tile - 1, tile + 1, 1, 2049, 0
    clean, clean_len = run(dsp, lens, up, down)
    L = max(lens)
    # (a) the padded form with NaN beyond every length, lengths on the device
    pad = np.full((len(lens), L), np.nan, dtype=np.float32)
    for b, n in enumerate(lens):
        pad[b, :n] = item(n)
    out = dsp.resample_batch(torch.from_numpy(pad).cuda(), down, up, wav_len=torch.tensor(lens).cuda())
    np.testing.assert_array_equal(out['wav'].cpu().numpy(), clean)
    assert out['wav_len'].cpu().tolist() == clean_len
    # (b) a NaN item and an Inf item beside the others
    for bad in (np.nan, np.inf):
        wavs = [item(n) for n in lens]
        wavs[3] = np.full(lens[3], bad, dtype=np.float32)
        got = dsp.resample_batch(wavs, down, up)
        wav = got['wav'].cpu().numpy()
        assert got['wav_len'].cpu().tolist() == clean_len
        for b in (0, 1, 2, 4):
            np.testing.assert_array_equal(wav[b], clean[b])
        assert not wav[3, clean_len[3]:].any()                      # its own padding is still exactly zero
        assert not np.isfinite(wav[3, :clean_len[3]]).all()
    # (c) every buffer of the path starts as NaN / garbage
    monkeypatch.setattr(audio, '_empty', _poison)
    dsp._rs_tabs.clear()                                            # the coefficient table is allocated again, poisoned
    wav, wav_len = run(dsp, lens, up, down)
    np.testing.assert_array_equal(wav, clean)
    assert wav_len == clean_len


# ---- 4. identity -------------------------------------------------------------------------------------------------
def test_identity_returns_the_input_bits(dsp):
    lens = [1023, 0, 1025, 7, 1024]
    for src in (22050, 48000):
        out = dsp.resample_batch([item(n) for n in lens], src, src)
        wav = out['wav'].cpu().numpy()
        assert out['wav_len'].cpu().tolist() == lens
        for b, n in enumerate(lens):
            np.testing.assert_array_equal(wav[b, :n].view(np.uint32), item(n).view(np.uint32))
            assert not wav[b, n:].any()
    y = dsp.resample(item(321), 22050)                              # target_sr defaults to the DSP's rate
    assert isinstance(y, np.ndarray)
    np.testing.assert_array_equal(y, item(321))


# ---- 5. the two input forms, argument errors ------------------------------------------------------------------------
def test_list_form_padded_form_and_single_wav_agree_and_bad_lengths_raise(dsp):
    from forwardtacotron_amd import _lib
    up, down = 147, 320
    lens = [321, 0, 2049, 7, 1500]
    clean, clean_len = run(dsp, lens, up, down)
    L = max(lens)                                                   # 2049: not a multiple of 4, the rows are re-laid
    pad = np.zeros((len(lens), L), dtype=np.float32)
    for b, n in enumerate(lens):
        pad[b, :n] = item(n)
    dev = torch.from_numpy(pad).cuda()
    for wl in (torch.tensor(lens), torch.tensor(lens).cuda()):      # host-side and device-side lengths
        out = dsp.resample_batch(dev, 48000, wav_len=wl)             # target_sr defaults to 22050
        assert out['wav'].is_cuda and out['wav_len'].is_cuda and out['wav_len'].dtype == torch.int64
        np.testing.assert_array_equal(out['wav'].cpu().numpy(), clean)
        assert out['wav_len'].cpu().tolist() == clean_len
    out = dsp.resample_batch([torch.from_numpy(item(n)).cuda() for n in lens], 48000)      # a list of device tensors
    np.testing.assert_array_equal(out['wav'].cpu().numpy(), clean)
    y = dsp.resample(torch.from_numpy(item(1500)).cuda(), 48000)
    assert y.is_cuda and y.shape == (clean_len[4],)
    np.testing.assert_array_equal(y.cpu().numpy(), clean[4, :clean_len[4]])
    y = dsp.resample(item(1500), 48000, 22050)
    np.testing.assert_array_equal(y, clean[4, :clean_len[4]])
    assert dsp.resample(np.zeros(0, np.float32), 48000).shape == (0,)
    # a device-side length out of range: raised at the end of the call, nothing faults
    for bad in ([321, 0, L + 1, 7, 1500], [321, -1, 2049, 7, 1500]):
        with pytest.raises(_lib.FtError, match='wav_len'):
            dsp.resample_batch(dev, 48000, wav_len=torch.tensor(bad).cuda())
        with pytest.raises(_lib.FtError, match='wav_len'):
            dsp.resample_batch(dev, 48000, wav_len=torch.tensor(bad))
    torch.cuda.synchronize()
    out = dsp.resample_batch(dev, 48000, wav_len=torch.tensor(lens).cuda())     # and the object still works
    np.testing.assert_array_equal(out['wav'].cpu().numpy(), clean)
    with pytest.raises(_lib.FtError):
        dsp.resample_batch(dev, 48000)                              # a padded batch without its lengths
    with pytest.raises(_lib.FtError):
        dsp.resample_batch(dev, 48000, wav_len=torch.tensor(lens[:-1]))
    with pytest.raises(_lib.FtError):
        dsp.resample_batch(dev, 48000, wav_len=torch.tensor(lens, dtype=torch.int32))
    with pytest.raises(_lib.FtError):
        dsp.resample_batch([item(7)], 48000, 22049)                 # 48000/22049: no ratio within 1024
    with pytest.raises(_lib.FtError):
        dsp.resample_batch([item(7)], 48000.0)
    with pytest.raises(_lib.FtError):
        dsp.resample_batch([], 48000)


# ---- 6. in front of the audio front end -------------------------------------------------------------------------
def test_preprocess_batch_with_a_source_rate_is_resample_then_preprocess(dsp):
    lens = [9000, 20000, 13001]
    wavs = [item(n) for n in lens]
    wavs[1] = np.concatenate([np.zeros(3000, np.float32), wavs[1], np.zeros(2500, np.float32)])     # silence to trim
    got = dsp.preprocess_batch(wavs, source_sr=48000)
    rs = dsp.resample_batch(wavs, 48000)
    rs_len = rs['wav_len'].cpu().tolist()
    assert rs_len == [R.out_len(len(w), 147, 320) for w in wavs]
    items = [rs['wav'][b, :rs_len[b]].cpu().numpy() for b in range(len(wavs))]
    want = dsp.preprocess_batch(items)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k
    assert int(got['trim_start'][1]) > 0                            # indices into the RESAMPLED signal
    assert int(got['trim_end'][1]) <= rs_len[1] < len(wavs[1])
    one = dsp.preprocess(wavs[0], source_sr=48000)
    assert torch.equal(one['mel'][0], dsp.preprocess_batch(items[:1])['mel'][0])
    # without a source rate, or at the DSP's own rate: today's call, bit for bit
    today = dsp.preprocess_batch(wavs)
    for sr in (None, dsp.sample_rate):
        same = dsp.preprocess_batch(wavs, source_sr=sr)
        for k in today:
            assert torch.equal(same[k], today[k]), (sr, k)


def test_preprocess_batch_issues_todays_calls_without_a_source_rate_and_one_more_with_it(dsp, monkeypatch):
    """every launch goes through _lib.call (as tools/call_trace.py relies on): the entries, in order"""
    from forwardtacotron_amd import _lib
    names, real = [], _lib.call

    def rec(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, 'call', rec)
    front_end = ['ft_wav_trim_peak', 'ft_wav_pack', 'ft_linear_multi_fwd_as', 'ft_mel_project']      # five launches
    wavs = [item(2049), item(1500)]
    for kw in ({}, {'source_sr': None}, {'source_sr': dsp.sample_rate}):
        del names[:]
        dsp.preprocess_batch(wavs, **kw)
        assert names == front_end, kw
    del names[:]
    dsp.preprocess_batch(wavs, source_sr=48000)
    assert names == ['ft_resample_poly_ragged'] + front_end


# ---- 7. behind the vocoder ---------------------------------------------------------------------------------------
def test_round_trip_from_griffinlim_batch(dsp):
    rng = np.random.default_rng(7)
    mel_len = [9, 5]
    mel = torch.from_numpy(rng.uniform(-8.0, 0.0, (2, SETTING['num_mels'], max(mel_len))).astype(np.float32)).cuda()
    gl = dsp.griffinlim_batch(mel, torch.tensor(mel_len).cuda(), n_iter=2, seed=5 << 40)
    out = dsp.resample_batch(gl['wav'], 22050, 16000, wav_len=gl['wav_len'])
    src_len = gl['wav_len'].cpu().tolist()
    assert src_len == [SETTING['hop_length'] * (n - 1) for n in mel_len]
    up, down = R.ratio(22050, 16000)
    assert out['wav_len'].cpu().tolist() == [R.out_len(n, up, down) for n in src_len]
    wav, src = out['wav'].cpu().numpy(), gl['wav'].cpu().numpy()
    worst = 0.0
    for b, n in enumerate(src_len):
        n_out = R.out_len(n, up, down)
        y64, S, T_n = R.resample(src[b, :n], up, down)
        worst = max(worst, worst_ratio(wav[b, :n_out], y64, S, T_n))
        assert not wav[b, n_out:].any()
    print(f'round trip 22050 -> 16000 behind griffinlim_batch: worst |gpu - fp64| / bound = {worst:.3f}')
    assert worst <= 1.0
