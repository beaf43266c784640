"""GPU: the ragged-batch intake (forwardtacotron_amd/ragged.py) and the batch-independent GEMM (hip.linear_fwd_as) at
the edges of the intake, not of the workloads behind it: an empty item, a row stride that is and is not a multiple of 4,
lengths on the host and on the device, a device-side length one past the bound, and a GEMM row alone against the same
row inside a launch that crosses one 128-row tile.  Everything here is exact."""
import numpy as np
import pytest
import torch

from poison import poison

pytestmark = pytest.mark.gpu

LENS = [0, 5, 13]
SMALL = dict(num_mels=40, sample_rate=22050, hop_length=128, win_length=400, n_fft=512, fmin=0, fmax=8000)
_state = {}


@pytest.fixture(scope='module')
def dsp():
    from forwardtacotron_amd.audio import DSP
    if 'dsp' not in _state:
        _state['dsp'] = DSP(**SMALL)
    return _state['dsp']


def _wavs():
    rng = np.random.default_rng(7)
    return [rng.standard_normal(n).astype(np.float32) for n in LENS]


@pytest.mark.parametrize('row_multiple,ld', [(4, 16), (1, 13)])
def test_gather_wavs_numpy_and_device_items_give_the_same_bytes(row_multiple, ld):
    from forwardtacotron_amd import ragged
    host = _wavs()
    got = []
    for wavs in (host, [torch.from_numpy(y).cuda() for y in host]):
        wav, lens, Lmax = ragged.gather_wavs(wavs, torch.device('cuda'), 'test', row_multiple=row_multiple, alloc=poison)
        assert wav.is_cuda and wav.dtype == torch.float32 and tuple(wav.shape) == (3, ld) and Lmax == 13
        assert lens.is_cuda and lens.dtype == torch.int64 and lens.cpu().tolist() == LENS
        got.append(wav.cpu().numpy())
    assert got[0].tobytes() == got[1].tobytes()
    for b, y in enumerate(host):
        assert got[0][b, :LENS[b]].tobytes() == y.tobytes() and not got[0][b, LENS[b]:].any()      # the padding is zero


def test_device_lens_host_lengths_get_no_flag_and_device_lengths_a_zero_one():
    from forwardtacotron_amd import ragged
    dev = torch.device('cuda')
    lens, flag = ragged.device_lens(torch.tensor(LENS), 3, 0, 13, 'test', 'wav_len', 'L', dev)
    assert flag is None and lens.is_cuda and lens.cpu().tolist() == LENS
    given = torch.tensor(LENS).cuda()
    lens, flag = ragged.device_lens(given, 3, 0, 13, 'test', 'wav_len', 'L', dev)
    assert lens.data_ptr() == given.data_ptr()                                  # taken as it is
    assert flag.is_cuda and flag.dtype == torch.int32 and flag.cpu().tolist() == [0]
    ragged.LenFlag().check(flag, 'not raised')
    lens, flag = ragged.device_lens(given, 3, 0, 13, 'test', 'wav_len', 'L', dev, flag=False)
    assert flag is None and lens.data_ptr() == given.data_ptr()


def test_resample_batch_raises_a_device_length_past_the_bound_and_the_word_does_not_stick(dsp):
    from forwardtacotron_amd._lib import FtError
    pad = np.zeros((3, 13), dtype=np.float32)
    for b, y in enumerate(_wavs()):
        pad[b, :LENS[b]] = y
    dev = torch.from_numpy(pad).cuda()
    with pytest.raises(FtError) as e:                                           # up == down: the copy route
        dsp.resample_batch(dev, SMALL['sample_rate'], wav_len=torch.tensor([0, 5, 14]).cuda())
    assert str(e.value) == 'resample_batch: every wav_len must be in [0, L = 13]'
    out = dsp.resample_batch(dev, SMALL['sample_rate'], wav_len=torch.tensor(LENS).cuda())
    assert out['wav_len'].cpu().tolist() == LENS
    wav = out['wav'].cpu().numpy()
    assert wav.shape == (3, 16) and wav[:, :13].tobytes() == pad.tobytes() and not wav[:, 13:].any()


def test_griffinlim_batch_raises_a_device_length_past_the_bound_and_the_word_does_not_stick(dsp):
    from forwardtacotron_amd._lib import FtError
    mel = torch.from_numpy(np.random.default_rng(3).uniform(-8.0, 0.0, (3, SMALL['num_mels'], 3)).astype(np.float32)).cuda()
    with pytest.raises(FtError) as e:
        dsp.griffinlim_batch(mel, torch.tensor([1, 2, 4]).cuda(), n_iter=1, seed=5)
    assert str(e.value) == 'griffinlim_batch: every mel_len must be in [1, Tmax = 3]'
    out = dsp.griffinlim_batch(mel, torch.tensor([1, 2, 3]).cuda(), n_iter=1, seed=5)
    assert out['wav_len'].cpu().tolist() == [0, SMALL['hop_length'], 2 * SMALL['hop_length']]
    host = dsp.griffinlim_batch(mel, torch.tensor([1, 2, 3]), n_iter=1, seed=5)          # host lengths: the same bits
    assert torch.equal(out['wav'], host['wav']) and bool(torch.isfinite(out['wav']).all())


def test_linear_fwd_as_gives_a_row_alone_the_bits_it_has_inside_a_launch_over_two_tiles():
    from forwardtacotron_amd import hip as H
    in_f, ldx, out_f, rows = 64, 16, 24, 130                                    # overlapping rows, as the STFT reads them
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.standard_normal((rows - 1) * ldx + in_f).astype(np.float32)).cuda()
    w = torch.from_numpy(rng.standard_normal((out_f, in_f)).astype(np.float32)).cuda()
    y = H.linear_fwd_as(x, ldx, w, rows, in_f, alloc=poison)
    assert tuple(y.shape) == (rows, out_f) and bool(torch.isfinite(y).all())
    # the rows are the right ones: inside the a-priori bound of an fp32 sum of in_f products, (in_f + 2) 2^-24 sum |x| |w|
    fr, wd = x.cpu().double().unfold(0, in_f, ldx), w.cpu().double()           # [rows, in_f] overlapping frames
    worst = float(((y.cpu().double() - fr @ wd.T).abs() / ((in_f + 2) * 2.0 ** -24 * (fr.abs() @ wd.abs().T))).max())
    print(f'linear_fwd_as: worst error / bound {worst:.3f}')
    assert worst <= 1.0
    for r in (0, 1, 127, 128, 129):
        one = H.linear_fwd_as(x[r * ldx:], ldx, w, 1, in_f, alloc=poison)
        assert torch.equal(one[0], y[r]), r
