"""CPU: the float64 restatement of the resampler (tests/resample_cpu.py) equals scipy.signal.resample_poly, the host
helpers of forwardtacotron_amd.audio (ratio, output length, filter, coefficient table) equal the restatement and the
hand values, a float32 sequential sum stays inside the a-priori bound the GPU test (tests/test_gpu_resample.py) holds
the kernel to, and the C ABI of the kernel is declared."""
import numpy as np
import pytest

import resample_cpu as R
from forwardtacotron_amd import _lib
from forwardtacotron_amd import audio as A


@pytest.mark.parametrize('case', list(R.CASES))
def test_restatement_equals_scipy_resample_poly(case):
    signal = pytest.importorskip('scipy.signal')
    up, down = R.ratio(*R.CASES[case])
    worst = 0.0
    for i, n in enumerate(R.LENGTHS):
        x = R.signal(n, 40 + i).astype(np.float64)
        y, _, _ = R.resample(x, up, down)
        ref = signal.resample_poly(x, up, down)
        assert y.shape == ref.shape == (R.out_len(n, up, down),)
        worst = max(worst, float(np.abs(y - ref).max()))
    print(f'{case} ({up}/{down}): max |restatement - scipy| = {worst:.2e}')
    assert worst <= 1e-12


def test_ratio_length_and_filter_equal_the_restatement_and_hand_values():
    assert A.resample_ratio(48000, 22050) == (147, 320)
    assert A.resample_ratio(22050, 22050) == (1, 1) and A.resample_ratio(7, 7) == (1, 1)
    assert A.resample_ratio(np.int64(44100), np.int32(22050)) == (1, 2)
    h, half = A.resample_filter(48000, 22050)
    assert half == 3200 and h.shape == (6401,) and h.dtype == np.float64
    assert abs(h.sum() - 147) <= 1e-12
    assert A.resample_len(1500, 48000, 22050) == 690
    assert A.resample_len(1, 44100, 22050) == 1
    assert A.resample_len(0, 48000, 22050) == 0
    for src, dst in list(R.CASES.values()) + [(22050, 22050), (48000, 16000), (8000, 48000)]:
        up, down = R.ratio(src, dst)
        assert A.resample_ratio(src, dst) == (up, down)
        hr, halfr = R.filt(up, down)
        h, half = A.resample_filter(src, dst)
        assert half == halfr == 10 * max(up, down)
        np.testing.assert_array_equal(h, hr)
        assert np.abs(h - h[::-1]).max() <= 1e-15                                 # symmetric: zero phase
        for n in (0, 1, 2, 7, 319, 320, 321, 1500, 2049, 1 << 33):
            assert A.resample_len(n, src, dst) == R.out_len(n, up, down) == -((-n * up) // down)


def test_bad_rates_and_ratios_raise():
    for bad in (0, -22050, 22050.0, '22050', None, True):
        with pytest.raises(_lib.FtError):
            A.resample_ratio(bad, 22050)
        with pytest.raises(_lib.FtError):
            A.resample_filter(22050, bad)
        with pytest.raises(_lib.FtError):
            A.resample_len(10, bad, 22050)
    assert A.resample_ratio(1024, 1) == (1, 1024) and A.resample_ratio(3, 1024) == (1024, 3)
    for src, dst in ((1025, 1), (1, 1025), (22050, 22051), (48000, 22049)):
        with pytest.raises(_lib.FtError, match='1024'):
            A.resample_ratio(src, dst)
    with pytest.raises(_lib.FtError):
        A.resample_len(-1, 48000, 22050)


def test_coefficient_table_is_the_filter_phase_major():
    for up, down in ((147, 320), (1, 2), (441, 320), (160, 441), (2, 1), (1, 1000)):
        h, half = R.filt(up, down)
        tab = A.resample_table(h, half, up)
        T = -(-(2 * half + 1) // up)
        assert tab.dtype == np.float32 and tab.shape == (up, T | 1)
        back = np.zeros(up * T, dtype=np.float32)
        back[:2 * half + 1] = h.astype(np.float32)
        np.testing.assert_array_equal(tab[:, :T], back.reshape(T, up).T)          # tab[p, t] = h[p + t up], 0 past the end
        assert not tab[:, T:].any()


@pytest.mark.parametrize('case', list(R.CASES))
def test_float32_sequential_sum_stays_inside_the_a_priori_bound(case):
    """pins the bound itself: numpy float32, h rounded once, every product and partial sum rounded, ascending k"""
    up, down = R.ratio(*R.CASES[case])
    worst = 0.0
    for i, n in enumerate(R.LENGTHS):
        x = R.signal(n, 60 + i)
        y64, S, T_n = R.resample(x, up, down)
        y32, _, _ = R.resample(x, up, down, np.float32)
        assert y32.dtype == np.float32 and (S > 0).all() and (T_n >= 1).all()
        worst = max(worst, float((np.abs(y32.astype(np.float64) - y64) / R.bound(S, T_n)).max()))
    print(f'{case} ({up}/{down}): worst |fp32 - fp64| / bound = {worst:.3f}')
    assert worst <= 1.0


def test_identity_and_empty_input():
    x = R.signal(33, 1)
    y, _, _ = R.resample(x, 1, 1)
    np.testing.assert_array_equal(y, x.astype(np.float64))
    y, S, T_n = R.resample(np.zeros(0, np.float32), 147, 320)
    assert y.shape == S.shape == T_n.shape == (0,)


def test_the_kernel_is_declared_in_the_abi():
    protos = _lib.parse_header()
    for name in ('ft_resample_poly_ragged', 'ft_resample_route', 'ft_resample_table_floats', 'ft_resample_tile'):
        assert name in protos
    args = [n for _, n in protos['ft_resample_poly_ragged'][1]]
    assert args == ['x', 'ldx', 'len', 'B', 'Lmax', 'tab', 'up', 'down', 'half', 'y', 'ldy', 'out_len', 'err_flag',
                    'stream']
