"""No device: the host side of the batched Griffin-Lim (forwardtacotron_amd/vocoder.py) -- the geometry of the packed
ragged batch, and the window-sum rule ft_overlap_add_ragged divides by, against the float64 oracle."""
import numpy as np
import pytest

from forwardtacotron_amd import _lib
from forwardtacotron_amd.vocoder import gl_batch_geometry, window_sumsquare_f32

TINY32 = float(np.finfo(np.float32).tiny)


@pytest.mark.parametrize('n_fft,hop', [(1024, 256), (512, 128), (1024, 200), (2048, 512), (16, 16), (1024, 1024), (24, 4)])
def test_geometry_holds_every_item_and_keeps_the_last_read_in_bounds(n_fft, hop):
    for B in (1, 2, 7, 32):
        for Tmax in (1, 2, 3, 4, 5, 9, 64, 127, 128, 129, 841):
            g = gl_batch_geometry(B, Tmax, n_fft, hop)
            Tcap = g['Tcap']
            assert Tcap >= Tmax - 1 + n_fft / hop and Tcap < Tmax + n_fft / hop        # holds it, and no row more
            assert g['stride'] == Tcap * hop >= n_fft + hop * (Tmax - 1)                # the longest padded signal fits
            assert g['rows'] == B * Tcap and g['wav_ld'] == hop * (Tmax - 1)
            assert g['packed'] == B * g['stride'] + n_fft                               # the n_fft zero tail
            # the one STFT GEMM reads n_fft samples from every row's offset row * hop: the last row ends inside
            assert g['last_read_end'] == (g['rows'] - 1) * hop + n_fft <= g['packed']
            # an item's own frames never leave its stride
            assert (Tmax - 1) * hop + n_fft <= g['stride']


def test_geometry_refuses_nonsense():
    for args in ((0, 4, 1024, 256), (2, 0, 1024, 256), (2, 4, 256, 1024), (2, 4, 1024, 0)):
        with pytest.raises(_lib.FtError):
            gl_batch_geometry(*args)


@pytest.mark.parametrize('n_fft,hop,win', [(1024, 256, 1024), (512, 128, 400), (1024, 200, 800)])
def test_window_sum_rule_matches_the_oracle_for_every_short_and_long_item(n_fft, hop, win):
    """fp32 accumulation of at most ceil(n_fft / hop) positive fp32-rounded terms plus the rounding of the reciprocal:
    (2 + ceil(n_fft / hop)) * 2^-24 <= 10 * 6e-8 < 1e-6 relative for n_fft / hop <= 8.  Where the oracle leaves a sample
    undivided (sum <= FLT_MIN) the rule must say so too: the window is exactly zero there or far above FLT_MIN."""
    from oracle import gl_oracle as G
    w2 = (G.hann_padded(win, n_fft) ** 2).astype(np.float32)
    R = -(-n_fft // hop)
    for N in range(1, 2 * R + 2):
        want = G.window_sumsquare(N, n_fft, hop, win)
        got = window_sumsquare_f32(w2, N, n_fft, hop)
        assert got.dtype == np.float32 and got.shape == want.shape == (n_fft + hop * (N - 1),)
        nz = want > TINY32
        assert np.array_equal(got > np.float32(TINY32), nz), N
        inv = np.float32(1.0) / got[nz]                                     # what the kernel multiplies by
        assert inv.dtype == np.float32
        rel = np.abs(inv.astype(np.float64) * want[nz] - 1.0).max()
        assert rel < 1e-6, (N, rel)


def test_the_ragged_entries_are_declared_and_exported():
    protos = _lib.parse_header()
    for name in ('ft_gl_exp_transpose_ragged', 'ft_gl_relu', 'ft_gl_init_ragged', 'ft_gl_phase_ragged',
                 'ft_overlap_add_ragged'):
        assert name in protos and hasattr(_lib.lib(), name), name
    assert [t for t, _ in protos['ft_gl_init_ragged'][1]][1] == 'uint64_t'
