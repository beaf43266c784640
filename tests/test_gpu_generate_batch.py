"""GPU: ForwardTacotron.generate_batch -- every item of a ragged batch gets what generate() gives it alone -- and the
length-aware kernels under it (packed GRU, masked eval convolution, masked max-pool) on their own."""
import numpy as np
import pytest
import torch

import generate_batch_contract as contract
from helpers import TINY, load_npz, maxdiff, sub

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    """(fixture, model on the device, x, x_len, generate_batch of the zero-padded fixture batch) -- computed once"""
    from forwardtacotron_amd import hip, model
    G = load_npz('generate_batch.npz')
    m = model.ForwardTacotron(**TINY)
    m.load_state_dict(sub(G, 'sd/'))
    m = m.cuda()
    x = torch.from_numpy(G['x']).cuda()
    x_len = torch.from_numpy(G['x_len'])
    out = m.generate_batch(x, x_len, alpha=float(G['alpha']))
    torch.cuda.synchronize()
    hip.check_rnn_status()
    return G, m, x, x_len, {k: v.cpu() for k, v in out.items()}


def test_golden(fx):
    contract.check_golden(fx, TINY)


def test_pad_content_is_irrelevant(fx):
    contract.check_pad_content_is_irrelevant(fx, TINY)


def test_neighbours_are_irrelevant(fx):
    contract.check_neighbours_are_irrelevant(fx, TINY)


def test_existing_generate_differs_in_a_padded_batch(fx):
    """why the method exists: generate() on the same zero-padded batch runs the pad token's embedding through the
    convolutions and starts the reverse GRUs inside the padding, so a short item's own tokens come out differently"""
    contract.check_existing_generate_differs_in_a_padded_batch(fx, TINY)


def test_user_function_applies_per_token(fx):
    contract.check_user_function_applies_per_token(fx, TINY)


def test_bad_user_function_raises_and_nothing_sticks(fx):
    contract.check_bad_user_function_raises_and_nothing_sticks(fx, TINY)


def test_overlap_switch_is_bit_neutral(fx, monkeypatch):
    contract.check_overlap_switch_is_bit_neutral(fx, TINY, monkeypatch)


# ---- packed GRU alone ------------------------------------------------------------------------------------------
def _gru_case(Hh, lens, seed):
    """GRU input 12 wide; -> (GPU output per persistent mode {1, 0}, float64 torch.nn.GRU over the packed batch)"""
    from forwardtacotron_amd import _lib, hip, model
    B, T, I = len(lens), max(lens), 12
    torch.manual_seed(seed)
    ref = torch.nn.GRU(I, Hh, batch_first=True, bidirectional=True)
    if Hh > 128:        # keep the recurrence contractive (test_gpu_rnn.py: _params)
        with torch.no_grad():
            for n_, p in ref.named_parameters():
                if n_.startswith('weight_hh'):
                    p.copy_(torch.randn_like(p) * (1.6 / Hh ** 0.5))
    x = torch.randn(B, T, I)
    lt = torch.tensor(lens)
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(x.double(), lt, batch_first=True, enforce_sorted=False)
        yo, _ = torch.nn.utils.rnn.pad_packed_sequence(ref.double()(packed)[0], batch_first=True, total_length=T)
    ref = ref.float()
    m = model.GRU(I, Hh)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    res, counts = {}, {}
    for mode in (1, 0):
        old = _lib.lib().ft_rnn_set_persistent(mode)
        try:
            c0 = hip.rnn_counters()
            m0 = hip.rnn_mode_counts()
            with torch.no_grad():
                y = m.forward_lens(x.cuda(), lt.cuda())
            hip.check_rnn_status()
            c1, m1 = hip.rnn_counters(), hip.rnn_mode_counts()
            res[mode] = y.cpu()
            counts[mode] = (c1[0] - c0[0], c1[1] - c0[1], (m1[0] - m0[0]) + (m1[1] - m0[1]))
        finally:
            _lib.lib().ft_rnn_set_persistent(old)
    return res, counts, yo, lt


def _check_gru(res, yo, lt):
    T = yo.shape[1]
    beyond = torch.arange(T)[None, :] >= lt[:, None]
    for mode in (1, 0):
        assert bool((res[mode][beyond] == 0).all()), 'outputs at t >= L_b must be exactly 0'
        d = maxdiff(res[mode], yo)
        print(f'persistent={mode}: {d:.3e} off torch.nn.GRU over the packed batch')
        assert d < 2e-5
    assert maxdiff(res[1], res[0]) < 5e-6, 'persistent forward differs from the per-step kernels'


def test_packed_gru_per_step_kernels():
    res, counts, yo, lt = _gru_case(8, [9, 1, 5], 11)                       # H % 16 != 0: one launch per time step
    assert counts[1][:2] == (0, 0) and counts[0][:2] == (0, 0)
    _check_gru(res, yo, lt)


def test_packed_gru_persistent():
    res, counts, yo, lt = _gru_case(16, [9, 1, 5], 12)
    assert counts[1] == (1, 0, 2), 'one persistent launch, one 16-row group per direction'
    assert counts[0][:2] == (0, 0)
    _check_gru(res, yo, lt)


def test_packed_gru_256_eight_row_groups():
    lens = [40, 1, 17, 33, 8, 40, 25, 2, 31]                              # B = 9: the second 8-row group holds one item
    res, counts, yo, lt = _gru_case(256, lens, 13)
    assert counts[1] == (1, 0, 4), 'one persistent launch of 2 directions x 2 eight-row groups'
    _check_gru(res, yo, lt)


def test_packed_gru_batch_slices(monkeypatch):
    """B = 65 when the whole batch is refused one persistent grid: 64-row slices, each with its own part of `lens`.
    This small grid fits the chip, so the refusal is arranged: with 4 % of the admission budget the whole batch
    (2 x 5 groups -> 4 workgroups in the fullest XCD slot, 1/16 of an XCD) is over it and a slice (2, 1/32) is not."""
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(1, 7, (65,), generator=g).tolist()
    lens[0], lens[63], lens[64] = 6, 1, 3
    monkeypatch.setenv('FT_RNN_ADMIT_PCT', '4')
    res, counts, yo, lt = _gru_case(16, lens, 14)
    assert counts[1][:2] == (2, 1), 'expected one refusal of the whole batch and two persistent slice launches'
    _check_gru(res, yo, lt)


# ---- masked eval convolution and max-pool alone ------------------------------------------------------------------
# The eval convolution is a row GEMM over the B * T rows (b, t) of the batch in tiles of M_TILE rows (ft_gemm_rows_kernel:
# BM = 64 for launches this small), so with T = 37 tile boundaries fall at (item 1, t = 27) and (item 3, t = 17): item 1
# ends one row BEHIND its boundary (last valid row = first row of the next tile), item 3 right AT it.
M_TILE = 64
T_CONV = 37
LENS_CONV = [37, 28, 1, 17]
assert (1 * T_CONV + LENS_CONV[1] - 1) == M_TILE and (3 * T_CONV + LENS_CONV[3]) == 2 * M_TILE


@pytest.mark.parametrize('k', [3, 5, 4])
def test_masked_conv_alone(k):
    from forwardtacotron_amd import hip
    B, T, Cin, Cout = len(LENS_CONV), T_CONV, 6, 10
    g = torch.Generator().manual_seed(20 + k)
    lens = torch.tensor(LENS_CONV)
    x = torch.randn(B, T, Cin, generator=g) * (torch.arange(T)[None, :, None] < lens[:, None, None])
    w = torch.randn(Cout, Cin, k, generator=g) * 0.3
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    wp = hip.conv_pack_weight(w.cuda())
    y = hip.conv1d_fwd_lens(x.cuda(), wp, True, lens.cuda(), scale.cuda(), shift.cuda()).cpu()
    # float64 restatement: y[b,t,o] = scale[o] * relu(sum_{j,c} x[b, t + j - k//2, c] * w[o,c,j]) + shift[o], 0 at t >= L_b
    xp = np.zeros((B, T + 2 * k, Cin))
    xp[:, k:k + T] = x.double().numpy()
    acc, mag = np.zeros((B, T, Cout)), np.zeros((B, T, Cout))
    wn = w.double().numpy()
    for j in range(k):
        seg = xp[:, k + j - k // 2:k + j - k // 2 + T]
        acc += np.einsum('btc,oc->bto', seg, wn[:, :, j])
        mag += np.einsum('btc,oc->bto', np.abs(seg), np.abs(wn[:, :, j]))
    sc, sh = scale.double().numpy(), shift.double().numpy()
    want = np.maximum(acc, 0) * sc + sh
    valid = (np.arange(T)[None, :] < lens.numpy()[:, None])
    # fp32 accumulation of n = k * Cin products (any order) plus the affine: |err| <= (n + 3) * 2^-24 * (scale * sum|x w| + |shift|)
    tol = (k * Cin + 3) * 2.0 ** -24 * (mag * sc + np.abs(sh)) + 1e-30
    err = np.abs(y.double().numpy() - want)
    assert bool((err[valid] <= tol[valid]).all()), float((err / tol)[valid].max())
    assert bool((y.numpy()[~valid] == 0).all()), 'masked rows must be exactly 0'
    for b, L in enumerate(LENS_CONV):       # valid rows: the unmasked kernel on the item alone, bit for bit
        alone = hip.conv1d_fwd(x[b:b + 1, :L].contiguous().cuda(), wp, True, L, scale.cuda(), shift.cuda()).cpu()
        assert torch.equal(y[b, :L], alone[0]), b


@pytest.mark.parametrize('C', [8, 7])           # 16-B lanes | scalar form
def test_masked_maxpool_alone(C):
    from forwardtacotron_amd import hip
    B, T = len(LENS_CONV), T_CONV
    g = torch.Generator().manual_seed(30 + C)
    lens = torch.tensor(LENS_CONV)
    x = torch.randn(B, T, C, generator=g)          # NOT masked: the bank's own store is not, either
    y = hip.maxpool2_fwd_lens(x.cuda(), lens.cuda()).cpu()
    xn = x.double().numpy()
    want = xn.copy()
    want[:, 1:] = np.maximum(xn[:, 1:], xn[:, :-1])
    want[np.arange(T)[None, :] >= lens.numpy()[:, None]] = 0.0
    assert np.array_equal(y.double().numpy(), want)
    for b, L in enumerate(LENS_CONV):
        alone = hip.maxpool2_fwd(x[b:b + 1, :L].contiguous().cuda()).cpu()
        assert torch.equal(y[b, :L], alone[0]) and bool((y[b, L:] == 0).all()), b


# ---- production widths ------------------------------------------------------------------------------------------
def test_production_widths_vs_oracle_per_item():
    from forwardtacotron_amd import data, hip
    from forwardtacotron_amd.model import ForwardTacotron
    from oracle import ft_oracle as O
    cfg = dict(data.SINGLESPEAKER_MODEL)
    x_len = [40, 13, 1, 27, 40]
    alpha = 0.9
    torch.manual_seed(0)
    m = ForwardTacotron(**cfg)
    with torch.no_grad():                           # as tests/golden/make_golden_generate_batch.py
        m.dur_pred.lin.weight.mul_(30.0)
        m.dur_pred.lin.bias.fill_(2.5)
    P = {k: v.clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(0)            # (token seed picked on the CPU so that the margins below hold)
    x = torch.zeros(5, 40, dtype=torch.long)
    for b, L in enumerate(x_len):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    want = []
    for b, L in enumerate(x_len):
        xb = x[b:b + 1, :L].clone()
        with torch.no_grad():
            d = O.series_predictor(xb, P, 'dur_pred.', False, alpha).double().numpy()
        assert np.abs(d - np.round(d)).min() >= 1e-3 and np.abs((d - 0.5) - np.round(d - 0.5)).min() >= 1e-3, b
        want.append(O.generate(P, xb, cfg, alpha=alpha))
    m = m.cuda()
    out = {k: v.cpu() for k, v in m.generate_batch(x.cuda(), torch.tensor(x_len), alpha=alpha).items()}
    hip.check_rnn_status()
    assert out['mel_len'].tolist() == [w['mel'].shape[2] for w in want]
    for b, L in enumerate(x_len):
        n = want[b]['mel'].shape[2]
        for k, v in contract.valid(out, b, L, n).items():
            d = maxdiff(v, want[b][k])
            print(f'item {b} {k}: {d:.3e}')
            assert d < 1e-4, (b, k, d)
        assert bool((out['mel'][b, :, n:] == contract.PAD).all()) and bool((out['mel_post'][b, :, n:] == contract.PAD).all())
