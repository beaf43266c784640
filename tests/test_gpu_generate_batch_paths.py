"""GPU: the forms of the length-aware kernels that ForwardTacotron.generate_batch reaches only at large or long-form
batches -- the row mask in the 128-row bf16-split GEMM epilogue (ft_gemm_b3.hip: rows_b3_epilogue's `keep` bits), its
one-plane bf16 form, the packed GRU with its input projection in time chunks (ft_gru_layer_fwd_lens) -- and the
embedding that does not read the ids in the padding (ft_embedding_fwd_lens).  Each test proves the path it took."""
import math

import numpy as np
import pytest
import torch

from helpers import TINY, load_npz, maxdiff, sub

pytestmark = pytest.mark.gpu


# ---- masked eval convolution: 128-row tiles ------------------------------------------------------------------------
# The launcher takes 128 x 128 tiles from 192 of them on (gemm_plan::tiles_big): Cout = 256 is 2 column tiles, so
# B * T >= 96 * 128 = 12288 rows.  B * T = 5 * 2480 = 12400 -> 97 row tiles, the last one ragged (112 rows).  Rows are
# (b, t) = (row // T, row % T); M_TILE-row tile boundaries against the items' ends:
#   item 0 ends ONE ROW BEHIND a boundary (last valid row 640 = first row of tile 5),
#   item 1 ends AT a boundary (first masked row 2480 + 720 = 3200 = 25 * 128),
#   item 2 has one valid row, item 3 is full, item 4 ends inside a tile and inside the second 32-row block of a wave
#   (9920 + 1337 = 87 * 128 + 121); tiles wholly in the padding lie behind items 0, 1, 2 and 4.
M_TILE = 128
T_BIG, CIN, COUT = 2480, 8, 256
LENS_BIG = [641, 720, 1, 2480, 1337]
assert len(LENS_BIG) * T_BIG >= 12288 and (LENS_BIG[0] - 1) % M_TILE == 0 and (T_BIG + LENS_BIG[1]) % M_TILE == 0
assert (4 * T_BIG + LENS_BIG[4]) % M_TILE == 121

# the same edges against the 64-row tiles of a small launch (test_gpu_generate_batch.py: LENS_CONV)
T_SMALL, LENS_SMALL = 37, [37, 28, 1, 17]
assert (T_SMALL + LENS_SMALL[1] - 1) == 64 and (3 * T_SMALL + LENS_SMALL[3]) == 128


def _conv_case(T, lens, Cin, Cout, k, accumulate, precision, seed):
    """-> (masked launch, unmasked launch of the same batch, residual or None, float64 restatement, its error bound,
    valid-row mask [B,T], {GEMM variant: launches of the masked call})"""
    from forwardtacotron_amd import hip
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    lt = torch.tensor(lens)
    x = torch.randn(B, T, Cin, generator=g) * (torch.arange(T)[None, :, None] < lt[:, None, None])
    w = torch.randn(Cout, Cin, k, generator=g) * 0.3
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g)
    y0 = torch.randn(B, T, Cout, generator=g) if accumulate else None       # (conv_project2: the residual, non-zero everywhere)
    wp = hip.conv_pack_weight(w.cuda())
    with hip.gemm_precision(precision):
        c0 = hip.gemm_variant_counts()
        y = hip.conv1d_fwd_lens(x.cuda(), wp, True, lt.cuda(), scale.cuda(), shift.cuda(),
                                accumulate_into=y0.cuda() if accumulate else None).cpu()
        c1 = hip.gemm_variant_counts()
        plain = hip.conv1d_fwd(x.cuda(), wp, True, T, scale.cuda(), shift.cuda(),
                               accumulate_into=y0.cuda() if accumulate else None).cpu()
        c2 = hip.gemm_variant_counts()
    took = {v: c1[v] - c0[v] for v in c1 if c1[v] != c0[v]}
    assert took == {v: c2[v] - c1[v] for v in c2 if c2[v] != c1[v]}, 'the unmasked launch took another kernel'
    # float64 restatement: y[b,t,o] = scale[o] * relu(sum_{j,c} x[b, t + j - k//2, c] * w[o,c,j]) + shift[o] (+ y0), 0 at
    # t >= L_b.  bf16 mode rounds both operands to the nearest bf16 first (their products are then exact in fp32).
    if precision == 'bf16':
        x, w = x.bfloat16().float(), w.bfloat16().float()
    xp = np.zeros((B, T + 2 * k, Cin))
    xp[:, k:k + T] = x.double().numpy()
    wn = w.double().numpy()
    acc, mag = np.zeros((B, T, Cout)), np.zeros((B, T, Cout))
    for j in range(k):
        seg = xp[:, k + j - k // 2:k + j - k // 2 + T]
        acc += np.einsum('btc,oc->bto', seg, wn[:, :, j])
        mag += np.einsum('btc,oc->bto', np.abs(seg), np.abs(wn[:, :, j]))
    sc, sh = scale.double().numpy(), shift.double().numpy()
    want = np.maximum(acc, 0) * sc + sh
    base = mag * sc + np.abs(sh)
    # Error bound, from the formats.  The accumulator is fp32 and takes at most one rounding per MFMA input product:
    # 16 per v_mfma_f32_32x32x16_bf16, one MFMA per 16 k (K padded up) and tap in bf16 mode, six (the six kept terms of
    # the three-way operand split) in fp32 mode, where the three dropped terms add <= 2^-23 |x||w| per product
    # (ft_gemm_b3.hip, head of file); + 3 roundings for the affine epilogue, + 1 for the residual.
    R = (1 if precision == 'bf16' else 6) * 16 * k * math.ceil(Cin / 16) + 3
    tol = R * 2.0 ** -24 * base + (0.0 if precision == 'bf16' else 2.0 ** -23) * mag * sc + 1e-30
    if accumulate:
        want = want + y0.double().numpy()
        tol = tol + 2.0 ** -24 * (base + np.abs(y0.double().numpy()))
    valid = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    return y, plain, y0, want, tol, valid, took


def _check_conv(y, plain, want, tol, valid):
    err = np.abs(y.double().numpy() - want)
    ratio = float((err / tol)[valid].max())
    print(f'worst error / bound over the valid rows: {ratio:.3f}')
    assert ratio <= 1.0
    assert bool((y.numpy()[~valid] == 0).all()), 'masked rows must be exactly 0'
    v = torch.from_numpy(valid)
    assert torch.equal(y[v], plain[v]), 'valid rows must be bit-equal to the unmasked launch'
    assert bool((plain.numpy()[~valid] != 0).any()), 'the unmasked launch leaves the padding non-zero: the mask has work'


@pytest.mark.parametrize('k,accumulate,precision', [(3, False, 'fp32'), (5, True, 'fp32'), (3, False, 'bf16')])
def test_masked_conv_128_row_tiles(k, accumulate, precision):
    """rows_b3_epilogue<2, 2>: two accumulator row blocks per lane, 32 keep bits; fp32-exact and one-plane bf16 operands"""
    y, plain, y0, want, tol, valid, took = _conv_case(T_BIG, LENS_BIG, CIN, COUT, k, accumulate, precision, 40 + k)
    assert took == {'rows_b3p': 1}, took
    _check_conv(y, plain, want, tol, valid)


@pytest.mark.parametrize('k,accumulate', [(3, False), (4, True)])
def test_masked_conv_bf16_64_row_tiles(k, accumulate):
    """bf16 mode sends a launch this small to ft_gemm_rows_b3_kernel<1, 1, 1>: rows_b3_epilogue<1, 1>, 16 keep bits"""
    y, plain, y0, want, tol, valid, took = _conv_case(T_SMALL, LENS_SMALL, CIN, 10, k, accumulate, 'bf16', 50 + k)
    assert took == {'rows_b3_64': 1}, took
    _check_conv(y, plain, want, tol, valid)


# ---- packed GRU, input projection in time chunks beside the recurrence ---------------------------------------------
def test_packed_gru_chunked_projection(monkeypatch):
    """ops.bigru_lens with the overlap knob on (rows >= 8192, T >= 256) -> ft_gru_layer_fwd_lens: 4 chunks of 64 steps
    behind gate words; the reverse direction of a group starts (T - min L) rows into its descending chunk order -- a
    group holding an L = 1 item waits for all four chunks at its first step.  Same kernels, same rows as the projection
    in front: bit-identical to it, and within the forward bar of test_gpu_rnn.py of torch.nn.GRU over the packed batch."""
    from forwardtacotron_amd import hip, model
    B, T, I, Hh = 32, 256, 12, 16
    g = torch.Generator().manual_seed(21)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0], lens[5], lens[16], lens[31] = T, 1, 200, 63          # (group 0 holds L = 1; group 1 starts 56 rows in)
    torch.manual_seed(22)
    ref = torch.nn.GRU(I, Hh, batch_first=True, bidirectional=True)
    x = torch.randn(B, T, I, generator=g)
    with torch.no_grad():
        packed = torch.nn.utils.rnn.pack_padded_sequence(x.double(), lens, batch_first=True, enforce_sorted=False)
        yo, _ = torch.nn.utils.rnn.pad_packed_sequence(ref.double()(packed)[0], batch_first=True, total_length=T)
    ref = ref.float()
    m = model.GRU(I, Hh)
    m.load_state_dict(ref.state_dict())
    m = m.cuda()
    calls = []
    inner = hip.gru_layer_fwd_lens

    def spy(*a):
        calls.append(a[-1])
        return inner(*a)

    monkeypatch.setattr(hip, 'gru_layer_fwd_lens', spy)
    xd, ld = x.cuda(), lens.cuda()
    with torch.no_grad():
        whole = m.forward_lens(xd, ld).cpu()
        assert calls == []
        monkeypatch.setenv('FT_RNN_OVERLAP', '1')
        c0 = hip.rnn_counters()
        chunked = m.forward_lens(xd, ld).cpu()
        torch.cuda.synchronize()
        hip.check_rnn_status()
        c1 = hip.rnn_counters()
    assert calls == [4], 'expected one ft_gru_layer_fwd_lens call with 4 chunks'
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0), 'the gated recurrence is the persistent form'
    beyond = torch.arange(T)[None, :] >= lens[:, None]
    assert bool((chunked[beyond] == 0).all()), 'outputs at t >= L_b must be exactly 0'
    d = maxdiff(chunked, yo)
    print(f'chunked projection: {d:.3e} off torch.nn.GRU over the packed batch')
    assert d < 2e-5
    assert torch.equal(chunked, whole), 'the chunked projection changed the result'


# ---- embedding of a ragged batch -----------------------------------------------------------------------------------
def _flag_clear(dev):
    from forwardtacotron_amd import hip
    try:
        hip.check_index_errors(dev)
    except IndexError:
        pass


def test_embedding_lens_does_not_read_the_padding():
    from forwardtacotron_amd import hip
    B, T, V, C = 4, 9, 11, 6
    g = torch.Generator().manual_seed(31)
    w = torch.randn(V, C, generator=g).cuda()
    lens = torch.tensor([9, 1, 5, 3])
    pad = torch.arange(T)[None, :] >= lens[:, None]
    idx = torch.randint(0, V, (B, T), generator=g)
    junk = torch.where(torch.arange(B * T).reshape(B, T) % 2 == 0, torch.tensor(-7), torch.tensor(V + 1000))
    dev = w.device
    _flag_clear(dev)
    want = hip.mask_rows(hip.embedding_fwd(idx.cuda(), w), lens.cuda())
    got = hip.embedding_fwd_lens(torch.where(pad, junk, idx).cuda(), lens.cuda(), w)
    assert torch.equal(got, want) and torch.equal(got.cpu()[~pad], w.cpu()[idx[~pad]])
    hip.check_index_errors(dev)                         # ids outside the vocabulary in the padding: no flag
    bad = idx.clone()
    bad[2, 4] = V                                       # the last VALID token of item 2
    out = hip.embedding_fwd_lens(bad.cuda(), lens.cuda(), w)
    assert bool((out[2, 4] == 0).all())
    with pytest.raises(IndexError):
        hip.check_index_errors(dev)


def test_generate_batch_with_ids_outside_the_vocabulary_in_the_padding():
    """'entries at t >= x_len[b] are ignored, whatever they hold': same bits as the zero-padded batch, and the sticky
    out-of-range flag of the embeddings stays down for the next caller of check_index_errors"""
    from forwardtacotron_amd import hip, model
    G = load_npz('generate_batch.npz')
    m = model.ForwardTacotron(**TINY)
    m.load_state_dict(sub(G, 'sd/'))
    m = m.cuda()
    x, x_len = torch.from_numpy(G['x']), torch.from_numpy(G['x_len'])
    pad = torch.arange(x.shape[1])[None, :] >= x_len[:, None]
    junk = torch.where(torch.arange(x.numel()).reshape(x.shape) % 2 == 0, torch.tensor(-3), torch.tensor(TINY['num_chars'] + 7))
    _flag_clear(x.cuda().device)
    out = m.generate_batch(x.cuda(), x_len, alpha=float(G['alpha']))
    out2 = m.generate_batch(torch.where(pad, junk, x).cuda(), x_len, alpha=float(G['alpha']))
    for k in out:
        assert torch.equal(out2[k], out[k]), f'{k} depends on what the padding holds'
    hip.check_index_errors(out['mel'].device)
