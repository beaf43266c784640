"""GPU: ft_attn_fwd_lens at head widths 192 and 256 (the multispeaker models), through hip.attn_fwd_lens, both precisions.

These widths run in 32-key blocks with 64-query workgroups, the head width split over a pair of waves.  T = 200; the
lengths sit on, one before and one behind every 32- / 64-key block and every 64- / 128-query workgroup boundary, plus the
shortest and the full item.  There is no fused byte-mask kernel at these widths, hence no bf16 bit-equality test."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

T, NH = 200, 2
LENS = [1, 31, 32, 33, 63, 64, 65, 97, 128, 129, 200]
B = len(LENS)
CASES = [(192, 'fp32'), (256, 'fp32'), (192, 'bf16'), (256, 'bf16')]
U32, UBF = 2.0 ** -24, 2.0 ** -9          # unit roundoffs of fp32 and bf16


def _qkv(hd, seed, batch=B, t=T):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(batch, t, 3 * NH * hd, generator=g)


def _key_pad(lens, t):
    return (torch.arange(t)[None, :] >= torch.tensor(lens)[:, None]).to(torch.uint8).contiguous()


def _run(qkv, lens, mode):
    from forwardtacotron_amd import hip
    hd = qkv.shape[2] // 3 // NH
    with hip.gemm_precision(mode):
        return hip.attn_fwd_lens(qkv.cuda(), torch.tensor(lens).cuda(), NH, 1.0 / math.sqrt(hd)).cpu()


def _reference(qkv, lens, mode):
    """float64 restatement per item over its first L rows -> ([att_b [L,d]], [tolerance_b]); the tolerance of
    test_gpu_attn_lens.py::_reference, restated: from the number formats alone.  With u the unit roundoff of the products'
    operands (bf16 mode: 2^-9 for q, k, v and the probabilities; fp32 mode: exact products) and n = hd fp32 accumulation
    steps, a score is off by at most ds = scale * (2 u_op + (n + 3) 2^-24) * max_qk sum_i |q_i k_i| + 2^-22 max|s|; a
    probability by the relative eps = exp(2 ds) - 1 + u_p + 4 * 2^-24; the output, a weighted mean of the v rows, by
    2 eps / (1 - eps) * max|v| plus the rounding of v and of the L-term fp32 sum.  (The pairwise sum of the two partial
    score tiles is one of the n + 3 accumulation steps.)"""
    d = qkv.shape[2] // 3
    hd = d // NH
    scale = 1.0 / math.sqrt(hd)
    u_op = UBF if mode == 'bf16' else 0.0
    outs, tols = [], []
    for b, L in enumerate(lens):
        x = qkv[b, :L].double()
        att = torch.empty(L, d, dtype=torch.float64)
        tol = 0.0
        for h in range(NH):
            q, k, v = (x[:, i * d + h * hd:i * d + (h + 1) * hd] for i in range(3))
            s = scale * q @ k.T
            att[:, h * hd:(h + 1) * hd] = torch.softmax(s, dim=-1) @ v
            ds = scale * (2 * u_op + (hd + 3) * U32) * float((q.abs() @ k.abs().T).max()) + 4 * U32 * float(s.abs().max())
            eps = math.expm1(2 * ds) + u_op + 4 * U32
            tol = max(tol, (2 * eps / (1 - eps) + u_op + (L + 2) * U32) * float(v.abs().max()))
        outs.append(att)
        tols.append(tol)
    return outs, tols


@pytest.fixture(scope='module')
def cases():
    """{(hd, mode): (qkv, kernel output, float64 reference per item, tolerance per item)} -- computed once"""
    out = {}
    for hd, mode in CASES:
        qkv = _qkv(hd, 100 + hd)
        ref, tol = _reference(qkv, LENS, mode)
        out[(hd, mode)] = (qkv, _run(qkv, LENS, mode), ref, tol)
    return out


def _err(att, ref, lens):
    return max(float((att[b, :L].double() - ref[b]).abs().max()) for b, L in enumerate(lens))


@pytest.mark.parametrize('hd,mode', CASES)
def test_valid_rows_vs_float64(cases, hd, mode):
    qkv, att, ref, tol = cases[(hd, mode)]
    assert att.shape == (B, T, NH * hd)
    for b, L in enumerate(LENS):
        e = float((att[b, :L].double() - ref[b]).abs().max())
        print(f'hd {hd} {mode} item {b} (L = {L}): {e:.3e} off float64, tolerance {tol[b]:.3e}')
        assert e <= tol[b], (b, L, e, tol[b])


@pytest.mark.parametrize('hd,mode', CASES)
def test_rows_past_the_length_are_exactly_zero(cases, hd, mode):
    _, att, _, _ = cases[(hd, mode)]
    for b, L in enumerate(LENS):
        assert bool((att[b, L:] == 0).all()), (b, L)


@pytest.mark.parametrize('hd', [192, 256])
def test_fp32_error_against_the_unfused_route(cases, hd):
    """e_new <= 4 e_old (test_gpu_attn_lens.py): the margin covers the online-softmax rescaling and the other summation
    order, not reduced-precision products"""
    from forwardtacotron_amd import hip
    from forwardtacotron_amd.fastpitch import _attn_unfused
    qkv, att, ref, _ = cases[(hd, 'fp32')]
    with hip.gemm_precision('fp32'):
        old = _attn_unfused(qkv.cuda(), _key_pad(LENS, T).cuda(), NH, 1.0 / math.sqrt(hd), 0.0, 0)[0].cpu()
    e_new, e_old = _err(att, ref, LENS), _err(old, ref, LENS)
    print(f'hd {hd} fp32: e_new {e_new:.3e} (ft_attn_fwd_lens), e_old {e_old:.3e} (bgemm / softmax / bgemm), '
          f'ratio {e_new / e_old:.2f}')
    assert e_new <= 4 * e_old, (e_new, e_old)


@pytest.mark.parametrize('hd,mode', CASES)
def test_nan_in_the_padding_never_reaches_a_valid_row(cases, hd, mode):
    qkv, att, _, _ = cases[(hd, mode)]
    poisoned = qkv.clone()
    poisoned[torch.arange(T)[None, :] >= torch.tensor(LENS)[:, None]] = float('nan')
    assert bool(torch.isnan(poisoned[0, 1:]).all()) and not bool(torch.isnan(poisoned[B - 1]).any())
    att2 = _run(poisoned, LENS, mode)
    assert torch.equal(att2, _run(torch.nan_to_num(poisoned, nan=0.0), LENS, mode))     # zeros there: bit-identical
    for b, L in enumerate(LENS):
        assert torch.equal(att2[b, :L], att[b, :L]) and bool((att2[b, L:] == 0).all()), (b, L)


@pytest.mark.parametrize('hd,mode', CASES)
def test_neighbours_are_irrelevant(cases, hd, mode):
    qkv, att, _, _ = cases[(hd, mode)]
    other = _qkv(hd, 7)
    for b in (3, 7):                               # 33 and 97 keys, moved between other neighbours
        other[b] = qkv[b]
    lens2 = [200, 5, 130, LENS[3], 1, 77, 64, LENS[7], 31, 200, 2]
    att2 = _run(other, lens2, mode)
    for b in (3, 7):
        assert torch.equal(att2[b, :LENS[b]], att[b, :LENS[b]]), b
    assert torch.equal(_run(qkv[7:8].contiguous(), [LENS[7]], mode)[0, :LENS[7]], att[7, :LENS[7]])    # and alone


@pytest.mark.parametrize('hd', [192, 256])
def test_single_key_returns_the_v_row(hd):
    qkv = _qkv(hd, 5, batch=1, t=1)
    att = _run(qkv, [1], 'fp32')
    assert torch.equal(att[0, 0], qkv[0, 0, 2 * NH * hd:])


@pytest.mark.parametrize('hd,mode', CASES)
def test_lengths_are_clamped(hd, mode):
    t = 70
    qkv = _qkv(hd, 9, batch=2, t=t)
    att = _run(qkv, [0, t + 5], mode)
    assert bool((att[0] == 0).all())
    assert torch.equal(att[1], _run(qkv, [1, t], mode)[1])
    ref, tol = _reference(qkv[1:], [t], mode)
    assert float((att[1].double() - ref[0]).abs().max()) <= tol[0]
