"""The float64 reference of tests/test_gpu_transformer_routes.py, checked without a GPU: oracle.fp_oracle.forward_transformer
(the restatement of common_layers.py:188-223 that tests/golden/tiny_fastpitch.npz pins in fp32) is dtype-agnostic, and its
float64 run of the first case agrees with its float32 run to fp32 rounding -- output, dx and the gradient of every parameter.
A reference that were wrong in float64 only (a stray .float(), a constant built in fp32) would show here, not as a GPU
failure.

Bars: 2e-5 on the output and 1e-4 * max(1, |g|max) on the gradients, the bars the suite holds fp32 HIP kernels to against the
same oracle (tests/test_gpu_fastpitch.py, tests/test_gpu_full_parity.py); two fp32 / float64 runs of one torch program stay
well inside them (sums of at most 210 rows x 9 taps x 192 channels in fp32)."""
import torch

from transformer_cases import CASES, err, reference, reference64


def test_float64_reference_agrees_with_its_float32_run():
    name = next(iter(CASES))
    assert name == 'hd64_T70_2layers'
    r64 = reference64(name)
    r32 = reference(name, torch.float32)
    assert set(r64) == set(r32) and 'pos_encoder.scale' in r64 and 'layers.1.norm2.bias' in r64
    assert len(r64) == 2 + 1 + 2 + 12 * CASES[name]['layers']
    for k, v in r64.items():
        assert v.dtype == torch.float64 and r32[k].dtype == torch.float32, k
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0, k
        e = err(r32[k], v)
        print(f'{k:44s} fp32 vs float64 {e:.3e}')
        assert e <= (2e-5 if k == 'y' else 1e-4), (k, e)
    # the layers really differ (a block mix-up in the code under test cannot hide behind identical blocks)
    assert err(r64['layers.0.conv1.weight'], r64['layers.1.conv1.weight']) > 1e-3


def test_masked_reference_at_p0_is_the_unmasked_one_and_p01_differs():
    """the oracle's `masks` path: masks of ones (p = 0) reproduce the unmasked reference exactly -- a multiplication by 1.0
    changes no bit -- and the p = 0.1 masks of the GPU tests change the output and every gradient but the final norm's bias
    (the column sums of w, whatever lies upstream)"""
    name = 'hd64_T70_2layers'
    plain = reference64(name)
    ones = reference(name, torch.float64, p=0.0, masked=True)
    drop = reference64(name, 0.1)
    assert set(plain) == set(ones) == set(drop)
    for k in plain:
        assert torch.equal(plain[k], ones[k]), k
        assert bool(torch.isfinite(drop[k]).all()), k
        if k == 'norm.bias':
            assert err(drop[k], plain[k]) < 1e-12
        else:
            assert err(drop[k], plain[k]) > 1e-3, k


def test_the_masks_of_a_case():
    """shapes, the two values a mask holds, the rate, and that no two sites of a stack share a mask"""
    from transformer_cases import dropout_masks
    name, p = 'hd64_T70_2layers', 0.1
    c = CASES[name]
    m = dropout_masks(name, p)
    assert tuple(m['pe'].shape) == (c['B'], c['T'], c['d']) and len(m['layers']) == c['layers']
    flat = [m['pe']] + [l[k] for l in m['layers'] for k in ('attn', 'res1', 'res2')]
    assert tuple(m['layers'][0]['attn'].shape) == (c['B'], c['nh'], c['T'], c['T'])
    for t in flat:
        assert t.dtype == torch.float64
        assert set(t.unique().tolist()) == {0.0, 1.0 / (1.0 - float(torch.tensor(p, dtype=torch.float32)))}
        assert abs(float((t == 0).double().mean()) - p) < 0.01
    same_shape = [m['pe']] + [l[k] for l in m['layers'] for k in ('res1', 'res2')]
    for i, a in enumerate(same_shape):
        for b in same_shape[i + 1:]:
            assert 0.1 < float(((a == 0) != (b == 0)).double().mean()) < 0.3        # 2 p (1 - p) = 0.18 if independent
    assert dropout_masks(name, 0.0, masked=False) is None
