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
