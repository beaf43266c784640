"""ft_fft_blocks_bwd with no sums workspace runs its batched bias / LayerNorm column sums inside the weight-gradient
workspace, so ft_fft_block_wgrad_workspace must cover them.  The shape is the smallest one the CPU sweep
(tests/cpp/reduce_plan_main.cpp) finds where the sums need MORE than the four weight gradients' split-K slabs: 961 rows give
the sums 16 chunks, and 512 column tiles of the 64 x 32708 convolution weights leave their gradient one slab.  The call gets
exactly the queried bytes with a guard region behind them, and must give the twelve parameter gradients of the same call
with separate, generous workspaces bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, T, D, HEADS, DFFT, K1, K2 = 1, 961, 64, 1, 32708, 1, 1
GUARD = 1 << 16


def test_blocks_bwd_sums_fit_a_wgrad_workspace_of_exactly_the_queried_size(monkeypatch):
    from forwardtacotron_amd import _lib, fastpitch as F, hip as H
    from forwardtacotron_amd.gradsink import installed
    assert installed() is None
    need = _lib.query('ft_fft_block_wgrad_workspace', B, T, D, DFFT, K1, K2)
    sums = _lib.query('ft_fft_block_sums_workspace', B, T, D, DFFT)
    slabs = 4 * D * DFFT                                    # conv1 / conv2: one slab of 64 x 32708 floats
    assert need == sums == 16 * 16 * (9 * D + DFFT) > slabs

    gen = torch.Generator().manual_seed(0)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=gen) * scale).cuda()

    params = [rnd(3 * D, D, scale=D ** -0.5), rnd(3 * D, scale=0.1), rnd(D, D, scale=D ** -0.5), rnd(D, scale=0.1),
              rnd(DFFT, D, K1, scale=D ** -0.5), rnd(DFFT, scale=0.1), rnd(D, DFFT, K2, scale=DFFT ** -0.5),
              rnd(D, scale=0.1), 1 + rnd(D, scale=0.1), rnd(D, scale=0.1), 1 + rnd(D, scale=0.1), rnd(D, scale=0.1)]
    h, dy = rnd(B, T, D), rnd(B, T, D)
    exact = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    roomy_w = torch.empty(4 * need, dtype=torch.uint8, device='cuda')
    roomy_s = torch.empty(4 * need, dtype=torch.uint8, device='cuda')
    # ft_fft_blocks_bwd(blocks, grads, n, ws, bytes, wgrad ws, bytes, sums ws, bytes, stream, wgrad stream, sums stream)
    tight = (exact.data_ptr(), need, None, 0)
    roomy = (roomy_w.data_ptr(), roomy_w.numel(), roomy_s.data_ptr(), roomy_s.numel())
    real_call, seen = _lib.call, []

    def run(workspaces):
        def call(name, *a):
            if name == 'ft_fft_blocks_bwd':
                a = a[:5] + workspaces + a[9:]
                seen.append(a[5:9])
            return real_call(name, *a)

        monkeypatch.setattr(_lib, 'call', call)
        dx, grads = F.blocks_bwd_composite(state, dy, params)
        monkeypatch.setattr(_lib, 'call', real_call)
        return [dx] + grads

    with H.gemm_precision('bf16'):
        _, state = F.blocks_fwd_composite(h, None, params, HEADS, 0.0, 1e-5, 1e-5, [1, 2, 3])
        got = run(tight)
        want = run(roomy)
    torch.cuda.synchronize()
    assert seen == [tight, roomy]
    assert bool((exact[need:] == 0xA5).all()), 'the call wrote behind its weight-gradient workspace'
    for name, a, b in zip(('dx',) + F._GRAD_FIELDS, got, want):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name
