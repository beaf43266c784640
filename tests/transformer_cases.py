"""The ForwardTransformer cases of tests/test_gpu_transformer_routes.py and their float64 reference (CPU side, shared with
tests/test_transformer_oracle_cpu.py, which checks the reference itself without a GPU).

A case is one ForwardTransformer (common_layers.py:188-223) alone: parameters perturbed by 0.05 * randn (every layer of the
reference starts as a deepcopy of ONE block; identical layers would hide a block mix-up), an input x [B,T,d], a ragged key
padding mask and a fixed weight tensor w for the loss (y * w).sum() over ALL rows -- neither the reference nor this project
masks the k > 1 convolutions in training, so padded query rows feed valid ones.
"""
import functools

import torch

#        id                 d   heads d_fft k1 k2 layers B  T    lens
CASES = {
    # T not a multiple of the fused attention's 64-key block; two blocks chained through the aliased arenas
    'hd64_T70_2layers': dict(d=128, nh=2, f=192, k1=9, k2=1, layers=2, B=3, T=70, lens=[70, 41, 64]),
    # head width 128; k2 > 1 through the ReLU-masked data gradient; T just over the 128-query workgroup
    'hd128_T129_k3k3': dict(d=128, nh=1, f=96, k1=3, k2=3, layers=2, B=2, T=129, lens=[129, 65]),
    # no mask pointer, a single short item
    'hd64_T7_nomask': dict(d=128, nh=2, f=192, k1=9, k2=1, layers=1, B=1, T=7, lens=None),
    # B * T above the row count at which the in-projection's GEMM switches to the 128x128 tile
    'hd128_T841_wide_tiles': dict(d=256, nh=2, f=256, k1=9, k2=1, layers=1, B=5, T=841, lens=[841, 500, 777, 64, 613]),
}


def err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got - ref| / max(1, max|ref|), the error test_fastpitch_mid_size_vs_oracle uses"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """-> (state dict of the perturbed ForwardTransformer, x [B,T,d], bool pad mask [B,T] or None, w [B,T,d]), fp32 CPU"""
    from forwardtacotron_amd.fastpitch import ForwardTransformer
    c = CASES[name]
    torch.manual_seed(sorted(CASES).index(name) + 101)
    m = ForwardTransformer(c['d'], c['f'], c['layers'], c['nh'], c['k1'], c['k2'], dropout=0.0)
    g = torch.Generator().manual_seed(c['T'] * 7 + c['d'])
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g))
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.randn(c['B'], c['T'], c['d'], generator=g)
    w = torch.randn(c['B'], c['T'], c['d'], generator=g)
    pad = None
    if c['lens'] is not None:
        assert len(c['lens']) == c['B'] and c['lens'][0] == c['T']
        pad = torch.arange(c['T'])[None, :] >= torch.tensor(c['lens'])[:, None]
    return P, x, pad, w


def reference(name: str, dtype=torch.float64):
    """oracle.fp_oracle.forward_transformer (dtype-agnostic) on `dtype` copies with requires_grad
    -> {'y', 'dx', <parameter name>: gradient}, pos_encoder.scale included"""
    from oracle import fp_oracle as FP
    c = CASES[name]
    P, x, pad, w = inputs(name)
    Pd = {k: v.to(dtype).requires_grad_(FP.is_param(k)) for k, v in P.items()}
    xd = x.to(dtype).requires_grad_(True)
    y = FP.forward_transformer(xd, pad, Pd, '', c['nh'], c['layers'])
    (y * w.to(dtype)).sum().backward()
    out = {'y': y.detach(), 'dx': xd.grad}
    out.update({k: v.grad for k, v in Pd.items() if FP.is_param(k)})
    assert all(v is not None for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def reference64(name: str):
    return reference(name, torch.float64)
