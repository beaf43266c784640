"""The ForwardTransformer cases of tests/test_gpu_transformer_routes.py and their float64 reference (CPU side, shared with
tests/test_transformer_oracle_cpu.py, which checks the reference itself without a GPU).

A case is one ForwardTransformer (common_layers.py:188-223) alone: parameters perturbed by 0.05 * randn (every layer of the
reference starts as a deepcopy of ONE block; identical layers would hide a block mix-up), an input x [B,T,d], a ragged key
padding mask and a fixed weight tensor w for the loss (y * w).sum() over ALL rows -- neither the reference nor this project
masks the k > 1 convolutions in training, so padded query rows feed valid ones.

With dropout p > 0 the reference gets the masks the GPU run will draw, built on the CPU (tests/dropout_cpu.py) from the
seeds base._seed() hands out after torch.manual_seed(DROPOUT_TORCH_SEED), in the draw order every route documents
(fastpitch.TransformerFn): the positional-encoding seed first, then per layer attention, norm1, norm2.
"""
import functools

import numpy as np
import torch

DROPOUT_TORCH_SEED = 4242      # the seed test_gpu_transformer_routes.py installs in front of every forward

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


def dropout_masks(name: str, p: float, dtype=torch.float64, masked: bool = True):
    """the masks argument of oracle.fp_oracle.forward_transformer for the case at dropout p (every site of a
    ForwardTransformer has the same p); masked=False with p = 0 -> None, the unmasked call"""
    import dropout_cpu as D
    if p <= 0.0 and not masked:
        return None
    c = CASES[name]
    B, T, d, nh = c['B'], c['T'], c['d'], c['nh']
    seeds = iter(D.seed_stream(DROPOUT_TORCH_SEED, 1 + 3 * c['layers']))
    npdt = np.float64 if dtype == torch.float64 else np.float32
    site = lambda shape: torch.from_numpy(D.site_mask(next(seeds), shape, p, npdt)).to(dtype)
    masks = {'pe': site((B, T, d)), 'layers': []}
    for _ in range(c['layers']):
        # both attention forms index [B,nh,T,T]; the LayerNorms index [rows, D] = [B * T, d], the same flat index as [B,T,d]
        masks['layers'].append({'attn': site((B, nh, T, T)), 'res1': site((B, T, d)), 'res2': site((B, T, d))})
    return masks


def reference(name: str, dtype=torch.float64, p: float = 0.0, masked=None):
    """oracle.fp_oracle.forward_transformer (dtype-agnostic) on `dtype` copies with requires_grad, with the dropout
    masks of the case at p (masked=True forces the masked code path at p = 0 too, with masks of ones)
    -> {'y', 'dx', <parameter name>: gradient}, pos_encoder.scale included"""
    from oracle import fp_oracle as FP
    c = CASES[name]
    P, x, pad, w = inputs(name)
    # copies: .to(float32) of the cached fp32 inputs would hand back the cached tensors themselves
    Pd = {k: v.detach().to(dtype, copy=True).requires_grad_(FP.is_param(k)) for k, v in P.items()}
    xd = x.detach().to(dtype, copy=True).requires_grad_(True)
    masks = dropout_masks(name, p, dtype, masked=p > 0 if masked is None else masked)
    y = FP.forward_transformer(xd, pad, Pd, '', c['nh'], c['layers'], masks=masks)
    (y * w.to(dtype)).sum().backward()
    out = {'y': y.detach(), 'dx': xd.grad}
    out.update({k: v.grad for k, v in Pd.items() if FP.is_param(k)})
    assert all(v is not None for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def reference64(name: str, p: float = 0.0):
    return reference(name, torch.float64, p)
