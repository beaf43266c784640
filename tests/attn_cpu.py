"""The fused training attention of csrc/ft_attn.hip (ft_attn_fwd / ft_attn_bwd), restated twice in torch on the host.

reference(): exact float64 attention and its gradients on the bf16-rounded q / k / v (the rounding of the operands is
    what the bf16 mode defines as its input; `datt` is not rounded): att, lse2 (log2 domain), dq, dk, dv.
emulate():   the same math with the kernels' rounding points and nothing else, read off the file header of ft_attn.hip and
    the three kernel bodies:
      forward   x = K Q^T in fp32, v = x * (scale * log2 e) in fp32; online softmax over 64-key blocks: p = exp2(v - m)
                as an fp32, m the running maximum (0 where it still is -inf); l sums the p BEFORE the dropout and before
                any bf16 rounding, and is an fp32 from block to block; p * keep is rounded to bf16 before PV;
                att = o / l and lse2 = m + log2 l are stored as fp32;
      delta     sum_d datt * att from the fp32 datt and the forward's own att;
      backward  datt is rounded to bf16 for dP = dO V^T and for dV; P = exp2(v - lse2) from the stored lse2;
                dS = scale * P * (keep * dP - delta) is rounded to bf16 before the dQ and the dK product; Pd = P * keep is
                rounded to bf16 before dV.
    Everything else is float64 (acc=torch.float64) -- or fp32 with the blocks summed in reverse order (acc=torch.float32,
    reverse=True): a legitimate other summation order, which the bar of the GPU tests has to leave room for.
    `mutate` / `where` switch on one wrong variant at the forward ('fwd'), the dQ kernel ('dq') or the dK/dV kernel
    ('dkv'): what tests/test_attn_cpu.py proves the bar of tests/test_gpu_attn_train.py to catch.

`keep` is dropout_cpu.site_mask(seed, (B, nh, T, T), p): 0 or 1 / (1 - p) per probability, ones at p = 0.  `key_pad` is any
byte mask [B, T] (non-zero = masked key) or None.  Padded QUERIES attend to the valid keys like every other row, as in
torch.  An item whose keys are all masked gives NaN, as in torch.

The cases of the GPU tests live here too (CASES, make_case), so that the CPU test proves its claims on the very inputs
the GPU test uses.  Nothing here touches the GPU or the package."""
import math
from collections import OrderedDict

import numpy as np
import torch

import dropout_cpu as D

KB = 64                                   # keys per block (ft_attn_tile.h)
LOG2E = np.float32(1.44269504088896341)
U32 = 2.0 ** -24
OUTPUTS = ('att', 'lse2', 'dq', 'dk', 'dv')
SITES = ('fwd', 'dq', 'dkv')
MUTATIONS = ('last_key', 'key64', 'mask_shift', 'mask_swap', 'mask_nohead', 'no_delta', 'delta_all_heads', 'keep_on_p',
             'no_scale', 'lse_natural', 'l_after_dropout')


def _heads(x, nh):
    """[B,T,nh*hd] -> [B,nh,T,hd]"""
    B, T, d = x.shape
    return x.reshape(B, T, nh, d // nh).permute(0, 2, 1, 3)


def _rows(x):
    """[B,nh,T,hd] -> [B,T,nh*hd]"""
    B, nh, T, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, nh * hd).contiguous()


def _bf(x):
    """round to bf16 the way the kernels do (from the fp32 value), keep x's dtype"""
    return x.float().bfloat16().to(x.dtype)


def _f32(x):
    return x.float().to(x.dtype)


def _masked(key_pad, B, T):
    return torch.zeros(B, T, dtype=torch.bool) if key_pad is None else key_pad.bool().cpu().clone()


def reference(qkv, datt, key_pad, nh, scale, keep):
    """-> dict att [B,T,d], lse2 [B,nh,T], dq / dk / dv [B,T,d], float64"""
    B, T, d3 = qkv.shape
    d = d3 // 3
    q, k, v = (_heads(t.float().bfloat16().double(), nh) for t in qkv.cpu().split(d, dim=-1))
    g = _heads(datt.cpu().double(), nh)
    keep = torch.as_tensor(np.asarray(keep), dtype=torch.float64).reshape(B, nh, T, T)
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(_masked(key_pad, B, T)[:, None, None, :], float('-inf'))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = e / l
    lse2 = ((m + torch.log(l)) / math.log(2.0)).squeeze(-1)
    Pd = P * keep
    att = Pd @ v
    dP = (g @ v.transpose(-1, -2)) * keep
    delta = (P * dP).sum(-1, keepdim=True)              # a single key: P = 1 and dS = 0 exactly
    dS = P * (dP - delta) * scale
    return dict(att=_rows(att), lse2=lse2, dq=_rows(dS @ k), dk=_rows(dS.transpose(-1, -2) @ q),
                dv=_rows(Pd.transpose(-1, -2) @ g))


def _mutated_keep(keep, mutate):
    """the mask a kernel with a wrong element index would draw: keep is the contiguous [B,nh,T,T] site mask"""
    B, nh, T, _ = keep.shape
    if mutate == 'mask_shift':                          # index + 1: the next key, the next row's key 0 behind the last
        flat = keep.reshape(-1)
        return torch.cat([flat[1:], flat[:1]]).reshape(keep.shape)
    if mutate == 'mask_swap':                           # (inst*T + k)*T + q
        return keep.transpose(-1, -2)
    if mutate == 'mask_nohead':                         # inst = b
        return keep.reshape(B * nh, T, T)[:B][:, None].expand(B, nh, T, T)
    return keep


def _mutated_mask(masked, mutate):
    masked = masked.clone()
    if mutate == 'last_key':                            # `>` for `>=`: the last valid key of each item is lost
        for b in range(masked.shape[0]):
            valid = (~masked[b]).nonzero()
            if valid.numel():
                masked[b, int(valid[-1])] = True
    if mutate == 'key64' and masked.shape[1] > KB:      # the first key of the second block
        masked[:, KB] = True
    return masked


def emulate(qkv, datt, key_pad, nh, scale, keep, mutate=None, where=SITES, acc=torch.float64, reverse=False):
    """-> the same dict as reference(), in dtype `acc`"""
    assert mutate is None or mutate in MUTATIONS
    B, T, d3 = qkv.shape
    d = d3 // 3
    hd = d // nh
    q, k, v = (_heads(t.float().bfloat16().to(acc), nh) for t in qkv.cpu().split(d, dim=-1))
    g32 = _heads(datt.cpu().float().to(acc), nh)
    g = _bf(g32)
    keep = torch.as_tensor(np.asarray(keep), dtype=torch.float64).reshape(B, nh, T, T).float().to(acc)
    scale32 = np.float32(scale)
    c = float(scale32 * LOG2E)                          # the kernels' fp32 product
    scale32 = float(scale32)
    masked0 = _masked(key_pad, B, T)
    site = lambda s: mutate if s in where else None
    blocks = [slice(i, min(i + KB, T)) for i in range(0, T, KB)]
    if reverse:
        blocks = blocks[::-1]
    neg_inf = float('-inf')

    x = _f32(q @ k.transpose(-1, -2))                   # fp32 accumulators of the bf16 products
    xc = _f32(x * c)

    # ---- forward
    mask = _mutated_mask(masked0, site('fwd'))[:, None, None, :]
    kp = _mutated_keep(keep, site('fwd'))
    vv = xc.masked_fill(mask, neg_inf)
    m = torch.full((B, nh, T), neg_inf, dtype=acc)
    l = torch.zeros(B, nh, T, dtype=acc)
    o = torch.zeros(B, nh, T, hd, dtype=acc)
    for ks in blocks:
        vb = vv[..., ks]
        mnew = torch.maximum(m, vb.max(-1).values)
        msafe = torch.where(mnew == neg_inf, torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - msafe)
        p = _f32(torch.exp2(vb - msafe[..., None]))     # v_exp_f32 returns an fp32
        pk = p * kp[..., ks]
        lsum = (pk if site('fwd') == 'l_after_dropout' else p).sum(-1)
        o = o * alpha[..., None] + _bf(pk) @ v[..., ks, :]
        l = _f32(l * alpha + _f32(lsum))                # the row sum is carried in fp32 from block to block
        m = mnew
    att = _f32(o / l[..., None])
    lse2 = m + _f32(torch.log2(l))
    if site('fwd') == 'lse_natural':
        lse2 = lse2 * math.log(2.0)
    lse2 = _f32(lse2)

    # ---- delta: fp32 datt, the forward's own att
    delta = (g32 * att).sum(-1)
    if mutate == 'delta_all_heads':
        delta = delta.sum(1, keepdim=True).expand(B, nh, T).contiguous()
    if mutate == 'no_delta':
        delta = torch.zeros_like(delta)

    y = _f32(g @ v.transpose(-1, -2))                   # dP before the dropout

    def tiles(s):
        mk = _mutated_mask(masked0, site(s))[:, None, None, :]
        kq = _mutated_keep(keep, site(s))
        P = torch.exp2(xc - lse2[..., None]).masked_fill(mk, 0.0)
        if site(s) == 'keep_on_p':
            dS = (P * kq) * (y - delta[..., None])
        else:
            dS = P * (y * kq - delta[..., None])
        if site(s) != 'no_scale':
            dS = scale32 * dS
        return _bf(P * kq), _bf(dS)

    # ---- dQ: sum over the key blocks
    _, dS = tiles('dq')
    dq = torch.zeros(B, nh, T, hd, dtype=acc)
    for ks in blocks:
        dq = dq + dS[..., ks] @ k[..., ks, :]

    # ---- dK, dV: sum over the query blocks
    Pd, dS = tiles('dkv')
    dk = torch.zeros(B, nh, T, hd, dtype=acc)
    dv = torch.zeros(B, nh, T, hd, dtype=acc)
    for qs in blocks:
        dk = dk + dS[..., qs, :].transpose(-1, -2) @ q[..., qs, :]
        dv = dv + Pd[..., qs, :].transpose(-1, -2) @ g[..., qs, :]
    return dict(att=_rows(att), lse2=lse2, dq=_rows(dq), dk=_rows(dk), dv=_rows(dv))


# ---------------------------------------------------------------------------------------------------
# per-slab comparison: a slab is one (item, head) of one output, over all T rows
# ---------------------------------------------------------------------------------------------------
def slabs(name, x, nh):
    """[B,nh,T*hd or T]: every (item, head) slab of output `name` as one row"""
    x = torch.as_tensor(x).double()
    if name == 'lse2':
        return x
    return _heads(x, nh).reshape(x.shape[0], nh, -1)


def slab_err(name, got, ref, nh):
    """max |got - ref| per slab [B,nh]; NaN where either side has one"""
    diff = (slabs(name, got, nh) - slabs(name, ref, nh)).abs()
    return torch.where(torch.isnan(diff).any(-1), torch.full(diff.shape[:2], float('nan'), dtype=diff.dtype),
                       diff.nan_to_num(0.0).max(-1).values)


def slab_bar(name, emu, ref, nh):
    """4 E + 16 * 2^-24 * max(1, max|ref|) per slab [B,nh], E = max |emulate - reference| over the slab.  The 4 is the
    room the project gives a kernel over a yardstick for summation order and v_exp_f32 (tests/test_gpu_attn_lens.py),
    the floor is the one of tests/test_gpu_taco_kernels.py."""
    E = slab_err(name, emu, ref, nh)
    top = slabs(name, ref, nh).abs().max(-1).values
    return 4 * E + 16 * U32 * torch.clamp(top, min=1.0), E


# ---------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_attn_train.py
# ---------------------------------------------------------------------------------------------------
EDGE_LENS = [1, 63, 64, 65, 128, 129, 200]


def _suffix(lens, T):
    return (torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]).to(torch.uint8).contiguous()


def _byte_masks(T):
    """four masks that are no suffix: keys 0..63 (the first block wholly masked: the online softmax starts a row at
    m = -inf), keys 64..127, every second key, all keys but the last"""
    kp = torch.zeros(4, T, dtype=torch.uint8)
    kp[0, :64] = 1
    kp[1, 64:128] = 1
    kp[2, 1::2] = 1
    kp[3, :T - 1] = 1
    return kp


def _cases():
    out = OrderedDict()
    n = 0
    for hd in (64, 128):
        for p in (0.0, 0.1):
            out[f'edges-hd{hd}-p{p}'] = dict(B=7, T=200, nh=2, hd=hd, p=p, lens=EDGE_LENS)
    for nh, hd in ((1, 64), (3, 64), (1, 128), (3, 128)):
        out[f'heads-nh{nh}-hd{hd}'] = dict(B=2, T=70, nh=nh, hd=hd, p=0.1, lens=[70, 33])
    for T in (1, 2, 31, 33, 129):
        for p in (0.0, 0.5):
            for hd in (64, 128):
                out[f'small-T{T}-hd{hd}-p{p}-nomask'] = dict(B=2, T=T, nh=2, hd=hd, p=p, lens=None)
                out[f'small-T{T}-hd{hd}-p{p}-lens'] = dict(B=2, T=T, nh=2, hd=hd, p=p, lens=[T, max(1, T - 1)])
    for hd in (64, 128):
        for p in (0.0, 0.1):
            out[f'bytes-hd{hd}-p{p}'] = dict(B=4, T=200, nh=2, hd=hd, p=p, lens='bytes')
    for n, c in enumerate(out.values()):
        c['index'] = n
    return out


CASES = _cases()
_SEEDS = D.seed_stream(20240, len(CASES))


def make_case(name):
    """-> dict with the inputs of case `name` (qkv, datt fp32 on the host; key_pad uint8 or None; nh, hd, scale, p, seed,
    keep) -- `randn * 0.7` operands as in the existing attention test, seeds from the stream base._seed() draws from"""
    c = dict(CASES[name])
    B, T, nh, hd = c['B'], c['T'], c['nh'], c['hd']
    g = torch.Generator().manual_seed(1000 + c['index'])
    c['qkv'] = torch.randn(B, T, 3 * nh * hd, generator=g) * 0.7
    c['datt'] = torch.randn(B, T, nh * hd, generator=g)
    lens = c['lens']
    c['key_pad'] = None if lens is None else _byte_masks(T) if lens == 'bytes' else _suffix(lens, T)
    c['scale'] = 1.0 / math.sqrt(hd)
    c['seed'] = _SEEDS[c['index']]
    c['keep'] = D.site_mask(c['seed'], (B, nh, T, T), c['p'])
    c['name'] = name
    return c


def args(c):
    return c['qkv'], c['datt'], c['key_pad'], c['nh'], c['scale'], c['keep']
