"""GPU: the two small kernels under the speaker-conditioned generate_batch, alone: ft_predictor_front_lens (a gather:
bit-equal to torch.cat of indexed rows) and ft_argmax_lens (torch.argmax per token)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _front_case(Ce, Cc, S, seed, B=4, T=9, V=11, Vc=4):
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([1, T, 5, T - 1][:B])
    idx = torch.randint(0, V, (B, T), generator=g)
    cond = torch.randint(0, Vc, (B, T), generator=g) if Cc else None
    w = torch.randn(V, Ce, generator=g)
    cw = torch.randn(Vc, Cc, generator=g) if Cc else None
    semb = torch.randn(B, S, generator=g) if S else None
    parts = [w[idx]] + ([cw[cond]] if Cc else []) + ([semb[:, None, :].expand(B, T, S)] if S else [])
    want = torch.cat(parts, dim=2)
    want[torch.arange(T)[None, :] >= lens[:, None]] = 0.0
    return idx, cond, lens, w, cw, semb, want


def _front(idx, cond, lens, w, cw, semb):
    from forwardtacotron_amd import hip
    c = lambda t: None if t is None else t.cuda()      # noqa: E731
    out = hip.predictor_front_lens(c(idx), c(lens), c(w), c(cond), c(cw), c(semb))
    torch.cuda.synchronize()
    return out.cpu()


# (Ce, Cc, S): the production predictor front (widths that are no multiple of 4 in sum or in part), a front without
# the cond part, one without the speaker part, and the trunk's front of the tiny config
@pytest.mark.parametrize('Ce,Cc,S', [(8, 4, 256), (16, 0, 8), (6, 3, 0), (5, 3, 7)])
def test_front_is_the_gather(Ce, Cc, S):
    from forwardtacotron_amd import hip
    idx, cond, lens, w, cw, semb, want = _front_case(Ce, Cc, S, 1)
    hip._err_flag('cuda').zero_()
    out = _front(idx, cond, lens, w, cw, semb)
    assert out.shape == want.shape and torch.equal(out, want)
    hip.check_index_errors('cuda')                 # nothing raised


@pytest.mark.parametrize('Ce,Cc,S', [(8, 4, 256), (16, 0, 8)])
def test_front_does_not_read_ids_in_the_padding(Ce, Cc, S):
    from forwardtacotron_amd import hip
    idx, cond, lens, w, cw, semb, want = _front_case(Ce, Cc, S, 2)
    pad = torch.arange(idx.shape[1])[None, :] >= lens[:, None]
    idx = torch.where(pad, torch.full_like(idx, 10 ** 9), idx)
    if cond is not None:
        cond = torch.where(pad, torch.full_like(cond, -7), cond)
    hip._err_flag('cuda').zero_()
    out = _front(idx, cond, lens, w, cw, semb)
    assert torch.equal(out, want)
    hip.check_index_errors('cuda')                 # out-of-range ids in the padding raise no flag


def test_front_flags_an_out_of_range_id_inside_a_sentence():
    from forwardtacotron_amd import hip
    idx, cond, lens, w, cw, semb, want = _front_case(8, 4, 16, 3)
    cond[1, 2] = 4                                 # Vc = 4
    hip._err_flag('cuda').zero_()
    out = _front(idx, cond, lens, w, cw, semb)
    with pytest.raises(IndexError):
        hip.check_index_errors('cuda')
    assert bool((out[1, 2, 8:12] == 0).all()) and torch.equal(out[1, 2, :8], want[1, 2, :8])


def test_argmax_follows_torch():
    from forwardtacotron_amd import hip
    g = torch.Generator().manual_seed(4)
    B, T, K = 3, 300, 3                            # more than one block of 256 tokens
    logits = torch.randn(B, T, K, generator=g)
    logits[0, 0] = torch.tensor([1.0, 1.0, 0.5])   # exact ties: the first index
    logits[0, 1] = torch.tensor([0.5, 2.0, 2.0])
    logits[0, 2] = torch.tensor([3.0, 3.0, 3.0])
    logits[0, 3] = torch.tensor([0.0, float('nan'), 9.0])      # a NaN counts as the maximum
    logits[0, 4] = torch.tensor([float('nan'), 1.0, float('nan')])
    logits[0, 5] = torch.tensor([float('-inf'), float('-inf'), float('-inf')])
    logits[0, 6] = torch.tensor([-0.0, 0.0, -1.0])
    lens = torch.tensor([T, 1, 257])
    want = torch.argmax(logits, dim=2)
    assert want[0, :7].tolist() == [0, 1, 0, 1, 0, 0, 0]
    want[torch.arange(T)[None, :] >= lens[:, None]] = 0
    poisoned = logits.clone()
    poisoned[1, 1:] = float('nan')                 # logits past the length are not looked at
    out = hip.argmax_lens(poisoned.cuda(), lens.cuda()).cpu()
    assert out.dtype == torch.int64 and out.shape == (B, T) and torch.equal(out, want)
    for K2 in (1, 5):
        l2 = torch.randn(2, 7, K2, generator=g)
        assert torch.equal(hip.argmax_lens(l2.cuda(), torch.tensor([7, 7]).cuda()).cpu(), torch.argmax(l2, dim=2))
