"""Rows per workgroup of the 256-wide GRU's persistent forward and all-gather BPTT (the postnet and prenet CBHG GRUs of
the train step).  At B = 32 the 16-row grid runs 4 (direction, batch group) groups on 8 XCD slots; 8 rows per workgroup
give one group per slot.  The 8-row form only moves batch rows between workgroups -- same k blocks per wave, same
reduction orders -- so every output must equal the 16-row form's (FT_RNN_MB=16) bit for bit, and every 8-row group must
still hand over XCD-local."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 256


def _gru_inputs(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    xp = (torch.randn(T, B, 6 * HD, generator=g) * 0.5).cuda()
    whh = [(torch.randn(3 * HD, HD, generator=g) * (1.5 / HD ** 0.5)).cuda() for _ in range(2)]
    bhh = [(torch.randn(3 * HD, generator=g) * 0.1).cuda() for _ in range(2)]
    dout = (torch.randn(T, B, 2 * HD, generator=g) * 0.1).cuda()
    return xp, whh, bhh, dout


def _run(monkeypatch, mb, B, T, seed):
    """(out, saved gates, dxp, dhp, (groups XCD-local, agent-scope), (persistent launches, refused))"""
    from forwardtacotron_amd import hip as H
    xp, whh, bhh, dout = _gru_inputs(B, T, seed)
    wt = [H.transpose2d(w) for w in whh]
    if mb is None:
        monkeypatch.delenv('FT_RNN_MB', raising=False)
    else:
        monkeypatch.setenv('FT_RNN_MB', str(mb))
    m0, c0 = H.rnn_mode_counts(), H.rnn_counters()
    out, gates = H.gru_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], HD, True)
    dxp, dhp = H.gru_bwd(dout, out, gates, wt[0], wt[1], HD)
    torch.cuda.synchronize()
    H.check_rnn_status()
    m1, c1 = H.rnn_mode_counts(), H.rnn_counters()
    modes = (m1[0] - m0[0], m1[1] - m0[1])
    launches = (c1[0] - c0[0], c1[1] - c0[1])
    return out.cpu(), gates.cpu(), dxp.cpu(), dhp.cpu(), modes, launches


@pytest.mark.parametrize('B,T,groups8', [
    (32, 841, 8),             # the benchmark's postnet GRU
    (32, 128, 8),             # the benchmark's prenet GRU
    (20, 37, 6),              # B % 8 != 0: the last 8-row group is partly padding
])
def test_gru_eight_rows_bit_equal_to_sixteen(monkeypatch, B, T, groups8):
    r16 = _run(monkeypatch, 16, B, T, 2000 + B + T)
    r8 = _run(monkeypatch, None, B, T, 2000 + B + T)
    for name, a, b in zip(('out', 'gates', 'dxp', 'dhp'), r8[:4], r16[:4]):
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f'{name}: 8-row form differs from the 16-row form'
    assert r8[5] == (2, 0) and r16[5] == (2, 0), 'forward and BPTT must both run persistent'
    groups16 = 2 * ((B + 15) // 16)
    # every (direction, batch group) group of both launches ran on the XCD-local hand-off
    assert r16[4] == (2 * groups16, 0)
    assert r8[4] == (2 * groups8, 0)


@pytest.mark.parametrize('B', [8, 64])
def test_gru_small_and_full_batches_stay_on_sixteen_rows(monkeypatch, B):
    """B <= 8 (16 rows already make one group per direction) and B = 64 (16-row groups already fill the 8 slots) keep
    the 16-row form: the default run has the FT_RNN_MB=16 run's groups and the same results"""
    r16 = _run(monkeypatch, 16, B, 23, 3000 + B)
    r = _run(monkeypatch, None, B, 23, 3000 + B)
    groups16 = 2 * ((B + 15) // 16)
    assert r[4] == r16[4] == (2 * groups16, 0)
    assert r[5] == r16[5] == (2, 0)
    for a, b in zip(r[:4], r16[:4]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('B', [8, 20, 32, 64])
def test_gru_xcd_fill_of_the_row_forms(monkeypatch, B):
    """ft_rnn_xcd_fill_pct probes the form the launch would take (8 rows at B = 20 / 32): a whole group per XCD slot,
    16 one-workgroup CUs of 32, in either form -- the same share the 16-row form reports"""
    from forwardtacotron_amd import _lib
    L = _lib.lib()
    monkeypatch.setenv('FT_RNN_MB', '16')
    f16 = [L.ft_rnn_xcd_fill_pct(3, bwd, B, 841, HD) for bwd in (0, 1)]
    monkeypatch.delenv('FT_RNN_MB', raising=False)
    f = [L.ft_rnn_xcd_fill_pct(3, bwd, B, 841, HD) for bwd in (0, 1)]
    assert f == f16 == [50, 50]
