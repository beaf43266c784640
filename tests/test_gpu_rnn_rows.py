"""Rows per workgroup of the 512-wide LSTM's persistent forward and reduce-scatter BPTT: where the 16-row grid would
leave XCD slots idle (B = 32: 4 groups on 8 slots), 8 rows per workgroup give one group per slot.  The 8-row form only
moves batch rows between workgroups -- same k blocks per wave, same reduction orders -- so its results must equal the
16-row form's (FT_RNN_MB=16) bit for bit, and every 8-row group must still hand over XCD-local."""
import pytest
import torch

pytestmark = pytest.mark.gpu

HD = 512


def _lstm_inputs(B, T, seed, ragged):
    g = torch.Generator().manual_seed(seed)
    xp = (torch.randn(T, B, 8 * HD, generator=g) * 0.5).cuda()
    whh = [(torch.randn(4 * HD, HD, generator=g) * 0.05).cuda() for _ in range(2)]
    bhh = [(torch.randn(4 * HD, generator=g) * 0.1).cuda() for _ in range(2)]
    dout = (torch.randn(T, B, 2 * HD, generator=g) * 0.1).cuda()
    lens = None
    if ragged:
        lens = torch.randint(1, T + 1, (B,), generator=g)
        lens[B // 2] = T
        lens = lens.cuda()
    return xp, whh, bhh, dout, lens


def _run(monkeypatch, mb, B, T, seed, ragged):
    """(forward out, cell states, saved gates, BPTT d(pre-activations), groups XCD-local / agent-scope, launches)"""
    from forwardtacotron_amd import hip as H
    xp, whh, bhh, dout, lens = _lstm_inputs(B, T, seed, ragged)
    wt = [H.transpose2d(w) for w in whh]
    monkeypatch.setenv('FT_RNN_MB', str(mb))
    m0, c0 = H.rnn_mode_counts(), H.rnn_counters()
    raw, cst, gates = H.lstm_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], lens, HD, True)
    dg = H.lstm_bwd(dout, raw, cst, gates, wt[0], wt[1], lens, HD)
    torch.cuda.synchronize()
    H.check_rnn_status()
    m1, c1 = H.rnn_mode_counts(), H.rnn_counters()
    modes = (m1[0] - m0[0], m1[1] - m0[1])
    launches = (c1[0] - c0[0], c1[1] - c0[1])
    return raw.cpu(), cst.cpu(), gates.cpu(), dg.cpu(), modes, launches


@pytest.mark.parametrize('B,T,ragged,groups8', [
    (32, 841, True, 8),       # the benchmark's decoder LSTM
    (32, 37, False, 8),
    (21, 29, True, 6),        # B % 8 != 0: the last 8-row group is partly padding
    (9, 23, False, 4),        # one row in the second 8-row group
    (9, 23, True, 4),
])
def test_lstm_eight_rows_bit_equal_to_sixteen(monkeypatch, B, T, ragged, groups8):
    r16 = _run(monkeypatch, 16, B, T, 1000 + B + T, ragged)
    r8 = _run(monkeypatch, 8, B, T, 1000 + B + T, ragged)
    lens = _lstm_inputs(B, T, 1000 + B + T, ragged)[4]
    tmask = torch.zeros(T, B, dtype=torch.bool) if lens is None else torch.arange(T)[:, None] >= lens.cpu()[None, :]
    for name, a, b in zip(('out', 'cst', 'gates', 'd(pre-activations)'), r8[:4], r16[:4]):
        if name == 'gates':             # saved activations are written at t < length only (the rest is never read)
            a, b = a[~tmask], b[~tmask]
        assert torch.equal(a, b), f'{name}: 8-row form differs from the 16-row form'
    assert r8[5] == (2, 0) and r16[5] == (2, 0), 'forward and BPTT must both run persistent'
    groups16 = 2 * ((B + 15) // 16)
    # every (direction, batch group) group of both launches ran on the XCD-local hand-off
    assert r16[4] == (2 * groups16, 0)
    assert r8[4] == (2 * groups8, 0)
    if ragged:
        assert float(r8[0][tmask].abs().max()) == 0.0 and float(r8[3][tmask].abs().max()) == 0.0


@pytest.mark.parametrize('B,T,launches,refused,groups', [
    (64, 17, 1, 0, 8),        # 4 groups of 16 rows per direction already fill the 8 slots: stays 16 rows
    # long-form inference: the whole batch does not fit one grid (one refusal, as before), then two 64-row slices run
    # persistent, 16 rows each
    (128, 9, 2, 1, 16),
])
def test_full_batches_stay_on_sixteen_rows_and_persistent(monkeypatch, B, T, launches, refused, groups):
    from forwardtacotron_amd import hip as H
    xp, whh, bhh, _, lens = _lstm_inputs(B, T, 77 + B, True)
    monkeypatch.delenv('FT_RNN_MB', raising=False)
    m0, c0 = H.rnn_mode_counts(), H.rnn_counters()
    H.lstm_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], lens, HD, True)
    torch.cuda.synchronize()
    H.check_rnn_status()
    m1, c1 = H.rnn_mode_counts(), H.rnn_counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (launches, refused), 'persistent launches / refusals'
    assert (m1[0] - m0[0], m1[1] - m0[1]) == (groups, 0), '16-row groups, all XCD-local'
