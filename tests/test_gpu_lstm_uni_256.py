"""GPU: ft_lstm_fwd_uni at H = 256, one direction -- the form speaker.VoiceEncoder runs three times per chunk of partials
and that tests/rnn_forms_table.py (ft_lstm_fwd_uni 512 only) does not pin -- against tests/rnn_cpu.lstm_fwd_uni in float64,
at the tolerance tests/test_gpu_rnn_forms.py holds the 512 form to (rnn_cpu.FWD_TOL).  Shapes (H, B, T): one batch group
with idle rows, a group and a row, three groups at two steps, and the encoder's own 160 steps."""
import numpy as np
import pytest
import torch

import rnn_cpu as R

pytestmark = pytest.mark.gpu

SHAPES = [(256, 3, 9), (256, 9, 9), (256, 40, 2), (256, 8, 160)]


def _run(inp, H, B, T):
    from forwardtacotron_amd import hip as Hp
    xp = torch.from_numpy(np.array(inp['xp'], order='C')).cuda()
    whh = torch.from_numpy(np.array(inp['whh'][0], order='C')).cuda()
    bhh = torch.from_numpy(np.array(inp['bhh'][0], order='C')).cuda()
    try:
        out, cst = Hp.lstm_fwd_uni(xp, whh, bhh, H)
        torch.cuda.synchronize()
    finally:
        Hp.check_rnn_status()
    return out.cpu(), cst.cpu()


@pytest.mark.parametrize('H,B,T', SHAPES)
def test_one_direction_lstm_256_vs_float64(H, B, T):
    inp = R.rnn_inputs(4, B, T, H, 1, 0, False, False)
    want_out, want_cst = R.lstm_fwd_uni(inp['xp'], inp['whh'][0], inp['bhh'][0], H)
    out, cst = _run(inp, H, B, T)
    assert out.shape == (T, B, H) and cst.shape == (T, B, H)
    e_out = float(np.abs(out.double().numpy() - want_out).max())
    e_cst = float(np.abs(cst.double().numpy() - want_cst).max())
    print(f'ft_lstm_fwd_uni H={H} B={B} T={T}: out {e_out:.2e} cst {e_cst:.2e} (bound {R.FWD_TOL:.0e})')
    assert torch.isfinite(out).all() and torch.isfinite(cst).all()
    assert e_out <= R.FWD_TOL and e_cst <= R.FWD_TOL
    again = _run(inp, H, B, T)
    assert torch.equal(out, again[0]) and torch.equal(cst, again[1]), 'not repeatable bit for bit'
