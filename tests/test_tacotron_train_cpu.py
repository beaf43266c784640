"""CPU: (a) the float64 training-mode restatement tests/taco_train_cpu.py against the reference model itself, run in
train() with torch.nn.functional.dropout and Decoder.zoneout replaced by functions that apply the same supplied masks
(tests/golden/make_golden_tacotron_train.run_reference; needs a checkout of the reference, FT_REFERENCE, and is skipped
without one); (b) the refusals of Tacotron.forward_train / forward that need no GPU.

(a) Both sides are float64 over ~1e4 operations: loss and outputs must agree to 1e-10 absolute, every parameter
gradient and every BatchNorm running statistic to 1e-9 of its OWN scale (three orders over rounding)."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import taco_train_cpu as TT  # noqa: E402
from make_golden_tacotron import TINY, make_batch  # noqa: E402

REF = os.environ.get('FT_REFERENCE', '/root/reference')

CASES = {
    'tiny-r3': dict(cfg=TINY, r=3, seed=1, x_len=[9, 12, 6], mel_len=[20, 27, 14]),
    'tiny-spk16-r2': dict(cfg=dict(TINY, speaker_emb_dim=16), r=2, seed=2, x_len=[7, 11, 10], mel_len=[25, 16, 30]),
    'tiny-r1-long': dict(cfg=TINY, r=1, seed=3, x_len=[33, 70, 40], mel_len=[120, 90, 100]),
}


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_equals_reference_in_training_mode(name):
    if not os.path.isfile(os.path.join(REF, 'models', 'tacotron.py')):
        pytest.skip('no reference checkout (FT_REFERENCE)')
    import make_golden_tacotron_train as G
    ref_mod = G.import_reference(REF)
    c = CASES[name]
    cfg, r = c['cfg'], c['r']
    batch = make_batch(c['x_len'], c['mel_len'], r, cfg['speaker_emb_dim'], 40 + len(name))
    seeds, probs = G.site_seeds(c['seed']), G.site_probs(cfg)
    masks = G.case_masks(cfg, r, batch, seeds, probs)
    assert set(masks) == set(TT.SITE_MASKS.values())
    for k, m in masks.items():                      # every site is really on
        assert 0 < float((m == 0).double().mean()) < 1, k
    ref, loss_r, m1_r, m2_r, attn_r = G.run_reference(ref_mod, cfg, r, c['seed'], batch, masks, torch.float64)
    assert int(ref.step) == 1

    torch.manual_seed(c['seed'])
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        init = ref_mod.Tacotron(**cfg).state_dict()                 # the weights the reference started from
    finally:
        torch.set_default_dtype(old)
    P = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and 'running_' not in k and v.dim() > 0 and
             k != 'stop_threshold' else v.clone()) for k, v in init.items()}
    tb = {k: torch.as_tensor(v) for k, v in batch.items()}
    m1, m2, attn, stats = TT.forward(P, tb, cfg, r, masks)
    mel = tb['mel'].double()
    loss = torch.nn.functional.l1_loss(m1, mel) + torch.nn.functional.l1_loss(m2, mel)
    loss.backward()

    assert abs(float(loss.detach()) - float(loss_r)) <= 1e-10
    for a, b, what in ((m1, m1_r, 'mel_outputs'), (m2, m2_r, 'linear'), (attn, attn_r, 'attn_scores')):
        assert a.shape == b.shape, what
        assert float((a.detach() - b).abs().max()) <= 1e-10, what
    worst = (0.0, None)
    for k, p in ref.named_parameters():
        g_ref = p.grad if p.grad is not None else torch.zeros_like(p)
        g = P[k].grad if P[k].grad is not None else torch.zeros_like(P[k])
        scale = float(g_ref.abs().max())
        err = float((g - g_ref).abs().max())
        assert err <= 1e-9 * scale, (k, err, scale)
        if scale > 0:
            worst = max(worst, (err / scale, k))
    print(name, "loss", float(loss.detach()), 'worst gradient error / own scale', worst)
    sd = ref.state_dict()
    n_stats = 0
    for k, v in stats.items():
        assert float((v - sd[k]).abs().max()) <= 1e-9 * float(sd[k].abs().max()), k
        assert float((sd[k] - init[k]).abs().max()) > 0, k                     # the step moved it
        n_stats += 1
    assert n_stats == sum(1 for k in sd if 'running_' in k)
    # the rows of mel_proj that the [:, :, :r] slice drops get exact zeros
    gm = P['decoder.mel_proj.weight'].grad.view(80, TT.MAX_R, -1)
    assert not bool(gm[:, r:].any()) and bool(gm[:, :r].any())


def _tiny_model():
    from forwardtacotron_amd.tacotron import Tacotron
    torch.manual_seed(1)
    return Tacotron(**TINY)


def _tiny_batch():
    b = make_batch([9, 12, 6], [20, 27, 14], 1, 0, 5)
    return {'x': torch.from_numpy(b['x']), 'mel': torch.from_numpy(b['mel'])}


def test_forward_train_refuses_eval_mode_and_cpu():
    from forwardtacotron_amd.tacotron import FtError
    m = _tiny_model()
    assert m.zoneout == 0.1 and 'zoneout' not in m.state_dict() and m.last_seeds == {}
    m.eval()
    with pytest.raises(FtError, match='eval mode'):
        m.forward_train(_tiny_batch())
    m.train()
    m.decoder.prenet.eval()                              # one module in eval mode is enough
    with pytest.raises(FtError, match='decoder.prenet is in eval mode'):
        m.forward_train(_tiny_batch())
    m.train()
    with pytest.raises(FtError, match='HIP'):            # a CPU model
        m.forward_train(_tiny_batch())
    assert int(m.step) == 0                              # a refused call leaves no trace


def test_forward_still_refuses_training_mode():
    from forwardtacotron_amd.tacotron import FtError
    m = _tiny_model()
    m.train()
    with pytest.raises(FtError, match='training the teacher') as e:
        m(_tiny_batch())
    assert 'forward_train' in str(e.value)
    with pytest.raises(FtError, match='training the teacher'):
        m.align(_tiny_batch())
