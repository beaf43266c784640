"""The contract of a GAN vocoder's inference_batch (gan_vocoder.GanVocoder), stated once for melgan.MelGAN and
hifigan.HiFiGAN.  A vocoder's GPU test file keeps its own `Case`

    case.voc, case.mel [B, n_mels, Tmax], case.mel_len, case.lens, case.out (inference_batch of the batch, on the host),
    case.ref32 / case.ref64 (the stock-torch restatement), case.run(mel, mel_len)

and its tests call the checks below with it.  `int16_of` is the restatement's quantisation; `module` the vocoder's own
module, whose `_empty` the poison allocator replaces."""
import numpy as np
import pytest
import torch

from poison import poison

HOP = 256


def check_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case, int16_of):
    assert case.out['wav_int16'].dtype == torch.int16
    assert torch.equal(case.out['wav_int16'], int16_of(case.out['wav']))


def check_inference_is_item_0_of_inference_batch(case):
    n = case.lens[0]
    with torch.no_grad():
        got = case.voc.inference(case.mel[0:1, :, :n].cuda())
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == (HOP * n,)
    assert np.array_equal(got, case.out['wav_int16'][0, :HOP * n].numpy())


def check_items_are_bit_identical_alone_and_at_any_position(case):
    order = [2, 0, 3, 1]
    mel = torch.stack([case.mel[i] for i in order]).cuda()
    out = case.run(mel, torch.tensor([case.lens[i] for i in order]))
    for pos, i in enumerate(order):
        n = case.lens[i]
        assert torch.equal(out['wav'][pos, :HOP * n].cpu(), case.out['wav'][i, :HOP * n]), i
        alone = case.run(case.mel[i:i + 1, :, :n].cuda(), torch.tensor([n]))
        assert alone['wav'].shape == (1, HOP * n)
        assert torch.equal(alone['wav'][0].cpu(), case.out['wav'][i, :HOP * n]), i
        assert torch.equal(alone['wav_int16'][0].cpu(), case.out['wav_int16'][i, :HOP * n]), i


def check_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, module, monkeypatch):
    """every buffer of the call (HiFi-GAN: the averaging buffers and the chain's temporaries among them) starts as NaN"""
    monkeypatch.setattr(module, '_empty', poison)
    mel = case.mel.clone()
    for b, n in enumerate(case.lens):
        mel[b, :, n:] = float('nan') if b % 2 else float('inf')
    mel[2] = float('nan')                                   # a whole NaN item
    out = {k: v.cpu() for k, v in case.run(mel.cuda(), case.mel_len).items()}
    for b, n in enumerate(case.lens):
        assert not out['wav'][b, HOP * n:].any() and not out['wav_int16'][b, HOP * n:].any(), b     # exactly 0, NaN is not
        if b != 2:
            assert torch.equal(out['wav'][b], case.out['wav'][b]) and torch.equal(out['wav_int16'][b], case.out['wav_int16'][b])
    assert torch.isnan(out['wav'][2, :HOP * case.lens[2]]).all()
    assert not case.out['wav'][0, HOP * case.lens[0]:].any()


def check_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case):
    from forwardtacotron_amd._lib import FtError
    mel = case.mel.cuda()
    out = case.run(mel, case.mel_len.cuda())
    assert torch.equal(out['wav'].cpu(), case.out['wav']) and torch.equal(out['wav_int16'].cpu(), case.out['wav_int16'])
    assert torch.equal(out['wav_len'].cpu(), case.out['wav_len'])
    for bad in ([23, 0, 2, 7], [24, 1, 2, 7], [23, 1, -5, 7], [23, 1, 2, 1 << 40]):
        with pytest.raises(FtError, match='mel_len must be in'):
            case.run(mel, torch.tensor(bad, dtype=torch.int64).cuda())
    torch.cuda.synchronize()
    again = case.run(mel, case.mel_len.cuda())               # the clamped runs indexed nothing out of bounds and broke nothing
    assert torch.equal(again['wav'].cpu(), case.out['wav'])


def check_autograd_is_refused(case):
    from forwardtacotron_amd._lib import FtError
    with pytest.raises(FtError, match='no autograd'):
        case.voc.inference_batch(case.mel.cuda(), case.mel_len)


def check_weights_are_repacked_when_a_parameter_changes(case, make, weight_g):
    """make(): a fresh vocoder of the case's configuration; weight_g(voc): a weight_g that reaches the output"""
    voc = make()
    voc.load_state_dict(case.ref32.state_dict())
    voc = voc.cuda().eval()
    mel = case.mel.cuda()
    with torch.no_grad():
        a = voc.inference_batch(mel, case.mel_len)['wav'].cpu()
        packs = {k: v[1] for k, v in voc._packs.items()}
        b = voc.inference_batch(mel, case.mel_len)['wav'].cpu()
        assert all(voc._packs[k][1] is v for k, v in packs.items())          # folded once, not per call
        weight_g(voc).mul_(0.5)
        c = voc.inference_batch(mel, case.mel_len)['wav'].cpu()
    assert torch.equal(a, case.out['wav']) and torch.equal(a, b) and not torch.equal(a, c)


def check_generate_batch_output_goes_straight_in(case, n_mels, int16_of):
    from forwardtacotron_amd import hip
    from forwardtacotron_amd.model import ForwardTacotron
    from helpers import TINY
    torch.manual_seed(4)
    m = ForwardTacotron(**dict(TINY, n_mels=n_mels)).cuda().eval()
    x_len = torch.tensor([9, 4, 12])
    x = torch.randint(1, 100, (3, 12))
    for b, n in enumerate(x_len):
        x[b, n:] = 0
    with torch.no_grad():
        gen = m.generate_batch(x.cuda(), x_len)
        out = case.voc.inference_batch(gen['mel_post'], gen['mel_len'])
    torch.cuda.synchronize()
    hip.check_rnn_status()
    mel, mel_len = gen['mel_post'].cpu(), gen['mel_len'].cpu()
    assert out['wav'].shape == (3, HOP * mel.shape[2]) and torch.equal(out['wav_len'].cpu(), HOP * mel_len)
    assert torch.equal(out['wav_int16'].cpu(), int16_of(out['wav'].cpu()))
    e_gpu = e_cpu = 0.0
    for b, n in enumerate(mel_len.tolist()):
        with torch.no_grad():
            want = case.ref64.stages(mel[b, :, :n].double())[2]
            ref = case.ref32.stages(mel[b, :, :n])[2]
        e_gpu = max(e_gpu, float((out['wav'][b, :HOP * n].cpu().double() - want).abs().max()))
        e_cpu = max(e_cpu, float((ref.double() - want).abs().max()))
        assert not out['wav'][b, HOP * n:].any()
    print(f'mel_len {mel_len.tolist()}: max |err| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32, ratio {e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu
