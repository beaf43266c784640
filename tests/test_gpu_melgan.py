"""GPU: melgan.MelGAN (csrc/ft_melgan.hip) against the stock-torch restatement of tests/melgan_cpu.py, item by item.

Models: the narrow one (8 mels, channels (32, 16, 16, 8, 8)) and the full-width one, both with torch's default
initialisation under a seed (tests/test_melgan_cpu.py holds that fixture to an unsaturated tanh).  Lengths [23, 1, 2, 7]
in Tmax = 23: mel_len = 1 gives the shortest input (11 frames, 88 rows at the 8x stage, where the dilation-9 reflections
of both ends are closest), and one more full-width item is sized from the launch plan so that its rows at the 8x stage
end one frame past a tile boundary.

Bounds.  Each kernel alone: |err| <= (K + 4) 2^-24 sum |w| |x| per output, evaluated in float64 from the kernel's own
fp32 input (melgan_cpu.*_stage; for the fused block plus the first convolution's bound carried through the second):
a-priori, nothing measured.  End to end: the max abs error of wav against float64 is at most 2x that of the fp32
stock-torch CPU route on the same weights and mels.  Every comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

import melgan_cpu as R

pytestmark = pytest.mark.gpu

LENS = [23, 1, 2, 7]
HOP = 256
TANH_ULPS = 4 * R.U            # tanhf: within 2 ulp of a value of magnitude <= 1, plus the rounding of its argument's last bit


def _poison(*shape, dtype=torch.float32, device=None):
    t = torch.empty(*shape, dtype=dtype, device=device)
    return t.fill_(float('nan')) if dtype.is_floating_point else t.fill_(-12345)


class Case:
    """one model: the stock trees (fp32 and float64, same weights), the module on the device, the batch, its result with
    every stage kept, and the per-item oracle stages -- built once, never modified"""

    def __init__(self, name, lens=LENS):
        from forwardtacotron_amd.melgan import MelGAN
        self.cfg = cfg = R.FULL if name == 'full' else R.NARROW
        self.name, self.lens, self.C = name, list(lens), cfg['channels']
        self.ref32 = R.build(0, **cfg)
        self.ref64 = R.build(0, **cfg).double()
        self.voc = MelGAN(**cfg)
        self.voc.load_state_dict(self.ref32.state_dict())
        self.voc = self.voc.cuda().eval()
        self.mel, self.items = R.make_mels(self.lens, cfg['mel_channel'], 11)
        self.mel_len = torch.tensor(self.lens, dtype=torch.int64)
        with torch.no_grad():
            out = self.voc.inference_batch(self.mel.cuda(), self.mel_len, keep_stages=True)
            torch.cuda.synchronize()
            self.out = {k: v.cpu() for k, v in out.items() if k != 'stages'}
            self.stages = [s.cpu() for s in out['stages']]
            self.wav64 = [self.ref64.stages(m.double())[2] for m in self.items]
            self.wav32 = [self.ref32.stages(m)[2] for m in self.items]

    def run(self, mel, mel_len, **kw):
        with torch.no_grad():
            return self.voc.inference_batch(mel, mel_len, **kw)

    def stage_item(self, k, b, scale):
        """item b of kernel output k -> fp32 [C, L], L = (len + 10) * scale"""
        stride = (max(self.lens) + 10) * scale
        L = (self.lens[b] + 10) * scale
        return self.stages[k][b * stride:b * stride + L].T.contiguous()


_cases = {}


@pytest.fixture(scope='module', params=['narrow', 'full'])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


@pytest.fixture(scope='module')
def narrow():
    if 'narrow' not in _cases:
        _cases['narrow'] = Case('narrow')
    return _cases['narrow']


def _held(what, got, want, bound):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{what}: max |err| {float(err.max()):.3e}, worst |err| / bound {worst:.3f}')
    assert torch.isfinite(got).all() and worst <= 1.0, (what, worst)


# ---- 1. each kernel alone ---------------------------------------------------------------------------------------------
def test_each_kernel_against_the_float64_restatement_of_its_stage(case):
    """Every kernel's output for every item, ALL rows (first and last rows, both reflection ends, the three dilations
    and all phases of both transposed shapes are among them), from the fp32 input that kernel was given"""
    g = case.ref64.generator
    assert len(case.stages) == 17
    for b, n in enumerate(case.lens):
        w, bias = R.folded(g[1])
        want, bound = R.conv_in_stage(case.items[b], 10, w, bias)
        _held(f'{case.name} item {b} conv_in', case.stage_item(0, b, 1), want, bound)
        k, scale = 0, 1
        for i, (_, s, _) in enumerate(case.cfg['upsamples']):
            w, bias = R.folded(g[3 * i + 3])
            want, bound = R.upsample_stage(case.stage_item(k, b, scale), w, bias, s)
            k, scale = k + 1, scale * s
            _held(f'{case.name} item {b} upsample {i} (x{scale})', case.stage_item(k, b, scale), want, bound)
            stack = g[3 * i + 4]
            for j, d in enumerate((1, 3, 9)):
                ops = R.folded(stack.blocks[j][2]) + R.folded(stack.blocks[j][4]) + R.folded(stack.shortcuts[j])
                want, bound = R.resblock_stage(case.stage_item(k, b, scale), d, *ops)
                k += 1
                _held(f'{case.name} item {b} resblock {i}.{j} (d {d})', case.stage_item(k, b, scale), want, bound)
        w, bias = R.folded(g[16])
        pre, bound = R.conv_out_stage(case.stage_item(k, b, scale), w, bias)
        _held(f'{case.name} item {b} conv_out', case.out['wav'][b, :HOP * n], torch.tanh(pre)[:HOP * n], bound[:HOP * n] + TANH_ULPS)


# ---- 2. end to end ----------------------------------------------------------------------------------------------------
def _end_to_end(case):
    e_gpu = max(float((case.out['wav'][b, :HOP * n].double() - case.wav64[b]).abs().max()) for b, n in enumerate(case.lens))
    e_cpu = max(float((case.wav32[b].double() - case.wav64[b]).abs().max()) for b in range(len(case.lens)))
    return e_gpu, e_cpu


def test_end_to_end_within_twice_the_fp32_cpu_route(case):
    """Measured on an MI355X (seed 0): ratio 0.86 full width, 1.19 narrow (profiles/melgan.txt)"""
    assert torch.equal(case.out['wav_len'], HOP * case.mel_len)
    e_gpu, e_cpu = _end_to_end(case)
    print(f'{case.name}: max |wav - float64| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32 on the CPU, ratio '
          f'{e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu


def test_an_item_one_frame_past_a_tile_boundary_at_the_8x_stage():
    """full width, B = 1: (n + 10) * 8 rows at the 8x stage = a whole number of the plan's residual-block tiles + one
    frame's 8 rows (the tile is read from the plan)"""
    from forwardtacotron_amd import hip as H
    tile = H.melgan_tile_rows('resblock', R.FULL['channels'][1])
    assert tile >= 8 and tile % 8 == 0
    n = next(m * tile // 8 + 1 - 10 for m in range(1, 64) if m * tile // 8 + 1 - 10 >= 1)
    assert ((n + 10) * 8) % tile == 8
    c = Case('full', [n])
    e_gpu, e_cpu = _end_to_end(c)
    print(f'tile {tile}, n {n}: max |wav - float64| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32, ratio {e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu


# ---- 3. quantisation --------------------------------------------------------------------------------------------------
def test_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case):
    assert case.out['wav_int16'].dtype == torch.int16
    assert torch.equal(case.out['wav_int16'], R.int16_of(case.out['wav']))


def test_inference_is_item_0_of_inference_batch(case):
    n = case.lens[0]
    with torch.no_grad():
        got = case.voc.inference(case.mel[0:1, :, :n].cuda())
    assert isinstance(got, np.ndarray) and got.dtype == np.int16 and got.shape == (HOP * n,)
    assert np.array_equal(got, case.out['wav_int16'][0, :HOP * n].numpy())


def test_forward_is_the_generator_without_the_tail(narrow):
    m = narrow.items[0]
    with torch.no_grad():
        got = narrow.voc.forward(m.unsqueeze(0).cuda()).cpu()
        want = narrow.ref64.forward(m.double().unsqueeze(0))
        ref = narrow.ref32.forward(m.unsqueeze(0))
    assert got.shape == want.shape == (1, 1, HOP * m.shape[1])
    e_gpu, e_cpu = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
    print(f'forward: max |err| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32')
    assert e_gpu <= 2.0 * e_cpu


# ---- 4. bit-identical items -------------------------------------------------------------------------------------------
def test_items_are_bit_identical_alone_and_at_any_position(case):
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


# ---- 5. NaN isolation -------------------------------------------------------------------------------------------------
def test_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, monkeypatch):
    from forwardtacotron_amd import melgan as M
    monkeypatch.setattr(M, '_empty', _poison)
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


# ---- 6. device-side lengths -------------------------------------------------------------------------------------------
def test_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case):
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


def test_autograd_is_refused(narrow):
    from forwardtacotron_amd._lib import FtError
    with pytest.raises(FtError, match='no autograd'):
        narrow.voc.inference_batch(narrow.mel.cuda(), narrow.mel_len)


def test_weights_are_repacked_when_a_parameter_changes(narrow):
    from forwardtacotron_amd.melgan import MelGAN
    voc = MelGAN(**R.NARROW)
    voc.load_state_dict(narrow.ref32.state_dict())
    voc = voc.cuda().eval()
    mel = narrow.mel.cuda()
    with torch.no_grad():
        a = voc.inference_batch(mel, narrow.mel_len)['wav'].cpu()
        packs = {k: v[1] for k, v in voc._packs.items()}
        b = voc.inference_batch(mel, narrow.mel_len)['wav'].cpu()
        assert all(voc._packs[k][1] is v for k, v in packs.items())          # folded once, not per call
        voc.generator[16].weight_g.mul_(0.5)
        c = voc.inference_batch(mel, narrow.mel_len)['wav'].cpu()
    assert torch.equal(a, narrow.out['wav']) and torch.equal(a, b) and not torch.equal(a, c)


# ---- 7. the real producer ---------------------------------------------------------------------------------------------
def test_generate_batch_output_goes_straight_in(narrow):
    from forwardtacotron_amd import hip
    from forwardtacotron_amd.model import ForwardTacotron
    from helpers import TINY
    torch.manual_seed(4)
    m = ForwardTacotron(**dict(TINY, n_mels=8)).cuda().eval()
    x_len = torch.tensor([9, 4, 12])
    x = torch.randint(1, 100, (3, 12))
    for b, n in enumerate(x_len):
        x[b, n:] = 0
    with torch.no_grad():
        gen = m.generate_batch(x.cuda(), x_len)
        out = narrow.voc.inference_batch(gen['mel_post'], gen['mel_len'])
    torch.cuda.synchronize()
    hip.check_rnn_status()
    mel, mel_len = gen['mel_post'].cpu(), gen['mel_len'].cpu()
    assert out['wav'].shape == (3, HOP * mel.shape[2]) and torch.equal(out['wav_len'].cpu(), HOP * mel_len)
    assert torch.equal(out['wav_int16'].cpu(), R.int16_of(out['wav'].cpu()))
    e_gpu = e_cpu = 0.0
    for b, n in enumerate(mel_len.tolist()):
        with torch.no_grad():
            want = narrow.ref64.stages(mel[b, :, :n].double())[2]
            ref = narrow.ref32.stages(mel[b, :, :n])[2]
        e_gpu = max(e_gpu, float((out['wav'][b, :HOP * n].cpu().double() - want).abs().max()))
        e_cpu = max(e_cpu, float((ref.double() - want).abs().max()))
        assert not out['wav'][b, HOP * n:].any()
    print(f'mel_len {mel_len.tolist()}: max |err| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32, ratio {e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu
