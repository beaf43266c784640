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
import pytest
import torch

import melgan_cpu as R
import vocoder_contract as VC

pytestmark = pytest.mark.gpu

LENS = [23, 1, 2, 7]
HOP = 256
TANH_ULPS = 4 * R.U            # tanhf: within 2 ulp of a value of magnitude <= 1, plus the rounding of its argument's last bit


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


# ---- 3. the contract shared with the HiFi-GAN vocoder (tests/vocoder_contract.py) ---------------------------------------
def test_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case):
    VC.check_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case, R.int16_of)


def test_inference_is_item_0_of_inference_batch(case):
    VC.check_inference_is_item_0_of_inference_batch(case)


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


def test_items_are_bit_identical_alone_and_at_any_position(case):
    VC.check_items_are_bit_identical_alone_and_at_any_position(case)


def test_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, monkeypatch):
    from forwardtacotron_amd import melgan as M
    VC.check_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, M, monkeypatch)


def test_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case):
    VC.check_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case)


def test_autograd_is_refused(narrow):
    VC.check_autograd_is_refused(narrow)


def test_weights_are_repacked_when_a_parameter_changes(narrow):
    from forwardtacotron_amd.melgan import MelGAN
    VC.check_weights_are_repacked_when_a_parameter_changes(narrow, lambda: MelGAN(**R.NARROW),
                                                           lambda voc: voc.generator[16].weight_g)


def test_generate_batch_output_goes_straight_in(narrow):
    VC.check_generate_batch_output_goes_straight_in(narrow, 8, R.int16_of)
