"""GPU: hifigan.HiFiGAN (csrc/ft_hifigan.hip) against the stock-torch restatement of tests/hifigan_cpu.py, item by item.

Models: `narrow` = V2, `full` = V1, `rb2` = V3 (ResBlock2), torch's default initialisation under seed 0
(tests/test_hifigan_cpu.py holds these fixtures to an unsaturated tanh and a signal 1e4 times the tolerance).  Lengths
[23, 1, 2, 7] in Tmax = 23: one frame is 8 rows at the first stage, fewer than the 25- and 36-row halos of (k, d) = (11,
5) and (7, 12), so both zero edges fall inside one tile; 23 frames are 184 rows there, so real halos cross tile boundaries
at every stage.  One more full-width item is sized from the launch plan so that its rows at the 8x stage end one frame
past a tile boundary.

Bounds.  Each kernel alone: |err| <= (K + 4) 2^-24 sum |w| |x| per output, evaluated in float64 from the kernel's own
fp32 input (hifigan_cpu.*_stage; a residual counts inside the absolute sum, the first convolution's bound is carried
through the second for the fused pair, one rounding each for the running sum's addition and the division of the
averaging launches): a-priori, nothing measured.  End to end: the max abs error of wav against float64 is at most 2x that
of the fp32 stock-torch CPU route on the same weights and mels.  Every comparison prints its figure before it asserts.

Measured on an MI355X (seed 0): see DESIGN.md section 7, "HiFi-GAN vocoder", Accuracy."""
import pytest
import torch

import hifigan_cpu as R
import vocoder_contract as VC

pytestmark = pytest.mark.gpu

LENS = [23, 1, 2, 7]
HOP = 256
TANH_ULPS = 4 * R.U            # tanhf: within 2 ulp of a value of magnitude <= 1, plus the rounding of its argument's last bit


class Case:
    """one model: the stock trees (fp32 and float64, same weights), the module on the device, the batch, its result with
    every stage kept, and the per-item oracle -- built once, never modified"""

    def __init__(self, name, lens=LENS):
        from forwardtacotron_amd.hifigan import HiFiGAN
        self.cfg = cfg = R.PRESETS[name]
        self.name, self.lens = name, list(lens)
        self.ref32 = R.build(0, **cfg)
        self.ref64 = R.build(0, **cfg).double()
        self.voc = HiFiGAN(**cfg)
        self.voc.load_state_dict(self.ref32.state_dict())
        self.voc = self.voc.cuda().eval()
        self.mel, self.items = R.make_mels(self.lens, cfg['num_mels'], 11)
        self.mel_len = torch.tensor(self.lens, dtype=torch.int64)
        with torch.no_grad():
            out = self.voc.inference_batch(self.mel.cuda(), self.mel_len, keep_stages=True)
            torch.cuda.synchronize()
            self.out = {k: v.cpu() for k, v in out.items() if k != 'stages'}
            self.dev_stages = out['stages']
            self.stages = [s.cpu() for s in out['stages']]
            self.wav64 = [self.ref64.stages(m.double())[2] for m in self.items]
            self.wav32 = [self.ref32.stages(m)[2] for m in self.items]

    def run(self, mel, mel_len, **kw):
        with torch.no_grad():
            return self.voc.inference_batch(mel, mel_len, **kw)

    def item(self, buf, b, scale):
        """item b of a channels-last buffer at `scale` -> fp32 [C, L], L = len * scale"""
        stride = max(self.lens) * scale
        return buf[b * stride:b * stride + self.lens[b] * scale].T.contiguous()


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(scope='module', params=['narrow', 'full', 'rb2'])
def case(request):
    return _case(request.param)


@pytest.fixture(scope='module')
def narrow():
    return _case('narrow')


_worst = {}


def _held(what, got, want, bound, key=None):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    if key:
        _worst[key] = max(_worst.get(key, 0.0), worst)
    else:
        print(f'{what}: max |err| {float(err.max()):.3e}, worst |err| / bound {worst:.3f}')
    assert torch.isfinite(got).all() and worst <= 1.0, (what, worst)


# ---- 1. each kernel alone ---------------------------------------------------------------------------------------------
def test_the_chain_kernels_against_the_float64_restatement_of_their_stages(case):
    """conv_in, every transposed convolution and conv_out for every item, ALL rows (both zero edges, every phase of
    every transposed shape among them), from the fp32 input that kernel was given"""
    g, cfg = case.ref64, case.cfg
    assert len(case.stages) == 1 + 2 * len(cfg['upsample_rates'])
    for b, n in enumerate(case.lens):
        want, bound = R.conv_in_stage(case.items[b], *R.folded(g.conv_pre))
        _held(f'{case.name} item {b} conv_in', case.item(case.stages[0], b, 1), want, bound)
        scale = 1
        for i, s in enumerate(cfg['upsample_rates']):
            want, bound = R.upsample_stage(case.item(case.stages[2 * i], b, scale), *R.folded(g.ups[i]), s)
            scale *= s
            _held(f'{case.name} item {b} upsample {i} (x{scale})', case.item(case.stages[2 * i + 1], b, scale), want, bound)
        pre, bound = R.conv_out_stage(case.item(case.stages[-1], b, scale), *R.folded(g.conv_post))
        _held(f'{case.name} item {b} conv_out', case.out['wav'][b, :HOP * n], torch.tanh(pre), bound + TANH_ULPS)


def test_the_residual_kernels_against_float64_every_k_d_at_every_width(case):
    """Every (k, d) of the preset at every stage width, all rows of all items, each launch from its own fp32 input (the
    stage's transposed-convolution output): the residual convolution without a residual, with the tile's own rows, with
    a residual from memory; ResBlock1's fused pair wherever the kernel exists (whatever the plan picks); and on each
    block's last convolution the two accumulating forms of the averaging, onto a running sum given in memory."""
    from forwardtacotron_amd import hip as H
    g, cfg, voc = case.ref64, case.cfg, case.voc
    nk, B, Tmax = len(cfg['resblock_kernel_sizes']), len(case.lens), max(case.lens)
    ml = case.mel_len.cuda()
    scale = 1
    _worst.clear()

    def check(key, got, stage_fn, *args, **kw):
        got = got.cpu()
        for b in range(B):
            want, bound = stage_fn(*[case.item(a, b, scale) if isinstance(a, torch.Tensor) and a.dim() == 2 and
                                     a.shape[0] == B * Tmax * scale else a for a in args],
                                   **{k: case.item(v, b, scale) if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
            _held(f'{case.name} {key} item {b}', case.item(got, b, scale), want, bound, key=key)

    with torch.no_grad():
        for i, s in enumerate(cfg['upsample_rates']):
            scale *= s
            xd = case.dev_stages[2 * i + 1]
            x, C = case.stages[2 * i + 1], xd.shape[1]
            prev_d = case.dev_stages[2 * i + 2]                      # a running sum: the stage's own result serves
            prev = case.stages[2 * i + 2]
            a = (xd, ml, B, Tmax, scale)
            for j, (k, ds) in enumerate(zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes'])):
                blk64, blk = g.resblocks[i * nk + j], voc.resblocks[i * nk + j]
                for m, d in enumerate(ds):
                    tag = f'C{C} k{k} d{d}'
                    accs = [(0, {}), (1, dict(prev=prev)), (2, dict(prev=prev, nk=nk, divide=True))] if m == len(ds) - 1 \
                        else [(0, {})]
                    if cfg['resblock'] == '2':
                        w64, b64 = R.folded(blk64.convs[m])
                        w, bias = voc._panel(blk.convs[m])
                        for acc, kw in accs:
                            got = H.hifigan_resconv(*a, d, w, bias, res='x', acc_mode=acc, nk=nk,
                                                    out=prev_d.clone() if acc else None)
                            check(f'resconv own-res acc{acc} {tag}', got, R.resconv_stage, x, d, w64, b64, res=x, **kw)
                        continue
                    w1_64, b1_64 = R.folded(blk64.convs1[m])
                    w2_64, b2_64 = R.folded(blk64.convs2[m])
                    w1, b1 = voc._panel(blk.convs1[m])
                    w2, b2 = voc._panel(blk.convs2[m])
                    mid_d = H.hifigan_resconv(*a, d, w1, b1)
                    check(f'resconv no-res {tag}', mid_d, R.resconv_stage, x, d, w1_64, b1_64)
                    mid = mid_d.cpu()
                    for acc, kw in accs:
                        got = H.hifigan_resconv(mid_d, ml, B, Tmax, scale, 1, w2, b2, res=xd, acc_mode=acc, nk=nk,
                                                out=prev_d.clone() if acc else None)
                        check(f'resconv mem-res acc{acc} C{C} k{k} d1', got, R.resconv_stage, mid, 1, w2_64, b2_64, res=x, **kw)
                        if H.hifigan_tile_rows('respair', C):
                            got = H.hifigan_respair(*a, d, w1, b1, w2, b2, acc_mode=acc, nk=nk,
                                                    out=prev_d.clone() if acc else None)
                            check(f'respair acc{acc} {tag}', got, R.respair_stage, x, d, w1_64, b1_64, w2_64, b2_64, **kw)
    torch.cuda.synchronize()
    for key, worst in sorted(_worst.items()):
        print(f'{case.name} {key}: worst |err| / bound {worst:.3f}')
    print(f'{case.name}: worst of all residual launches {max(_worst.values()):.3f} over {len(_worst)} kinds')


# ---- 2. end to end ----------------------------------------------------------------------------------------------------
def _end_to_end(case):
    e_gpu = max(float((case.out['wav'][b, :HOP * n].double() - case.wav64[b]).abs().max()) for b, n in enumerate(case.lens))
    e_cpu = max(float((case.wav32[b].double() - case.wav64[b]).abs().max()) for b in range(len(case.lens)))
    return e_gpu, e_cpu


def test_end_to_end_within_twice_the_fp32_cpu_route(case):
    assert torch.equal(case.out['wav_len'], HOP * case.mel_len)
    e_gpu, e_cpu = _end_to_end(case)
    print(f'{case.name}: max |wav - float64| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32 on the CPU, ratio '
          f'{e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu


def test_an_item_one_frame_past_a_tile_boundary_at_the_8x_stage():
    """full width, B = 1: n * 8 rows at the 8x stage = a whole number of the plan's residual-convolution tiles + one
    frame's 8 rows (the tile is read from the plan)"""
    from forwardtacotron_amd import hip as H
    tile = H.hifigan_tile_rows('resconv', R.V1['upsample_initial_channel'] // 2)
    assert tile >= 8 and tile % 8 == 0
    n = tile // 8 + 1
    assert (n * 8) % tile == 8
    c = Case('full', [n])
    e_gpu, e_cpu = _end_to_end(c)
    print(f'tile {tile}, n {n}: max |wav - float64| {e_gpu:.3e} on the device, {e_cpu:.3e} stock fp32, ratio {e_gpu / e_cpu:.2f}')
    assert e_gpu <= 2.0 * e_cpu


# ---- 3. the contract shared with the MelGAN vocoder (tests/vocoder_contract.py) -----------------------------------------
def test_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case):
    VC.check_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case, R.int16_of)
    assert case.out['wav_int16'].any()


def test_inference_is_item_0_of_inference_batch(case):
    VC.check_inference_is_item_0_of_inference_batch(case)


def test_forward_is_the_batch_path_with_full_lengths(case):
    mel = torch.stack([case.items[0], case.items[0].flip(1)])            # two items of the full length
    with torch.no_grad():
        got = case.voc.forward(mel.cuda()).cpu()
        ref = case.run(mel.cuda(), torch.tensor([mel.shape[2]] * 2))['wav'].cpu()
    assert got.shape == (2, 1, HOP * mel.shape[2])
    assert torch.equal(got[:, 0], ref) and torch.equal(got[0, 0], case.out['wav'][0])


def test_items_are_bit_identical_alone_and_at_any_position(case):
    VC.check_items_are_bit_identical_alone_and_at_any_position(case)


def test_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, monkeypatch):
    from forwardtacotron_amd import hifigan as M
    VC.check_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, M, monkeypatch)


def test_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case):
    VC.check_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case)


def test_autograd_is_refused(narrow):
    VC.check_autograd_is_refused(narrow)


def test_weights_are_repacked_when_a_parameter_changes(narrow):
    from forwardtacotron_amd.hifigan import HiFiGAN
    VC.check_weights_are_repacked_when_a_parameter_changes(narrow, lambda: HiFiGAN(**R.V2),
                                                           lambda voc: voc.resblocks[7].convs2[1].weight_g)


def test_generate_batch_output_goes_straight_in(narrow):
    VC.check_generate_batch_output_goes_straight_in(narrow, 80, R.int16_of)
