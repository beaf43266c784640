"""GPU: HiFiGAN.matmul_dtype = 'fp16' (csrc/ft_hifigan_h16.hip) -- the kernel alone against float64 on its own rounded
operands, the saturating conversion, the end-to-end error against the CPU emulation of the mode
(tests/hifigan_fp16_cpu.py), the ragged contract in fp16 mode, and that the two modes are what they say.

Models, mels and lengths are those of tests/test_gpu_hifigan.py (its cases are shared, built once): `narrow` = V2, `full`
= V1, `rb2` = V3, mel_len = [23, 1, 2, 7], and the full-width item whose rows at the 8x stage end one frame past a tile
boundary.  V2 brings the widths 16 and 8, whose contraction is zero-padded to 16; 24 (padded to 32) is run on its own.

Bounds.  The kernel alone: |err| <= (K + 4) 2^-24 S + D per output (hifigan_fp16_cpu.resconv_h16_stage), K = k cpad the
padded contraction, S the absolute sum, D what a flush of fp16-subnormal operands could lose: a-priori, nothing measured.
The reference takes a from the kernel's own fp32 input by the mode's definition and w_h from the kernel's own pack
(tests/test_hifigan_fp16_cpu.py holds the pack to fold_weight_norm(v, g).half() element for element).  End to end: max |wav
- float64| is at most twice that of the CPU emulation of the mode.  Every comparison prints its figure before it asserts.

Measured on an MI355X (seed 0): DESIGN.md section 7, "HiFi-GAN vocoder", fp16 mode."""
import math

import numpy as np
import pytest
import torch

import hifigan_cpu as R
import hifigan_fp16_cpu as E
import test_gpu_hifigan as T
import vocoder_contract as VC

pytestmark = pytest.mark.gpu

LENS = T.LENS
HOP = 256


class H16Case:
    """a case of tests/test_gpu_hifigan.py (fixtures, float64 results and the fp32-mode run: shared, unchanged) with a
    second module of the same weights in fp16 mode and its result"""

    def __init__(self, base):
        from forwardtacotron_amd.hifigan import HiFiGAN
        self.base = base
        for k in ('name', 'cfg', 'lens', 'ref32', 'ref64', 'mel', 'items', 'mel_len', 'wav64'):
            setattr(self, k, getattr(base, k))
        self.voc = HiFiGAN(**self.cfg)
        self.voc.load_state_dict(self.ref32.state_dict())
        self.voc = self.voc.cuda().eval()
        self.voc.matmul_dtype = 'fp16'
        with torch.no_grad():
            out = self.voc.inference_batch(self.mel.cuda(), self.mel_len, keep_stages=True)
            torch.cuda.synchronize()
            self.out = {k: v.cpu() for k, v in out.items() if k != 'stages'}
            self.stages = [s.cpu() for s in out['stages']]
        self._emul = None

    def run(self, mel, mel_len, **kw):
        with torch.no_grad():
            return self.voc.inference_batch(mel, mel_len, **kw)

    item = T.Case.item

    @property
    def emul(self):
        if self._emul is None:
            with torch.no_grad():
                self._emul = [E.emulate(self.ref64, m) for m in self.items]
        return self._emul


_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = H16Case(T._case(name))
    return _cases[name]


@pytest.fixture(scope='module', params=['narrow', 'full', 'rb2'])
def case(request):
    return _case(request.param)


def _pack_weights(pack, C):
    """the kernel's own fp16 weights, from its pack on the device -> float64 [C, C, k]"""
    w, _ = E.unpack_h16(pack.cpu().numpy(), C, C)
    return torch.from_numpy(np.ascontiguousarray(w)).double()


def _ratio(got, want, bound):
    """worst |err| / bound over a tensor; a non-finite output counts as infinitely wrong"""
    if not torch.isfinite(got).all():
        return math.inf
    return float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())


def _items(buf, lens, scale):
    stride = max(lens) * scale
    return [buf[b * stride:b * stride + n * scale].T.contiguous() for b, n in enumerate(lens)]


_refs = {}       # (memo key, form, item) -> (want, bound): the 256-channel references, shared by tests 5 and 6


def _check_launch(run, x, lens, scale, d, w_h, bias64, prev, nk, worst, tag, memo=None):
    """one (k, d) at one width: the three res_modes with acc_mode 0, and the three acc_modes with a residual from
    memory, all rows of all items.  run(res, acc, out) launches and returns the output on the device.  memo: a key
    under which the float64 references are kept for the next caller with the same inputs."""
    other = torch.roll(x, 1, dims=1).contiguous()      # a residual that is not x (rows stay where they are)
    xs, os_, ps = _items(x.cpu(), lens, scale), _items(other.cpu(), lens, scale), _items(prev.cpu(), lens, scale)
    forms = [('no-res acc0', None, 0), ('own-res acc0', 'x', 0), ('mem-res acc0', other, 0), ('mem-res acc1', other, 1),
             ('mem-res acc2', other, 2)]
    for what, res, acc in forms:
        got = run(res, acc, prev.clone() if acc else None).cpu()
        for b, g in enumerate(_items(got, lens, scale)):
            r = None if res is None else xs[b] if isinstance(res, str) else os_[b]
            kw = {} if acc == 0 else dict(prev=ps[b]) if acc == 1 else dict(prev=ps[b], nk=nk, divide=True)
            if memo is None or (memo, what, b) not in _refs:
                ref = E.resconv_h16_stage(xs[b], d, w_h, bias64, res=r, **kw)
                if memo is not None:
                    _refs[(memo, what, b)] = ref
            want, bound = ref if memo is None else _refs[(memo, what, b)]
            key = f'{tag} {what}'
            worst[key] = max(worst.get(key, 0.0), _ratio(g, want, bound))


def _report(name, worst):
    for key, v in sorted(worst.items()):
        print(f'{name} {key}: worst |err| / bound {v:.3f}')
    top = max(worst.values())
    print(f'{name}: worst |err| / bound of all fp16 residual launches {top:.3f} over {len(worst)} kinds')
    assert top <= 1.0, (name, max(worst, key=worst.get), top)


# ---- 5. the kernel alone ----------------------------------------------------------------------------------------------
def _preset_launches(case, route, only_width=None):
    """_check_launch for every (k, d) of the preset (and dilation 1, ResBlock1's second convolution) at every stage
    width, on the stage's real input (the fp32-mode transposed convolution's output), all rows of all items.  route
    'fp16': ft_hifigan_resconv_h16 on the fp16 pack; 'fp32': ft_hifigan_resconv on the fp32 pack of the same
    convolution, held to the SAME references (the fp16 pack's weights)."""
    from forwardtacotron_amd import hip as H
    cfg, voc, base = case.cfg, case.voc, case.base
    nk, B, Tmax = len(cfg['resblock_kernel_sizes']), len(case.lens), max(case.lens)
    ml = case.mel_len.cuda()
    scale, worst = 1, {}
    with torch.no_grad():
        for i, s in enumerate(cfg['upsample_rates']):
            scale *= s
            xd, prev_d = base.dev_stages[2 * i + 1], base.dev_stages[2 * i + 2]
            C = xd.shape[1]
            if only_width and C != only_width:
                continue
            for j, (k, ds) in enumerate(zip(cfg['resblock_kernel_sizes'], cfg['resblock_dilation_sizes'])):
                blk = voc.resblocks[i * nk + j]
                convs = [(c, d) for c, d in zip(blk.convs, ds)] if cfg['resblock'] == '2' else \
                    [(c, d) for c, d in zip(blk.convs1, ds)] + [(blk.convs2[0], 1)]
                for n, (conv, d) in enumerate(convs):
                    w, bias = voc._panel_h16(conv)
                    w32, b32 = voc._panel(conv)

                    def run(res, acc, out):
                        a = (xd, ml, B, Tmax, scale, d)
                        kw = dict(res=res, acc_mode=acc, nk=nk, out=out)
                        return H.hifigan_resconv_h16(*a, w, bias, **kw) if route == 'fp16' else H.hifigan_resconv(*a, w32, b32, **kw)
                    _check_launch(run, xd, case.lens, scale, d, _pack_weights(w, C), conv.bias.detach().cpu().double(), prev_d,
                                  nk, worst, f'C{C} k{k} d{d}', memo=(case.name, i, j, n) if C == 256 else None)
    torch.cuda.synchronize()
    return worst


def test_the_fp16_residual_kernel_against_float64_on_its_own_rounded_operands(case):
    _report(case.name, _preset_launches(case, 'fp16'))


@pytest.mark.parametrize('C', [8, 16, 24])
def test_the_fp16_residual_kernel_at_widths_whose_contraction_is_zero_padded(C):
    """8 and 24 are padded to 16 and 32 in the tile and in the pack; 184 rows cross the 128-row tile of these widths.
    NaN behind every item and in the padding of the running sum must not reach a valid row."""
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd.hifigan import pack_taps_h16
    from forwardtacotron_amd.gan_vocoder import pack_bias
    gen = torch.Generator().manual_seed(C)
    B, Tmax, scale, nk = len(LENS), max(LENS), 8, 3
    x = torch.randn(B * Tmax * scale, C, generator=gen)
    prev = torch.randn(B * Tmax * scale, C, generator=gen)
    for b, n in enumerate(LENS):
        x[(b * Tmax + n) * scale:(b + 1) * Tmax * scale] = float('nan')
    xd, prev_d, ml = x.cuda(), prev.cuda(), torch.tensor(LENS).cuda()
    worst = {}
    for k, d in [(1, 1), (3, 1), (7, 3), (11, 5), (7, 12)]:
        w32 = torch.randn(C, C, k, generator=gen) / math.sqrt(k * C)
        b32 = torch.randn(C, generator=gen)
        w, bias = pack_taps_h16(w32.cuda()), pack_bias(b32.cuda())

        def run(res, acc, out):
            return H.hifigan_resconv_h16(xd, ml, B, Tmax, scale, d, w, bias, res=res, acc_mode=acc, nk=nk, out=out)
        _check_launch(run, xd, LENS, scale, d, w32.half().double(), b32.double(), prev_d, nk, worst, f'C{C} k{k} d{d}')
    torch.cuda.synchronize()
    _report(f'synthetic C{C}', worst)


# ---- 6. the check tells the routes apart ------------------------------------------------------------------------------
def test_the_same_check_fails_the_fp32_kernel_at_256_channels():
    """ft_hifigan_resconv's fp32 output on test 5's 256-channel inputs, held to test 5's references and bound, must
    FAIL: it lies about 2^-12 sqrt(sum (a w)^2) from the fp16-operand value.  The bound grows with K and that distance
    with sqrt(K), so the three-tap launches (K = 768) are the ones that separate the routes; the worst ratio per k is
    printed."""
    case = _case('full')
    w16 = _preset_launches(case, 'fp16', only_width=256)
    w32 = _preset_launches(case, 'fp32', only_width=256)
    assert w16.keys() == w32.keys() and len(w16) == 45                 # 3 k x 3 d x 5 forms
    for k in case.cfg['resblock_kernel_sizes']:
        print(f'C256 k{k}: worst |err| / bound {max(v for key, v in w16.items() if f" k{k} " in key):.3f} for the fp16 kernel, '
              f'{max(v for key, v in w32.items() if f" k{k} " in key):.2f} for the fp32 kernel')
    assert max(w16.values()) <= 1.0 < max(w32.values())


# ---- 7. saturation ----------------------------------------------------------------------------------------------------
def test_values_beyond_fp16_saturate_and_no_inf_appears():
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd.hifigan import pack_taps_h16
    from forwardtacotron_amd.gan_vocoder import pack_bias
    gen = torch.Generator().manual_seed(5)
    C, k, d, lens, scale = 32, 3, 2, [20, 3], 8
    B, Tmax = len(lens), max(lens)
    x = torch.randn(B * Tmax * scale, C, generator=gen)
    x[5, 3], x[70, 0], x[131, 31], x[Tmax * scale + 2, 7] = 7e4, -8e5, 3.0e38, 3.0e38      # 131: across the 128-row tile edge
    w32 = torch.randn(C, C, k, generator=gen) / math.sqrt(k * C)
    b32 = torch.randn(C, generator=gen)
    xd, ml = x.cuda(), torch.tensor(lens).cuda()
    w, bias = pack_taps_h16(w32.cuda()), pack_bias(b32.cuda())
    a = E.operand(x)
    assert a[5, 3] == 65504 and a[70, 0] == -65504 and a[131, 31] == 65504 and torch.isfinite(a).all()
    worst = {}
    for what, res in (('no-res', None), ('own-res', 'x')):
        got = H.hifigan_resconv_h16(xd, ml, B, Tmax, scale, d, w, bias, res=res).cpu()
        for b, (g, xi) in enumerate(zip(_items(got, lens, scale), _items(x, lens, scale))):
            assert torch.isfinite(g).all(), (what, b)                       # no Inf, no NaN anywhere in the output
            want, bound = E.resconv_h16_stage(xi, d, w32.half().double(), b32.double(), res=xi if res else None)
            worst[what] = max(worst.get(what, 0.0), _ratio(g, want, bound))
        # the saturated operands reached the rows around them: |out| there is of the order of 65504 |w|
        assert float(got[5 - d:5 + d + 1].abs().max()) > 1e3
    _report('saturation C32', worst)


def test_fp16_subnormal_operands():
    """one fp16-subnormal activation (2^-20) against a weight of 1, and a subnormal weight (2^-20) against an activation
    of 1: the MFMA KEEPS fp16 subnormal inputs (measured) -- the result is 2^-20, not 0"""
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd.hifigan import pack_taps_h16
    C = 16
    x = torch.zeros(8, C)
    x[3, 2], x[5, 4] = 2.0 ** -20, 1.0
    w32 = torch.zeros(C, C, 1)
    w32[0, 2, 0], w32[1, 4, 0] = 1.0, 2.0 ** -20
    got = H.hifigan_resconv_h16(x.cuda(), None, 1, 8, 1, 1, pack_taps_h16(w32.cuda()), torch.zeros(32).cuda()).cpu()
    print(f'subnormal activation x 1: {float(got[3, 0]):.6e}; 1 x subnormal weight: {float(got[5, 1]):.6e}; 2^-20 = {2.0 ** -20:.6e}')
    assert float(got[3, 0]) == 2.0 ** -20 and float(got[5, 1]) == 2.0 ** -20
    got[3, 0] = got[5, 1] = 0
    assert not got.any()


# ---- 8. end to end ----------------------------------------------------------------------------------------------------
def _end_to_end(case):
    valid = [(case.out['wav'][b, :HOP * n].double(), case.wav64[b], case.emul[b]) for b, n in enumerate(case.lens)]
    e_gpu = max(float((g - w).abs().max()) for g, w, _ in valid)
    e_emul = max(float((e - w).abs().max()) for _, w, e in valid)
    return e_gpu, e_emul


def test_end_to_end_within_twice_the_cpu_emulation_of_the_mode(case):
    assert torch.equal(case.out['wav_len'], HOP * case.mel_len)
    e_gpu, e_emul = _end_to_end(case)
    top = max(float(w.abs().max()) for w in case.wav64)
    std = float(torch.cat(case.wav64).std())
    print(f'{case.name} fp16 mode: max |wav - float64| {e_gpu:.3e} on the device, {e_emul:.3e} emulated on the CPU, ratio '
          f'{e_gpu / e_emul:.2f}; wav std {std:.3e} = {std / e_emul:.0f} x the emulation\'s error, max |wav| {top:.3f}')
    assert top < math.tanh(1.0)                      # the pre-tanh maximum is below 1: no saturated tanh hides an error
    assert std >= 100.0 * e_emul                     # the signal stands two orders of magnitude above the yardstick
    assert e_gpu <= 2.0 * e_emul


def test_an_item_one_frame_past_a_tile_boundary_at_the_8x_stage():
    from forwardtacotron_amd import hip as H
    tile = H.hifigan_h16_plan('tile_rows', R.V1['upsample_initial_channel'] // 2)
    assert tile >= 8 and tile % 8 == 0
    n = tile // 8 + 1
    assert (n * 8) % tile == 8
    c = H16Case(T.Case('full', [n]))
    e_gpu, e_emul = _end_to_end(c)
    print(f'tile {tile}, n {n}: max |wav - float64| {e_gpu:.3e} on the device, {e_emul:.3e} emulated, ratio {e_gpu / e_emul:.2f}')
    assert e_gpu <= 2.0 * e_emul


# ---- 9. the ragged contract in fp16 mode (tests/vocoder_contract.py) -----------------------------------------------------
def test_items_are_bit_identical_alone_and_at_any_position(case):
    VC.check_items_are_bit_identical_alone_and_at_any_position(case)


def test_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, monkeypatch):
    from forwardtacotron_amd import hifigan as M
    VC.check_nan_padding_a_nan_item_and_poisoned_buffers_change_nothing(case, M, monkeypatch)


def test_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case):
    VC.check_device_side_mel_len_gives_the_same_bits_and_reports_a_bad_length(case)


def test_int16_and_inference_in_fp16_mode(case):
    VC.check_int16_is_the_scale_clamp_and_truncate_of_the_returned_wav(case, R.int16_of)
    VC.check_inference_is_item_0_of_inference_batch(case)


# ---- 10. the modes are what they say -----------------------------------------------------------------------------------
def _valid_rows(case, stages):
    """the rows of every stage buffer that belong to an item (what lies behind an item is never written)"""
    scales = [1]
    for s in case.cfg['upsample_rates']:
        scales += [scales[-1] * s] * 2
    return [torch.cat(_items(buf.cpu(), case.lens, scale), dim=1) for buf, scale in zip(stages, scales)]


def test_fp32_mode_is_untouched_by_a_visit_to_fp16_mode(case):
    """one module: fp32, fp16, fp32 again.  The fp32 results are those of the untouched module of tests/test_gpu_hifigan.py
    bit for bit (no cached fp16 pack leaks), the fp16 result is this file's and differs, conv_pre's output is shared."""
    from forwardtacotron_amd.hifigan import HiFiGAN
    voc = HiFiGAN(**case.cfg)
    voc.load_state_dict(case.ref32.state_dict())
    voc = voc.cuda().eval()
    mel = case.mel.cuda()
    runs = []
    with torch.no_grad():
        for mode in ('fp32', 'fp16', 'fp32'):
            voc.matmul_dtype = mode
            out = voc.inference_batch(mel, case.mel_len, keep_stages=True)
            runs.append((out['wav'].cpu(), _valid_rows(case, out['stages'])))
    (a, sa), (h, sh), (c, sc) = runs
    assert torch.equal(a, case.base.out['wav']) and torch.equal(c, a)
    assert all(torch.equal(p, q) for p, q in zip(sa, sc)) and \
        all(torch.equal(p, q) for p, q in zip(sa, _valid_rows(case, case.base.stages)))
    assert torch.equal(h, case.out['wav']) and not torch.equal(h, a)
    assert torch.equal(sh[0], sa[0]) and torch.equal(sh[1], sa[1])             # conv_pre and the first transposed convolution
    assert not torch.equal(sh[2], sa[2])                                       # the first residual stage is where they part
    assert any(k[0] == 'h16' for k in voc._packs if isinstance(k, tuple)) and \
        all(v[1][0].dtype == torch.float32 for k, v in voc._packs.items() if not isinstance(k, tuple))
    valid = torch.cat([(h[b, :HOP * n] - a[b, :HOP * n]) for b, n in enumerate(case.lens)]).double()
    ref = torch.cat([a[b, :HOP * n] for b, n in enumerate(case.lens)]).double()
    print(f'{case.name}: max |wav_fp16 - wav_fp32| {float(valid.abs().max()):.3e}, SNR '
          f'{10 * math.log10(float(ref.pow(2).sum() / valid.pow(2).sum())):.1f} dB')
