"""CPU: what of HiFiGAN.matmul_dtype = 'fp16' needs no device -- the launch plan of the fp16-operand residual
convolution (csrc/ft_voc_plan_h16.h) against a hand-written table, in a sanitized stand-alone host program and through
the library's query; the fp16 weight pack against fold_weight_norm(v, g).half() element for element; the property; and
the CPU emulation of the mode (tests/hifigan_fp16_cpu.py), which with its rounding switched off is the float64
definition."""
import os
import subprocess

import numpy as np
import pytest
import torch

import hifigan_cpu as R
import hifigan_fp16_cpu as E
from forwardtacotron_amd import hifigan as M
from forwardtacotron_amd._lib import FtError
from forwardtacotron_amd.gan_vocoder import fold_weight_norm

# widest width -> (rows per tile, threads, static LDS bytes): (rows + 80) x (width + 8) halves x 2 bytes, by hand
PLAN = [(32, (128, 256, 16640)), (64, (64, 256, 20736)), (128, (64, 256, 39168)), (256, (64, 512, 76032))]
LDS_OF_A_CU = 160 * 1024


def _plan(c):
    if c < 8 or c % 8:
        return None
    return next(((upto,) + row for upto, row in PLAN if c <= upto), None)


def test_plan_table_in_a_sanitized_host_program(tmp_path):
    """tests/cpp/voc_plan_h16_main.cpp includes nothing but csrc/ft_voc_plan_h16.h (and through it ft_voc_plan.h): plain
    C++, built for the host only with the address and undefined-behaviour sanitizers, warnings as errors"""
    from forwardtacotron_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f'{build.HIPCC}: no compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'voc_plan_h16_main')
    cc = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-I', build.CSRC,
                         os.path.join(root, 'tests', 'cpp', 'voc_plan_h16_main.cpp'), '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


def test_the_plan_query_answers_the_table_for_every_width():
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd import hip as H
    for c in range(0, 281):
        row = _plan(c)
        got = [_lib.query('ft_hifigan_h16_plan', f, c) for f in range(5)]
        want = [0] * 5 if row is None else [row[1], row[3], row[2], row[0], -(-c // 16) * 16]
        assert got == want, c
    assert _lib.query('ft_hifigan_h16_plan', 5, 64) == -1 and _lib.query('ft_hifigan_h16_plan', -1, 64) == -1
    assert all(row[2] <= LDS_OF_A_CU for _, row in PLAN)
    assert H.hifigan_h16_plan('lds_bytes', 256) == 76032 <= LDS_OF_A_CU // 2      # two 256-channel workgroups on a CU
    assert H.hifigan_h16_plan('tile_rows', 256) == H.hifigan_tile_rows('resconv', 256) == 64
    assert H.hifigan_h16_plan('cpad', 8) == 16 and H.hifigan_h16_plan('cpad', 24) == 32
    # the fp32 plan answers as before
    assert _lib.query('ft_voc_plan', 4, 0, 0, 0) == -1 and H.hifigan_tile_rows('resconv', 32) == 128


@pytest.mark.parametrize('k', [1, 3, 7, 11])
@pytest.mark.parametrize('width', [8, 16, 24, 32, 256])
def test_the_fp16_pack_is_the_folded_weight_in_half_element_for_element(k, width):
    torch.manual_seed(1000 * k + width)
    voc = M.HiFiGAN.v2()
    conv = M._conv(width, k, 1)
    with torch.no_grad():
        conv.weight_g.mul_(torch.rand_like(conv.weight_g) + 0.5)
        pack, bias = voc._panel_h16(conv)
        want = fold_weight_norm(conv.weight_v, conv.weight_g).half().numpy()
    cpad, CP = -(-width // 16) * 16, -(-width // 32) * 32
    assert pack.dtype == torch.float16 and tuple(pack.shape) == (k, cpad // 8, CP, 8) and pack.is_contiguous()
    w, rest = E.unpack_h16(pack.numpy(), width, width)
    assert w.shape == want.shape and np.array_equal(w.view(np.uint16), want.view(np.uint16))
    assert not rest.view(np.uint16).any()                                      # padded rows and columns: exact (+0) zeros
    assert bias.dtype == torch.float32 and bias.numel() == CP and torch.equal(bias[:width], conv.bias) and not bias[width:].any()
    assert voc._panel_h16(conv)[0] is pack                                     # cached under its own key ...
    assert voc._panel(conv)[0].dtype == torch.float32 and voc._panel_h16(conv)[0] is pack      # ... beside the fp32 pack
    with torch.no_grad():
        conv.weight_g.mul_(2.0)
        assert voc._panel_h16(conv)[0] is not pack                             # rebuilt for a new parameter version


def test_a_weight_beyond_fp16_is_refused_at_pack_time():
    voc = M.HiFiGAN.v2()
    conv = M._conv(16, 3, 1)
    with torch.no_grad():
        w = fold_weight_norm(conv.weight_v, conv.weight_g)
        conv.weight_g[3] *= 1e5 / float(w[3].abs().max())                      # one folded weight of 1e5
        assert float(fold_weight_norm(conv.weight_v, conv.weight_g).abs().max()) == pytest.approx(1e5, rel=1e-5)
        with pytest.raises(FtError, match='finite in fp16'):
            voc._panel_h16(conv)
        voc._panel(conv)                                                       # fp32 mode takes it


def test_the_property_its_default_its_refusals_and_the_state_dict():
    voc = M.HiFiGAN.v2().eval()
    assert voc.matmul_dtype == 'fp32'
    keys = list(voc.state_dict())
    for bad in ('bf16', 'FP16', None, 16):
        with pytest.raises(FtError, match='matmul_dtype'):
            voc.matmul_dtype = bad
    assert voc.matmul_dtype == 'fp32'
    voc.matmul_dtype = 'fp16'
    assert voc.matmul_dtype == 'fp16' and list(voc.state_dict()) == keys
    assert M.HiFiGAN.v2().matmul_dtype == 'fp32'                               # per object
    ok, lens = torch.zeros(2, 80, 5), torch.tensor([5, 3])
    with torch.no_grad():
        for mode in ('fp16', 'fp32'):                                          # a CPU-placed model: the device error
            voc.matmul_dtype = mode
            with pytest.raises(FtError, match='HIP'):
                voc.inference_batch(ok, lens)
            with pytest.raises(FtError, match='HIP'):
                voc.forward(ok)


@pytest.mark.parametrize('name', ['narrow', 'rb2'])
def test_the_emulation_without_rounding_is_the_float64_definition(name):
    cfg = R.PRESETS[name]
    ref = R.build(3, torch.float64, **cfg)
    for n in (1, 5):
        mel = R.make_mels([n], 80, n)[1][0]
        with torch.no_grad():
            want = ref.stages(mel.double())[2]
            got = E.emulate(ref, mel, rounding=False)
            rounded = E.emulate(ref, mel)
        assert got.shape == want.shape == (256 * n,)
        assert float((got - want).abs().max()) <= 1e-13
        err = float((rounded - want).abs().max())
        print(f'{name}, {n} frames: max |fp16 emulation - float64| {err:.3e}, wav std {float(want.std()):.3e}')
        assert 0.0 < err < 0.05 * float(want.std())                            # the rounding is on, and it is small


def test_the_operand_rule_saturates_keeps_nan_and_zero():
    x = torch.tensor([0.0, -0.0, 7e4, -8e5, 3.0e38, float('inf'), float('nan'), 65519.9, -1.0, 2.0 ** -20])
    a = E.operand(x)
    assert a[0] == 0 and a[1] == 0 and a[2] == 65504 and a[3] == -65504 and a[4] == 65504 and a[5] == 65504
    assert torch.isnan(a[6]) and a[7] == 65504 and a[8] == pytest.approx(-0.1, rel=2.0 ** -11) and a[9] == 2.0 ** -20
    assert torch.isfinite(a[[0, 1, 2, 3, 4, 5, 7, 8, 9]]).all()
