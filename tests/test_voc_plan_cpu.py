"""The launch plan of the GAN vocoders (csrc/ft_voc_plan.h) without a GPU.  The stand-alone tests/cpp/voc_plan_main.cpp
holds the header to a hand-written table -- tile rows for every width, LDS bytes and threads per arrangement, the limits,
the fused-pair rule, the grids -- built here with the host sanitizers.  The library's host-only queries
(ft_melgan_tile_rows, ft_hifigan_tile_rows, ft_voc_plan) are held to the same rows, limits and pair rule, and so is
what Python exposes of them."""
import os
import subprocess

import pytest

# kind -> [(widest width, rows per tile)], ascending; widths are multiples of 8 from 8; every other width is 0
ROWS = {'conv_in': [(128, 64)], 'upsample': [(128, 128), (512, 64)], 'residual': [(32, 128), (256, 64)],
        'conv_out': [(32, 250)], 'respair': [(64, 128)]}
LIMITS = {0: 11, 1: 40, 2: 25}      # ft_voc_plan field -> value: residual taps, resconv halo, respair halo


def table_rows(kind, c):
    if c < 8 or c % 8:
        return 0
    return next((rows for upto, rows in ROWS[kind] if c <= upto), 0)


def test_plan_table_in_a_sanitized_host_program(tmp_path):
    """tests/cpp/voc_plan_main.cpp includes nothing but csrc/ft_voc_plan.h: plain C++, built by the library's compiler
    for the host only with the address and undefined-behaviour sanitizers, warnings as errors"""
    from forwardtacotron_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f'{build.HIPCC}: no compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'voc_plan_main')
    # -Xarch_host: the sanitizers are for this host program alone, never for code built for a GPU
    cc = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-I', build.CSRC,
                         os.path.join(root, 'tests', 'cpp', 'voc_plan_main.cpp'), '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


@pytest.mark.parametrize('family,kinds', [('melgan', ('conv_in', 'upsample', 'residual', 'conv_out')),
                                          ('hifigan', ('conv_in', 'upsample', 'residual', 'conv_out', 'respair'))])
def test_tile_rows_queries_answer_the_table_for_every_width(family, kinds):
    from forwardtacotron_amd import _lib
    for kind, name in enumerate(kinds):
        got = [_lib.query(f'ft_{family}_tile_rows', kind, c) for c in range(0, 521)]
        assert got == [table_rows(name, c) for c in range(0, 521)], (family, name)
    for kind in (-1, len(kinds), 6, 99):                        # no such kind (MelGAN has no fused pair)
        assert all(_lib.query(f'ft_{family}_tile_rows', kind, c) == 0 for c in (8, 32, 64))


def test_wrappers_take_the_kind_by_name():
    from forwardtacotron_amd import hip as H
    assert H.melgan_tile_rows('resblock', 256) == 64 and H.melgan_tile_rows('resblock', 32) == 128
    assert H.hifigan_tile_rows('resconv', 256) == 64 and H.hifigan_tile_rows('respair', 64) == 128
    assert H.hifigan_tile_rows('respair', 72) == 0 and H.melgan_tile_rows('conv_out', 32) == 250


def test_plan_query_answers_the_limits():
    from forwardtacotron_amd import _lib
    for field, value in LIMITS.items():
        assert _lib.query('ft_voc_plan', field, 0, 0, 0) == value, field
    assert _lib.query('ft_voc_plan', 4, 0, 0, 0) == -1 and _lib.query('ft_voc_plan', -1, 0, 0, 0) == -1


def test_python_takes_its_limits_and_the_pair_rule_from_the_plan():
    from forwardtacotron_amd import hifigan as M
    from forwardtacotron_amd import hip as H
    assert (M.MAX_KERNEL, M.MAX_HALO, H.HIFIGAN_MAX_HALO, H.HIFIGAN_PAIR_HALO) == (11, 40, 40, 25)
    assert M.pair_is_fused is H.hifigan_pair_is_fused
    H._pair_plan.clear()                                        # every answer below comes from the library
    for width in (8, 32, 40, 64, 72, 128):
        for k in (1, 3, 7, 11):
            for d in (1, 3, 5, 12, 13):
                want = False if k < 3 or d * (k - 1) // 2 > 25 else width <= 32 or (width <= 64 and k == 3)
                got = M.pair_is_fused(width, k, d)
                assert got is want, (width, k, d)
