"""The launch plan of the GEMMs (csrc/ft_gemm_plan.h) without a GPU: which kernel, tile, split count and grid a rows
(NT / NN) or TN (weight-gradient) launch gets.  The header has no C entry point of its own: the stand-alone
tests/cpp/gemm_plan_main.cpp holds it to a hand-written table, built here with the host sanitizers.  The scratch sizes the
library answers through its host-only workspace queries are held to the numbers recorded before the planner moved into
the header: the same split counts the table has."""
import os
import subprocess

import pytest

# (rows, in_f, out_f) -> slabs of in_f x out_f floats ft_linear_bwd_weight_workspace asks for: the larger of the aligned
# and the unaligned plan's row splits (the query does not know the operands' alignment)
TN_SPLITS = [(9001, 516, 1000, 12), (2001, 1100, 1000, 8), (9001, 516, 1001, 12), (9001, 518, 1000, 12),
             (2001, 1100, 1001, 8), (17 * 529, 516, 1000, 12), (4 * 501, 1100, 1000, 8), (333, 36, 132, 3),
             (130, 257, 66, 2), (333, 10, 7, 3), (4096, 256, 512, 16), (26912, 256, 256, 32), (4096, 512, 2048, 8),
             (100, 80, 80, 1), (26912, 80, 256, 61), (26912, 512, 2048, 8),
             (200, 1022, 1021, 2), (5000, 516, 1000, 4), (2000, 8192, 128, 8), (4096, 8192, 64, 4),
             # both sides of the planner's thresholds (tests/cpp/gemm_plan_main.cpp, test_tn_boundaries)
             (8192, 1024, 512, 16), (8191, 1024, 512, 4), (8191, 512, 1024, 4), (7168, 1024, 516, 12),
             (5120, 2176, 384, 3), (1, 80, 80, 1), (128, 80, 80, 1), (129, 80, 80, 2), (3840, 512, 2048, 8),
             (4096, 64, 8192, 4), (4096, 4672, 64, 8), (4096, 4096, 4096, 1), (17408, 768, 640, 17),
             (532591, 516, 1000, 12)]
# (tasks, rows, in_f, out_f) -> slabs of rows x in_f floats ft_linear_bwd_data_multi_workspace asks for: the split-K
# ranges of the chained data gradient, 0 = not split
ROWS_SPLITS = [(2, 4096, 512, 2048, 4), (1, 4096, 512, 2048, 4), (2, 128, 512, 2048, 8), (2, 4100, 100, 2048, 8),
               (2, 4100, 132, 2048, 7), (2, 4096, 256, 768, 0), (2, 26912, 512, 2048, 0), (2, 200, 132, 2052, 8),
               (2, 4096, 132, 2052, 8), (2, 128, 512, 8192, 16), (1, 256, 256, 16384, 16),
               # both sides of the split-K thresholds (test_rows_boundaries)
               (1, 4096, 512, 2032, 0), (1, 4096, 512, 2036, 4), (2, 65, 512, 2048, 8), (2, 64, 512, 2048, 0),
               (2, 4096, 68, 2048, 8), (2, 4096, 64, 2048, 0), (2, 4096, 510, 2048, 0), (2, 8192, 512, 2048, 2),
               (2, 8256, 512, 2048, 0), (2, 4096, 516, 2048, 3), (1, 128, 512, 4112, 8)]


def test_plan_table_switches_and_invariants_in_a_sanitized_host_program(tmp_path):
    """tests/cpp/gemm_plan_main.cpp includes nothing but csrc/ft_gemm_plan.h: plain C++, built by the library's compiler
    for the host only with the address and undefined-behaviour sanitizers, warnings as errors"""
    from forwardtacotron_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f'{build.HIPCC}: no compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'gemm_plan_main')
    # -Xarch_host: the sanitizers are for this host program alone, never for code built for a GPU
    cc = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-I', build.CSRC,
                         os.path.join(root, 'tests', 'cpp', 'gemm_plan_main.cpp'), '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


@pytest.mark.parametrize('rows,in_f,out_f,S', TN_SPLITS)
def test_weight_gradient_workspace_is_the_recorded_split(rows, in_f, out_f, S):
    from forwardtacotron_amd import _lib
    assert _lib.lib().ft_linear_bwd_weight_workspace(rows, in_f, out_f) == 4 * S * in_f * out_f


@pytest.mark.parametrize('n,rows,in_f,out_f,S', ROWS_SPLITS)
def test_chained_data_gradient_workspace_is_the_recorded_split(n, rows, in_f, out_f, S):
    from forwardtacotron_amd import _lib
    assert _lib.lib().ft_linear_bwd_data_multi_workspace(n, rows, in_f, out_f, None) == 4 * S * rows * in_f


def test_the_other_workspace_queries_are_the_recorded_splits():
    """padded-row batched TN, a 5-tap convolution's and the postnet conv bank's weight gradients (benchmark shapes)"""
    from forwardtacotron_amd import _lib
    L = _lib.lib()
    assert L.ft_bgemm_tn_workspace(1001, 518, 9001, 1, 1) == 4 * 12 * 1001 * 518
    assert L.ft_bgemm_tn_workspace(1001, 1102, 2001, 1, 1) == 4 * 8 * 1001 * 1102
    assert L.ft_bgemm_tn_workspace(65, 2048, 16384, 1, 1) == 4 * 32 * 65 * 2048
    assert L.ft_bgemm_tn_workspace(64, 2048, 16384, 1, 1) == 4 * 16 * 64 * 2048
    assert L.ft_conv1d_bwd_weight_workspace(32, 841, 512, 512, 5, 841) == 4 * 7 * 5 * 512 * 512
    assert L.ft_conv1d_bwd_weight_workspace(32, 841, 80, 512, 5, 841) == 4 * 25 * 5 * 80 * 512
    assert L.ft_conv_bank_bwd_weight_workspace(32, 841, 80, 256, 8, 842) == 4 * 29 * 8 * (8 * 256) * 80
    assert L.ft_conv_bank_bwd_weight_workspace(32, 128, 256, 128, 16, 129) == 4 * 8 * 16 * (16 * 128) * 256
