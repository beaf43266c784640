"""The plan of the column reductions and of the scratch sizes around them (csrc/ft_reduce_plan.h) without a GPU.  The
header has no C entry point of its own: the stand-alone tests/cpp/reduce_plan_main.cpp holds it to a hand-written table and
to the conditions every composed size must meet, built here with the host sanitizers.  The library's host-only workspace
queries are held to the answers recorded before the sizes moved into the header, on the benchmark's shapes, the tests'
shapes and both sides of every threshold."""
import os
import subprocess

import pytest

# (B, Tbuf, C) -> ft_bn_workspace: 16 bytes per chunk and column
BN_WS = [((32, 841, 512), 524288), ((32, 841, 256), 262144), ((32, 841, 80), 81920), ((32, 842, 2048), 1048576),
         ((32, 129, 2048), 1048576), ((32, 128, 256), 262144), ((32, 128, 128), 131072), ((32, 128, 512), 524288),
         ((32, 841, 128), 131072), ((16, 620, 384), 393216), ((5, 13, 64), 2048), ((1, 1, 64), 1024), ((3, 70, 64), 4096),
         ((7, 59, 64), 7168), ((9, 61, 64), 9216), ((27, 161, 64), 65536), ((3, 70, 70), 4480), ((4, 12, 16), 256),
         ((4, 13, 64), 1024), ((3, 14, 16), 256), ((2, 2, 8), 128), ((5, 41, 64), 4096), ((4, 9, 12), 192), ((1, 1, 1), 16),
         ((1, 64, 63), 1008), ((1, 65, 65), 2080), ((1, 4096, 4096), 1048576), ((1, 4097, 4096), 1048576),
         ((1, 1024, 1024), 262144), ((1, 1025, 1088), 295936), ((1, 960, 64), 15360), ((1, 961, 64), 16384),
         ((1, 4096, 64), 65536), ((1, 4097, 64), 62464), ((1, 16384, 1), 1024), ((1, 128, 256), 8192),
         ((1, 129, 256), 12288), ((2, 500000, 4), 4096)]
# the same shapes -> ft_conv_stats_workspace: the larger of the chunk partials and one partial per 128-row GEMM tile
CONV_STATS_WS = [((32, 841, 512), 1728512), ((32, 841, 256), 864256), ((32, 841, 80), 270080), ((32, 842, 2048), 6914048),
                 ((32, 129, 2048), 1081344), ((32, 128, 256), 262144), ((32, 128, 128), 131072), ((32, 128, 512), 524288),
                 ((32, 841, 128), 432128), ((16, 620, 384), 479232), ((5, 13, 64), 2048), ((1, 1, 64), 1024),
                 ((3, 70, 64), 4096), ((7, 59, 64), 7168), ((9, 61, 64), 9216), ((27, 161, 64), 65536), ((3, 70, 70), 4480),
                 ((4, 12, 16), 256), ((4, 13, 64), 1024), ((3, 14, 16), 256), ((2, 2, 8), 128), ((5, 41, 64), 4096),
                 ((4, 9, 12), 192), ((1, 1, 1), 16), ((1, 64, 63), 1008), ((1, 65, 65), 2080), ((1, 4096, 4096), 2097152),
                 ((1, 4097, 4096), 2162688), ((1, 1024, 1024), 262144), ((1, 1025, 1088), 295936), ((1, 960, 64), 15360),
                 ((1, 961, 64), 16384), ((1, 4096, 64), 65536), ((1, 4097, 64), 62464), ((1, 16384, 1), 2048),
                 ((1, 128, 256), 8192), ((1, 129, 256), 12288), ((2, 500000, 4), 500032)]
# (rows, C) -> ft_colsum_workspace
COLSUM_WS = [((26912, 512), 524288), ((26912, 256), 262144), ((26912, 80), 81920), ((26912, 1536), 1032192),
             ((4096, 256), 262144), ((4096, 768), 786432), ((4096, 1024), 1048576), ((4096, 384), 393216),
             ((4096, 1536), 1007616), ((4096, 3), 3072), ((0, 5), 80), ((5, 0), 16), ((0, 0), 16), ((1, 1), 16),
             ((64, 64), 1024), ((65, 64), 2048), ((128, 65), 2080), ((4097, 4096), 1048576), ((1048576, 1), 1024),
             ((4128, 512), 499712), ((333, 36), 3456), ((130, 257), 12336), ((64, 128), 2048), ((64, 192), 3072),
             ((961, 32768), 8388608), ((961, 64), 16384), ((961, 192), 49152)]
# (B, Tout, Cout, k) -> ft_conv1d_fwd_stats_workspace: the statistics partials (256-byte aligned) + k tap slabs where the
# taps run as independent tasks (row tiles x column tiles < 192 <= tiles x k, 2 <= k <= 16, Cout > 64, Cout % 4 == 0)
CONV_FWD_STATS_WS = [((32, 128, 256, 3), 12845056), ((32, 128, 256, 2), 262144), ((32, 128, 256, 5), 21233664),
                     ((32, 128, 256, 1), 262144), ((32, 128, 256, 16), 67371008), ((32, 128, 256, 17), 262144),
                     ((32, 128, 4096, 3), 2097152), ((32, 128, 768, 3), 786432), ((32, 128, 640, 3), 32112640),
                     ((32, 841, 512, 5), 1728512), ((32, 841, 80, 5), 270080), ((32, 128, 64, 3), 65536),
                     ((32, 128, 68, 3), 69632), ((32, 128, 68, 6), 6754304), ((32, 128, 258, 3), 264192),
                     ((1, 64, 256, 16), 4096), ((1, 65, 256, 16), 8192), ((3, 65, 256, 16), 16384),
                     ((32, 128, 512, 3), 25690112), ((32, 128, 128, 5), 131072), ((32, 128, 128, 6), 12713984),
                     ((4, 12, 16, 5), 256), ((4, 13, 16, 4), 256), ((5, 13, 64, 3), 2048), ((27, 161, 64, 3), 65536)]
# (B, T, Cin, K) -> ft_conv_bank_bwd_data_workspace: K per-member partials under the same thresholds, else nothing
BANK_BWD_DATA_WS = [((32, 128, 256, 16), 67108864), ((32, 841, 80, 8), 0), ((32, 841, 512, 8), 0), ((32, 128, 256, 2), 0),
                    ((32, 128, 256, 3), 12582912), ((32, 128, 64, 16), 0), ((32, 128, 68, 16), 17825792),
                    ((32, 128, 768, 2), 0), ((32, 128, 640, 2), 20971520), ((1, 64, 256, 16), 0), ((1, 65, 256, 16), 0),
                    ((3, 65, 256, 16), 0), ((2, 64, 256, 16), 0), ((4, 12, 16, 4), 0), ((32, 128, 256, 1), 0),
                    ((32, 128, 128, 6), 12582912), ((32, 128, 128, 5), 0)]
# (B, T, d, dfft) -> ft_fft_block_sums_workspace
FFT_SUMS_WS = [((32, 128, 256, 1024), 3407872), ((32, 841, 256, 1024), 3407872), ((32, 128, 384, 1536), 4362240),
               ((32, 841, 384, 1536), 4423680), ((16, 128, 128, 256), 720896), ((2, 37, 128, 256), 45056),
               ((2, 37, 64, 128), 22528), ((1, 64, 64, 128), 11264), ((1, 1, 64, 64), 10240), ((3, 50, 256, 512), 135168),
               ((1, 1024, 64, 4096), 1196032), ((1, 960, 64, 32768), 8002560), ((1, 961, 64, 32768), 8536064),
               ((1, 961, 64, 32704), 8519680), ((1, 961, 64, 32708), 8520704), ((1, 1024, 64, 32768), 8536064),
               ((1, 1024, 128, 32768), 8683520), ((1, 2048, 64, 32768), 8683520), ((1, 1024, 64, 65536), 16924672),
               ((1, 4096, 64, 32768), 8978432), ((4, 300, 128, 512), 505856)]
# (B, T, d, dfft, k1, k2) -> ft_fft_block_wgrad_workspace where the four weight-gradient slab sets are the larger term:
# unchanged
FFT_WGRAD_WS = [((32, 128, 256, 1024, 9, 1), 37748736), ((32, 841, 256, 1024, 9, 1), 37748736),
                ((32, 128, 384, 1536, 3, 3), 35389440), ((32, 841, 384, 1536, 3, 3), 35389440),
                ((16, 128, 128, 256, 3, 3), 6291456), ((2, 37, 128, 256, 3, 3), 393216), ((2, 37, 64, 128, 3, 1), 98304),
                ((1, 64, 64, 128, 1, 1), 49152), ((1, 64, 64, 128, 3, 3), 98304), ((1, 1, 64, 64, 1, 1), 49152),
                ((3, 50, 256, 512, 9, 1), 9437184), ((1, 1024, 64, 4096, 1, 1), 8388608),
                ((1, 960, 64, 32768, 1, 1), 8388608), ((1, 961, 64, 32704, 1, 1), 16744448),
                ((1, 1024, 64, 32768, 3, 1), 25165824), ((1, 1024, 128, 32768, 1, 1), 33554432),
                ((4, 300, 128, 512, 3, 3), 7864320)]
# ... and where the batched column sums are: shape -> (the slabs alone, as the query answered before; the answer now =
# ft_fft_block_sums_workspace of the shape).  With no sums workspace ft_fft_blocks_bwd runs the sums in this buffer.
FFT_WGRAD_WS_GROWN = [((1, 961, 64, 32768, 1, 1), 8388608, 8536064), ((1, 961, 64, 32708, 1, 1), 8373248, 8520704),
                      ((1, 1024, 64, 32768, 1, 1), 8388608, 8536064), ((1, 2048, 64, 32768, 1, 1), 8388608, 8683520),
                      ((1, 1024, 64, 65536, 1, 1), 16777216, 16924672), ((1, 4096, 64, 32768, 1, 1), 8388608, 8978432)]

RECORDED = [(name, shape, nbytes) for name, table in (
    ('ft_bn_workspace', BN_WS), ('ft_conv_stats_workspace', CONV_STATS_WS), ('ft_colsum_workspace', COLSUM_WS),
    ('ft_conv1d_fwd_stats_workspace', CONV_FWD_STATS_WS), ('ft_conv_bank_bwd_data_workspace', BANK_BWD_DATA_WS),
    ('ft_fft_block_sums_workspace', FFT_SUMS_WS), ('ft_fft_block_wgrad_workspace', FFT_WGRAD_WS))
    for shape, nbytes in table]


def test_plan_table_and_composed_sizes_in_a_sanitized_host_program(tmp_path):
    """tests/cpp/reduce_plan_main.cpp includes nothing but csrc/ft_reduce_plan.h: plain C++, built by the library's
    compiler for the host only with the address and undefined-behaviour sanitizers, warnings as errors"""
    from forwardtacotron_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f'{build.HIPCC}: no compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'reduce_plan_main')
    # -Xarch_host: the sanitizers are for this host program alone, never for code built for a GPU
    cc = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-I', build.CSRC,
                         os.path.join(root, 'tests', 'cpp', 'reduce_plan_main.cpp'), '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr


@pytest.mark.parametrize('name,shape,nbytes', RECORDED)
def test_workspace_query_is_the_recorded_size(name, shape, nbytes):
    from forwardtacotron_amd import _lib
    assert _lib.query(name, *shape) == nbytes


@pytest.mark.parametrize('shape,slabs,sums', FFT_WGRAD_WS_GROWN)
def test_fft_block_wgrad_workspace_covers_the_column_sums(shape, slabs, sums):
    """the one intended change of an answer: where the batched sums need more than the weight-gradient slabs, the query
    answers the sums' size (it answered `slabs`, and a call without a sums workspace failed)"""
    from forwardtacotron_amd import _lib
    assert slabs < sums == _lib.query('ft_fft_block_sums_workspace', *shape[:4])
    assert _lib.query('ft_fft_block_wgrad_workspace', *shape) == sums
