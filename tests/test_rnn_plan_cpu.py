"""The launch plan of the persistent recurrences (csrc/ft_rnn_plan.h, queried through ft_rnn_plan) against the hand-written
table of tests/rnn_forms_table.py, without a GPU: the kernel instantiation, threads, rows, chunks, groups and workgroups of
every (G, H) and switch set the GPU suite runs, at more batch sizes than it can afford, and the layout the launch takes
on 256 CUs.  The admission arithmetic, the aligned layout's rotor and the workspace carve have no C entry point: the
stand-alone tests/cpp/rnn_plan_main.cpp checks them, built here with the host sanitizers."""
import os
import subprocess

import pytest

from rnn_forms_table import DEFAULT, HANDOFF, HANDOFF_WIDTHS, VARIANTS, expect, forms_of, has_granules, spread_only

BATCHES = (3, 5, 9, 16, 17, 21, 32, 33, 40, 64)
T = 12
ENVS = [(G, H, {}) for (G, H) in DEFAULT] + [(G, H, env) for (G, H, env, _, _) in VARIANTS] + \
    [(G, H, env) for (env, _) in HANDOFF.values() for (G, H) in HANDOFF_WIDTHS]


def set_env(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith('FT_RNN_')]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def check_plan(form, G, H, B, nd, backward, env):
    """ft_rnn_plan against expect(); the layout rule on 256 CUs with the occupancies tests/rnn_forms_table.py documents:
    2 workgroups per CU for the 4-wave forward kernels, 1 for every 8- and 16-wave one"""
    from forwardtacotron_amd import _lib, hip
    what = (G, H, B, nd, backward, env)
    plan, exp = hip.rnn_plan(G, backward, B, T, H, nd), expect(form, nd, B, env)
    assert plan is not None, what
    got = dict(tag=plan['tag'], block=plan['threads'], nchunks=plan['nchunks'], rows=plan['rows'], groups=plan['groups'],
               total=plan['total'])
    assert got == {k: exp[k] for k in got}, what
    assert plan['kind'] == plan['tag'].split('<')[0] and plan['granules'] == has_granules(plan['tag']), (what, plan)
    per_cu = 2 if not backward and plan['threads'] == 256 else 1
    aligned_applies = plan['nchunks'] <= 64 and not spread_only(env)
    assert plan['aligned'] == (plan['nchunks'] * -(-plan['groups'] // 8) if aligned_applies else 0), (what, plan)
    assert plan['spread'] == -(-plan['total'] // 8), (what, plan)
    layout = 'aligned' if aligned_applies and plan['aligned'] <= 32 * per_cu else 'spread'
    admitted = plan[layout] <= 32 * per_cu
    assert admitted == exp['admitted'], (what, plan, layout)
    if admitted:
        assert layout == exp['layout'], (what, plan)
    assert _lib.lib().ft_rnn_workspace(G, B, H) >= plan['workspace'] > 0, (what, plan)


@pytest.mark.parametrize('G,H,env', ENVS, ids=[f'{G}-{H}-' + (','.join(f'{k[7:]}={v}' for k, v in e.items()) or 'default')
                                               for (G, H, e) in ENVS])
def test_plan_gives_the_form_the_table_expects(G, H, env, monkeypatch):
    set_env(monkeypatch, env)
    fwd, bwd = forms_of(G, H, env)
    for B in BATCHES:
        check_plan(fwd, G, H, B, 2, False, env)
        check_plan(bwd, G, H, B, 2, True, env)


@pytest.mark.parametrize('switch', ['default'] + list(HANDOFF))
def test_plan_of_the_one_direction_lstm_512(switch, monkeypatch):
    env = HANDOFF.get(switch, ({}, True))[0]
    set_env(monkeypatch, env)
    for B in BATCHES:
        check_plan(forms_of(4, 512, env)[0], 4, 512, B, 1, False, env)


def test_shapes_the_persistent_form_refuses_plan_as_per_step(monkeypatch):
    from forwardtacotron_amd import _lib, hip
    set_env(monkeypatch, {})
    for G in (3, 4):
        for backward in (False, True):
            assert hip.rnn_plan(G, backward, 4, 12, 12) is None             # H % 16 != 0
            assert hip.rnn_plan(G, backward, 21, 12, 72) is None
            assert hip.rnn_plan(G, backward, 21, 1, 64) is None             # T < 2
            assert hip.rnn_plan(G, backward, 21, 2, 64) is not None
    old = _lib.lib().ft_rnn_set_persistent(0)
    try:
        assert hip.rnn_plan(4, False, 32, 12, 512) is None                  # switched off: per-step kernels
    finally:
        _lib.lib().ft_rnn_set_persistent(old)


def test_admission_layout_and_carve_in_a_sanitized_host_program(tmp_path):
    """tests/cpp/rnn_plan_main.cpp includes nothing but csrc/ft_rnn_plan.h: plain C++, built by the library's compiler for
    the host only with the address and undefined-behaviour sanitizers, warnings as errors"""
    from forwardtacotron_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip(f'{build.HIPCC}: no compiler')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'rnn_plan_main')
    # -Xarch_host: the sanitizers are for this host program alone, never for code built for a GPU
    cc = subprocess.run([build.HIPCC, '-x', 'c++', '-std=c++17', '-Wall', '-Werror',
                         '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                         '-I', build.CSRC,
                         os.path.join(root, 'tests', 'cpp', 'rnn_plan_main.cpp'), '-o', exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
