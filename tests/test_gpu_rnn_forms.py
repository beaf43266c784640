"""Every form and hand-off of the persistent recurrences (csrc/ft_rnn_persist.hip) against float64.

Each case calls the primitives directly (hip.gru_fwd / gru_fwd_lens / gru_bwd, hip.lstm_fwd / lstm_bwd, ft_lstm_fwd_uni)
with one set of FT_RNN_* switches (read per launch), compares EVERY output with tests/rnn_cpu.py in float64, proves the
path taken -- launch counters, XCD-local / agent-scope group counts and the library's FT_RNN_DEBUG line, which names the
kernel instantiation, the layout and the hand-off -- and, where a switch only changes how values travel or where
workgroups sit, demands the default form's bits.  dout is random.  profiles/rnn_forms.txt is the record of one run.

The forms, their tags, layouts and switches: tests/rnn_forms_table.py (THE TABLE), shared with the CPU test of the plan.
A packed item of length 0 is admitted by every entry point (clamp_len: never active) and is part of every packed case."""
import os
import re

import numpy as np
import pytest
import torch

import rnn_cpu as R
from rnn_forms_table import HANDOFF, HANDOFF_WIDTHS, RS, VARIANTS, expect, forms_of, rows_per_wg

pytestmark = pytest.mark.gpu

GRAN4_BASE = {'FT_RNN_FWD_UB16': '0'}            # the form FT_RNN_GRAN4 addresses
GRAN4_ENVS = {g: dict(GRAN4_BASE, FT_RNN_GRAN4=g) for g in ('1', '0')}
HANDOFF_BT = [(21, 9, False), (33, 12, True), (5, 2, False)]
VARIANT_BT = [(21, 9, False), (33, 12, True), (5, 2, False), (5, 12, True)]

LINE = re.compile(r'\[ft_rnn\] (\w+<[-\d,]+>) block (\d+) total (\d+) nchunks (\d+): (\w+) layout, (\d+) workgroups per XCD '
                  r'slot, demand ([\d.]+) -> (\w+); hand-off ([\w-]+), cell (\w+)')
RECORD = []


@pytest.fixture(scope='module', autouse=True)
def record_file():
    """FT_RNN_FORMS_RECORD=<path>: write what this run observed (profiles/rnn_forms.txt is made from it)"""
    yield
    path = os.environ.get('FT_RNN_FORMS_RECORD')
    if path:
        with open(path, 'w') as f:
            f.write('\n'.join(RECORD) + '\n')


def cuda(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()  # (a C-contiguous copy: the shared inputs are read-only)


class Launches:
    """counter deltas and the debug lines around one entry-point call"""

    def __init__(self, capfd):
        from forwardtacotron_amd import hip as H
        self.H, self.capfd = H, capfd
        torch.cuda.synchronize()
        capfd.readouterr()
        self.c0, self.m0 = H.rnn_counters(), H.rnn_mode_counts()

    def done(self):
        torch.cuda.synchronize()
        c1, m1 = self.H.rnn_counters(), self.H.rnn_mode_counts()
        err = self.capfd.readouterr().err
        lines = [m.groups() for m in LINE.finditer(err)]
        assert len(lines) == err.count('[ft_rnn]'), err
        return dict(persistent=c1[0] - self.c0[0], refused=c1[1] - self.c0[1], local=m1[0] - self.m0[0],
                    agent=m1[1] - self.m0[1], lines=lines)


def check_path(obs, exp, T, persistent, what):
    if T < 2 or not persistent:                 # refused by the persistent form (a.T < 2) / switched off: per-step kernels
        assert obs['persistent'] == 0 and obs['lines'] == [] and (obs['local'], obs['agent']) == (0, 0), (what, obs)
        return 'per-step'
    if not exp['admitted']:
        # the grid does not fit the chip in either layout: ONE refused launch, no persistent one, no group ever counted,
        # every candidate line says so (the spread one last, with the form the dispatch picked); the per-step kernels ran
        assert obs['persistent'] == 0 and obs['refused'] == 1 and (obs['local'], obs['agent']) == (0, 0), (what, obs)
        assert obs['lines'] and all(ln[7] == 'refused' for ln in obs['lines']), (what, obs['lines'])
        tag, block, total, nchunks, layout, per, demand = obs['lines'][-1][:7]
        got = dict(tag=tag, block=int(block), total=int(total), nchunks=int(nchunks), layout=layout)
        want = dict({k: exp[k] for k in got}, layout='spread')
        assert got == want and float(demand) > 1.0, (what, got, want, demand)
        return f'{tag} block {block} nchunks {nchunks} total {total} spread demand {demand} REFUSED -> per-step'
    assert obs['persistent'] == 1 and obs['refused'] == 0, (what, obs)
    adm = [ln for ln in obs['lines'] if ln[7] == 'admitted']
    assert len(adm) == 1 and adm[0] == obs['lines'][-1], (what, obs['lines'])
    tag, block, total, nchunks, layout, per, demand, _, handoff, cell = adm[0]
    got = dict(tag=tag, block=int(block), total=int(total), nchunks=int(nchunks), layout=layout, handoff=handoff, cell=cell)
    want = {k: exp[k] for k in got}
    assert got == want, (what, got, want)
    # the verdict of the groups themselves: XCD-local only where the layout allows it and the switch leaves it on
    counts = (exp['groups'], 0) if exp['handoff'].startswith('local') else (0, exp['groups'])
    assert (obs['local'], obs['agent']) == counts, (what, obs, counts)
    return f'{tag} block {block} nchunks {nchunks} total {total} {layout} {handoff} {cell} demand {demand}'


def run_forms(G, H, B, T, packed, nd, env, monkeypatch, capfd, forms=None, persistent=True):
    """one forward (+ BPTT) of a case under `env`; -> results (CPU tensors), what the launches said"""
    from forwardtacotron_amd import hip as Hp, _lib
    inp = R.rnn_inputs(G, B, T, H, nd, 0, packed, packed)
    for k in [k for k in os.environ if k.startswith('FT_RNN_')]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('FT_RNN_DEBUG', '1')
    xp, dout = cuda(inp['xp']), cuda(inp['dout'])
    whh, bhh = [cuda(w) for w in inp['whh']], [cuda(b) for b in inp['bhh']]
    lens = None if inp['lens'] is None else cuda(inp['lens'])
    res, said = {}, {}
    old = _lib.lib().ft_rnn_set_persistent(int(persistent))
    try:
        la = Launches(capfd)
        if nd == 1:
            out = torch.empty(T, B, H, device='cuda')
            cst = torch.empty(T, B, H, device='cuda')
            ws, nb = Hp._rnn_workspace(4, B, H, xp.device)
            _lib.call('ft_lstm_fwd_uni', xp.data_ptr(), whh[0].data_ptr(), bhh[0].data_ptr(), out.data_ptr(), cst.data_ptr(),
                      B, T, H, None if ws is None else ws.data_ptr(), nb, Hp._stream())
            gates = None
        elif G == 4:
            out, cst, gates = Hp.lstm_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], lens, H, True)
        elif packed:
            out, cst, gates = Hp.gru_fwd_lens(xp, whh[0], whh[1], bhh[0], bhh[1], lens, H), None, None
        else:
            (out, gates), cst = Hp.gru_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], H, True), None
        said['fwd'] = la.done()
        res.update(out=out.cpu(), cst=None if cst is None else cst.cpu(), gates=None if gates is None else gates.cpu())
        if gates is not None:
            wt = [cuda(w.T) for w in inp['whh']]
            la = Launches(capfd)
            if G == 4:
                res['dxp'] = Hp.lstm_bwd(dout, out, cst, gates, wt[0], wt[1], lens, H).cpu()
            else:
                dxp, dhp = Hp.gru_bwd(dout, out, gates, wt[0], wt[1], H)
                res['dxp'], res['dhp'] = dxp.cpu(), dhp.cpu()
            said['bwd'] = la.done()
    finally:
        _lib.lib().ft_rnn_set_persistent(old)
        Hp.check_rnn_status()           # here a failed assertion cannot skip it: the sticky fault word is left clear
    return inp, res, said


def errors(inp, res):
    """max |GPU - float64| per output with its bound; asserts the exact zeros beyond an item's length"""
    G, B, T, H, nd, packed = inp['G'], inp['B'], inp['T'], inp['H'], inp['nd'], inp['lens'] is not None
    ref = R.reference64(G, B, T, H, nd, 0, packed, packed)
    act = R.active_mask(inp['lens'], B, T)
    out = {}
    for k, v in res.items():
        if v is None:
            continue
        g, r = v.double().numpy(), ref['dxp' if (k == 'dhp' and G == 4) else k]
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if k == 'gates':                          # saved activations exist at active positions only
            g, r = g[act], r[act]
        else:
            assert np.all(g[~act] == 0.0), f'{k}: not exactly zero beyond an item\'s length'
        assert np.all(np.isfinite(g)), k
        bound = R.FWD_TOL if k in ('out', 'cst', 'gates') else R.GRAD_TOL * max(1.0, float(np.abs(r).max()))
        out[k] = (float(np.abs(g - r).max()) if g.size else 0.0, bound)
    return out


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in a if k != 'gates') and \
        set(a) == set(b)


_base = {}


def base_run(G, H, B, T, packed, nd, env, monkeypatch, capfd):
    key = (G, H, B, T, packed, nd, tuple(sorted(env.items())))
    if key not in _base:
        _base[key] = run_forms(G, H, B, T, packed, nd, env, monkeypatch, capfd)[1]
    return _base[key]


def one_case(name, G, H, B, T, packed, nd, env, monkeypatch, capfd, base_env=None, equal=False, persistent=True):
    fwd, bwd = forms_of(G, H, env)
    inp, res, said = run_forms(G, H, B, T, packed, nd, env, monkeypatch, capfd, persistent=persistent)
    what = f'{name} G={G} H={H} B={B} T={T} packed={packed} nd={nd}'
    err = errors(inp, res)
    print(what, {k: f'{e:.2e}' for k, (e, _) in err.items()})
    paths = [check_path(said['fwd'], expect(fwd, nd, B, env), T, persistent, what + ' forward')]
    if 'bwd' in said:
        paths.append(check_path(said['bwd'], expect(bwd, 2, B, env), T, persistent, what + ' BPTT'))
    line = f'{what} | ' + ' | '.join(paths) + ' | ' + ' '.join(f'{k} {e:.2e}' for k, (e, _) in err.items())
    for k, (e, bound) in err.items():
        assert e <= bound, (what, k, e, bound)
    if base_env is not None:
        base = base_run(G, H, B, T, packed, nd, base_env, monkeypatch, capfd)
        fb = {k: v for k, v in base.items() if k in ('out', 'cst')}
        bits_f = same_bits({k: v for k, v in res.items() if k in ('out', 'cst')}, fb)
        # the BPTT of a switch that moves it from the reduce-scatter to the all-gather form sums in another order:
        # its bits are those of FT_RNN_BWD_RS=0
        bb = base
        if forms_of(G, H, env)[1]['tag'] != forms_of(G, H, base_env)[1]['tag']:
            bb = base_run(G, H, B, T, packed, nd, dict(base_env, **{RS: '0'}), monkeypatch, capfd)
        bits_b = same_bits({k: v for k, v in res.items() if k in ('dxp', 'dhp')},
                           {k: v for k, v in bb.items() if k in ('dxp', 'dhp')})
        if res['gates'] is not None:
            act = torch.from_numpy(R.active_mask(inp['lens'], B, T))
            bits_f = bits_f and torch.equal(res['gates'][act], base['gates'][act])
        base_name = ','.join(f'{k[7:]}={v}' for k, v in base_env.items()) or 'default'
        line += f' | bits vs {base_name}: forward {"equal" if bits_f else "DIFFER"}, BPTT ' + \
                (('equal' if bits_b else 'DIFFER') if 'dxp' in res else 'n/a')
        RECORD.append(line)
        if equal:
            assert bits_f, what + ': forward bits differ from the base form'
            assert bits_b, what + ': BPTT bits differ from the base form'
    else:
        RECORD.append(line)
    return res


DEFAULT_CASES = [(G, H, B, T, p) for (G, H) in R.WIDTHS for (B, T, p) in R.BT]


@pytest.mark.parametrize('G,H,B,T,packed', DEFAULT_CASES)
def test_default_form_vs_float64_and_repeatable(G, H, B, T, packed, monkeypatch, capfd):
    first = one_case('default', G, H, B, T, packed, 2, {}, monkeypatch, capfd)
    again = run_forms(G, H, B, T, packed, 2, {}, monkeypatch, capfd)[1]
    assert same_bits({k: v for k, v in first.items() if k != 'gates'}, {k: v for k, v in again.items() if k != 'gates'}), \
        'the default form is not repeatable bit for bit'
    _base.setdefault((G, H, B, T, packed, 2, ()), first)


VARIANT_CASES = [(i, B, T, p) for i in range(len(VARIANTS)) for (B, T, p) in VARIANT_BT]


@pytest.mark.parametrize('i,B,T,packed', VARIANT_CASES,
                         ids=[f'{VARIANTS[i][0]}-{VARIANTS[i][1]}-' + ','.join(f'{k[7:]}={v}' for k, v in VARIANTS[i][2].items())
                              + f'-{B}-{T}-{p}' for (i, B, T, p) in VARIANT_CASES])
def test_form_switch_vs_float64(i, B, T, packed, monkeypatch, capfd):
    G, H, env, _, _ = VARIANTS[i]
    one_case(','.join(f'{k[7:]}={v}' for k, v in env.items()), G, H, B, T, packed, 2, env, monkeypatch, capfd)


@pytest.mark.parametrize('B,T,packed', HANDOFF_BT)
@pytest.mark.parametrize('G,H', HANDOFF_WIDTHS)
@pytest.mark.parametrize('switch', list(HANDOFF))
def test_handoff_switch_vs_float64_and_default_bits(switch, G, H, B, T, packed, monkeypatch, capfd):
    env, equal = HANDOFF[switch]
    one_case(switch, G, H, B, T, packed, 2, env, monkeypatch, capfd, base_env={}, equal=equal)


@pytest.mark.parametrize('B,T,packed', HANDOFF_BT)
@pytest.mark.parametrize('gran4', ['1', '0'])
def test_gran4_on_the_four_block_forward(gran4, B, T, packed, monkeypatch, capfd):
    """FT_RNN_GRAN4 on the only kernel it addresses (fwd<4,4,1,8,4,16>): flag words either way, the form's own bits"""
    one_case(f'FWD_UB16=0,GRAN4={gran4}', 4, 512, B, T, packed, 2, GRAN4_ENVS[gran4], monkeypatch, capfd,
             base_env=GRAN4_BASE, equal=True)


@pytest.mark.parametrize('G,H', [(3, 64), (3, 256), (4, 128), (4, 512)])
@pytest.mark.parametrize('B,T,packed', [(21, 9, False), (33, 12, True)])
def test_per_step_form_vs_float64(G, H, B, T, packed, monkeypatch, capfd):
    one_case('per-step', G, H, B, T, packed, 2, {}, monkeypatch, capfd, persistent=False)


@pytest.mark.parametrize('H,B,T', R.UNI)
@pytest.mark.parametrize('switch', ['default'] + list(HANDOFF))
def test_one_direction_lstm_512(switch, H, B, T, monkeypatch, capfd):
    """ft_lstm_fwd_uni: the bidirectional forward with one direction's groups; rows_per_wg(1, B) picks 8 rows at B = 9
    and 40 (two and five groups), 16 at B = 3"""
    env, equal = HANDOFF.get(switch, ({}, True))
    assert rows_per_wg(1, B, {}) == (16 if B == 3 else 8)
    res = one_case(switch, 4, H, B, T, False, 1, env, monkeypatch, capfd, base_env={}, equal=equal)
    if switch == 'default':
        again = run_forms(4, H, B, T, False, 1, {}, monkeypatch, capfd)[1]
        assert torch.equal(res['out'], again['out']) and torch.equal(res['cst'], again['cst'])


def test_every_documented_switch_is_set_by_a_case():
    """the switches INTEGRATION.md documents against the environments the cases above really run with (the keys of
    VARIANTS, HANDOFF and the FT_RNN_GRAN4 test's), not against this file's text"""
    doc = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()
    documented = set(re.findall(r'`(FT_RNN_[A-Z0-9_]+)', doc))
    covered_elsewhere = {'FT_RNN_PERSISTENT', 'FT_RNN_ADMIT_PCT', 'FT_RNN_DEBUG', 'FT_RNN_OVERLAP', 'FT_RNN_CHUNKS',
                         'FT_RNN_REV_LEAD'}
    envs = [v[2] for v in VARIANTS] + [e for e, _ in HANDOFF.values()] + list(GRAN4_ENVS.values())
    set_here = set(k for e in envs for k in e)
    assert {i for (i, _, _, _) in VARIANT_CASES} == set(range(len(VARIANTS))), 'a form switch has no case left'
    missing = documented - covered_elsewhere - set_here
    assert not missing, f'documented but set by no case: {sorted(missing)}'
