"""Every form and hand-off of the persistent recurrences (csrc/ft_rnn_persist.hip) against float64.

Each case calls the primitives directly (hip.gru_fwd / gru_fwd_lens / gru_bwd, hip.lstm_fwd / lstm_bwd, ft_lstm_fwd_uni)
with one set of FT_RNN_* switches (read per launch), compares EVERY output with tests/rnn_cpu.py in float64, proves the
path taken -- launch counters, XCD-local / agent-scope group counts and the library's FT_RNN_DEBUG line, which names the
kernel instantiation, the layout and the hand-off -- and, where a switch only changes how values travel or where
workgroups sit, demands the default form's bits.  dout is random.  profiles/rnn_forms.txt is the record of one run.

THE TABLE.  Derived from fwd_persistent / bwd_persistent / bwd_persistent_rs.  Kernel tags as the debug line prints them:
    fwd<G, waves, bf16-split, units per workgroup, resident 32-k blocks per wave, rows per workgroup>
    bwd<G, waves, resident 16-k groups per wave, bf16-split, rows>            (all-gather BPTT)
    bwd_rs<G, waves, output tiles per wave, rows>                             (reduce-scatter BPTT)
threads per workgroup = 64 * waves; nchunks (workgroups per (direction, batch group)) = H / units per workgroup (fwd),
H / 16 (both BPTT forms); rows 'R' = rows_per_wg(nd, B): 8 at B = 21 (nd = 2), 16 at B = 5 and 33, 16 with FT_RNN_MB=16.
Layout A = aligned (a group per XCD slot: XCD-local hand-off), S = spread (agent scope): aligned needs nchunks <= 64 and
nchunks * ceil(groups / 8) workgroups per slot within 32 CUs x (workgroups per CU of the kernel, 1 for all 8- and
16-wave kernels here, 2 for the 4-wave forward ones).  A grid beyond that in the spread layout too (ceil(total / 8) per slot) is
REFUSED: the refused-launch counter moves by one, no persistent launch, and the call runs on the per-step kernels; the
cases keep those batches and expect exactly that (the BPTT of the same shape may still fit, and then runs persistent).

  G H    switches                  forward                 thr  nch lay | BPTT                   thr  nch lay
  3 16   -                         fwd<3,4,0,8,1,16>       256  2   A   | bwd<3,4,8,0,16>        256  1   A    K % 32 != 0: f32 MFMA
  3 48   -                         fwd<3,4,0,8,1,16>       256  6   A   | bwd<3,4,8,0,16>        256  3   A
  3 64   -                         fwd<3,4,1,8,1,16>       256  8   A   | bwd<3,4,8,1,16>        256  4   A
  3 64   BWD_RS=2                  (as above)                           | bwd_rs<3,4,1,16>       256  4   A
  3 128  -                         fwd<3,4,1,8,1,16>       256  16  A   | bwd<3,8,8,1,16>        512  8   A
  3 128  BWD_RS=2                  (as above)                           | bwd_rs<3,8,1,16>       512  8   A
  3 256  -                         fwd<3,8,1,16,1,R>       512  16  A   | bwd<3,8,8,1,R>         512  16  A
  3 256  GRU_WIDE=0                fwd<3,4,1,8,2,16>       256  32  A   | (as above)
  3 256  BWD_RS=2                  (as default)                         | bwd_rs<3,8,2,16>       512  16  A
  3 272  -                         fwd<3,8,0,8,1,16>       512  34  S   | bwd<3,8,8,0,16>        512  17  A    H % 32 != 0 on 8 waves
  3 512  -                         fwd<3,8,1,8,2,16>       512  64  S   | bwd_rs<3,8,4,16>       512  32  A    forward refused at B = 33
  3 512  BWD_RS=0                  (as above)                           | bwd<3,8,16,1,16>       512  32  A
  3 512  B3=0                      fwd<3,8,0,8,1,16>       512  64  S   | bwd<3,8,16,0,16>       512  32  A
  3 704  -                         fwd<3,8,0,8,1,16>       512  88  S   | bwd<3,16,16,1,16>      1024 44  S    refused: forward B > 16, BPTT B = 33
  3 704  B3=0                      (as above)                           | bwd<3,16,16,0,16>      1024 44  S
  4 16   -                         fwd<4,4,0,8,1,16>       256  2   A   | bwd<4,4,8,1,16>        256  1   A
  4 64   -                         fwd<4,4,1,8,1,16>       256  8   A   | bwd<4,4,8,1,16>        256  4   A
  4 64   B3=0                      fwd<4,4,0,8,1,16>       256  8   A   | bwd<4,4,8,0,16>        256  4   A
  4 64   BWD_RS=2                  (as default)                         | bwd_rs<4,4,1,16>       256  4   A
  4 128  -                         fwd<4,4,1,8,1,16>       256  16  A   | bwd<4,8,8,1,16>        512  8   A
  4 128  B3=0                      fwd<4,4,0,8,1,16>       256  16  A   | bwd<4,8,8,0,16>        512  8   A
  4 128  BWD_RS=2                  (as default)                         | bwd_rs<4,8,1,16>       512  8   A
  4 256  -                         fwd<4,4,1,8,2,16>       256  32  A   | bwd_rs<4,8,2,16>       512  16  A
  4 256  BWD_RS=0                  (as above)                           | bwd<4,8,8,1,16>        512  16  A
  4 512  -                         fwd<4,8,1,16,2,R>       512  32  A   | bwd_rs<4,8,4,R>        512  32  A    the benchmark's decoder
  4 512  MB=16                     fwd<4,8,1,16,2,16>      512  32  A   | bwd_rs<4,8,4,16>       512  32  A
  4 512  FWD_UB16=0                fwd<4,4,1,8,4,16>       256  64  A   | (as default)                         4 resident k-blocks
  4 512  FWD_UB16=0 FWD_NW4=0      fwd<4,8,1,8,2,16>       512  64  S   | (as default)                         forward refused at B = 33
  4 512  B3=0                      fwd<4,4,0,8,1,16>       256  64  A   | bwd<4,8,16,0,16>       512  32  A    (no bf16 split, no reduce-scatter)
  4 512  B3=0 FWD_NW4=0            fwd<4,8,0,8,1,16>       512  64  S   | (as above)                           forward refused at B = 33
  4 512  BWD_RS=0                  (as default)                         | bwd<4,8,16,1,16>       512  32  A
  4 528  -                         fwd<4,8,0,8,1,16>       512  66  S   | bwd<4,16,16,1,16>      1024 33  S    16-wave all-gather; forward refused at B > 16
  4 528  B3=0                      (as above)                           | bwd<4,16,16,0,16>      1024 33  S
  ft_lstm_fwd_uni 512 (nd = 1)     fwd<4,8,1,16,2,R>       512  32  A                                          R = 8 at B = 9 and 40, 16 at B = 3

Hand-off and layout switches, on top of the default form (GRU 64, 256; LSTM 128, 256, 512; ft_lstm_fwd_uni 512):
  FT_RNN_LOCAL=0      aligned layout, agent-scope hand-off: (0, groups)                    bit-equal to the default
  FT_RNN_XCDALIGN=0   spread layout: (0, groups)                                           bit-equal
  FT_RNN_XCDMAP=0     identity grid decode, hence spread: (0, groups)                      bit-equal
  FT_RNN_SIG=0        one signal per workgroup, hence spread: (0, groups); the reduce-scatter BPTT needs per-wave
                      signals, so LSTM 256 / 512 take the all-gather form                  bit-equal (BPTT: to FT_RNN_BWD_RS=0)
  FT_RNN_GRANULES=0   XCD-local hand-off through flag words: (groups, 0)                   bit-equal
  FT_RNN_GRAN4=0      LSTM-512 FT_RNN_FWD_UB16=0 form (4 resident k-blocks): that kernel has no granule form (GRAN needs
                      BC <= 2), it hands over through flag words either way: NO EFFECT     bit-equal
  FT_RNN_FAST_CELL=0  exact exp / tanh in the cell: other roundings                        float64 bound only
  FT_RNN_MB=16        16 rows per workgroup where the default takes 8 (B = 21)             bit-equal
(the same products in the same order reach every accumulator under all of these: an MFMA result element depends on its
own A row only, the bf16 split is one function for producer and consumer, and no switch but FT_RNN_FAST_CELL, FT_RNN_B3
and the form switches changes an operand or a summation order.)

Instantiations compiled but not reachable through any (G, H, switch):
  fwd<G,8,1,8,1,16> (G = 3, 4)   8 waves need H > 256, one k-block per wave needs H <= 256
  fwd<3,4,1,8,4,16>              4 waves x 4 blocks: only the LSTM is moved from 8 to 4 waves (FT_RNN_FWD_NW4)
  fwd<3,8,1,16,2,16>             the 16-unit, 2-block form is the LSTM's (wide requires G == 4)
A packed item of length 0 is admitted by every entry point (clamp_len: never active) and is part of every packed case."""
import os
import re

import numpy as np
import pytest
import torch

import rnn_cpu as R

pytestmark = pytest.mark.gpu


def F(tag, threads, nchunks, layout='A', fits=99):
    """fits: the largest batch whose grid fits the chip (demand <= 1 in the spread layout); a larger one is REFUSED the
    persistent form -- one refused launch on the counters -- and runs on the per-step kernels"""
    return dict(tag=tag, threads=threads, nchunks=nchunks, layout=layout, fits=fits)


# (G, H) -> default forms
DEFAULT = {
    (3, 16): (F('fwd<3,4,0,8,1,16>', 256, 2), F('bwd<3,4,8,0,16,-1>', 256, 1)),
    (3, 48): (F('fwd<3,4,0,8,1,16>', 256, 6), F('bwd<3,4,8,0,16,-1>', 256, 3)),
    (3, 64): (F('fwd<3,4,1,8,1,16>', 256, 8), F('bwd<3,4,8,1,16,-1>', 256, 4)),
    (3, 128): (F('fwd<3,4,1,8,1,16>', 256, 16), F('bwd<3,8,8,1,16,-1>', 512, 8)),
    (3, 256): (F('fwd<3,8,1,16,1,R>', 512, 16), F('bwd<3,8,8,1,R,-1>', 512, 16)),
    (3, 272): (F('fwd<3,8,0,8,1,16>', 512, 34, 'S'), F('bwd<3,8,8,0,16,-1>', 512, 17)),
    (3, 512): (F('fwd<3,8,1,8,2,16>', 512, 64, 'S', 32), F('bwd_rs<3,8,4,16,-1,-1>', 512, 32)),
    (3, 704): (F('fwd<3,8,0,8,1,16>', 512, 88, 'S', 16), F('bwd<3,16,16,1,16,-1>', 1024, 44, 'S', 32)),
    (4, 16): (F('fwd<4,4,0,8,1,16>', 256, 2), F('bwd<4,4,8,1,16,-1>', 256, 1)),
    (4, 64): (F('fwd<4,4,1,8,1,16>', 256, 8), F('bwd<4,4,8,1,16,-1>', 256, 4)),
    (4, 128): (F('fwd<4,4,1,8,1,16>', 256, 16), F('bwd<4,8,8,1,16,-1>', 512, 8)),
    (4, 256): (F('fwd<4,4,1,8,2,16>', 256, 32), F('bwd_rs<4,8,2,16,-1,-1>', 512, 16)),
    (4, 512): (F('fwd<4,8,1,16,2,R>', 512, 32), F('bwd_rs<4,8,4,R,-1,-1>', 512, 32)),
    (4, 528): (F('fwd<4,8,0,8,1,16>', 512, 66, 'S', 16), F('bwd<4,16,16,1,16,-1>', 1024, 33, 'S')),
}
AG256 = F('bwd<4,8,8,1,16,-1>', 512, 16)
AG512 = F('bwd<4,8,16,1,16,-1>', 512, 32)
RS = 'FT_RNN_BWD_RS'
# form switches: (G, H, switches) -> (forward, BPTT) where they differ from the default (None: as the default)
VARIANTS = [
    (3, 64, {RS: '2'}, None, F('bwd_rs<3,4,1,16,-1,-1>', 256, 4)),
    (3, 128, {RS: '2'}, None, F('bwd_rs<3,8,1,16,-1,-1>', 512, 8)),
    (3, 256, {RS: '2'}, None, F('bwd_rs<3,8,2,16,-1,-1>', 512, 16)),
    (3, 256, {'FT_RNN_GRU_WIDE': '0'}, F('fwd<3,4,1,8,2,16>', 256, 32), None),
    (3, 512, {RS: '0'}, None, F('bwd<3,8,16,1,16,-1>', 512, 32)),
    (3, 512, {'FT_RNN_B3': '0'}, F('fwd<3,8,0,8,1,16>', 512, 64, 'S', 32), F('bwd<3,8,16,0,16,-1>', 512, 32)),
    (3, 704, {'FT_RNN_B3': '0'}, None, F('bwd<3,16,16,0,16,-1>', 1024, 44, 'S', 32)),
    (4, 64, {'FT_RNN_B3': '0'}, F('fwd<4,4,0,8,1,16>', 256, 8), F('bwd<4,4,8,0,16,-1>', 256, 4)),
    (4, 64, {RS: '2'}, None, F('bwd_rs<4,4,1,16,-1,-1>', 256, 4)),
    (4, 128, {'FT_RNN_B3': '0'}, F('fwd<4,4,0,8,1,16>', 256, 16), F('bwd<4,8,8,0,16,-1>', 512, 8)),
    (4, 128, {RS: '2'}, None, F('bwd_rs<4,8,1,16,-1,-1>', 512, 8)),
    (4, 256, {RS: '0'}, None, AG256),
    (4, 512, {'FT_RNN_FWD_UB16': '0'}, F('fwd<4,4,1,8,4,16>', 256, 64), None),
    (4, 512, {'FT_RNN_FWD_UB16': '0', 'FT_RNN_FWD_NW4': '0'}, F('fwd<4,8,1,8,2,16>', 512, 64, 'S', 32), None),
    (4, 512, {'FT_RNN_B3': '0'}, F('fwd<4,4,0,8,1,16>', 256, 64), F('bwd<4,8,16,0,16,-1>', 512, 32)),
    (4, 512, {'FT_RNN_B3': '0', 'FT_RNN_FWD_NW4': '0'}, F('fwd<4,8,0,8,1,16>', 512, 64, 'S', 32),
     F('bwd<4,8,16,0,16,-1>', 512, 32)),
    (4, 512, {RS: '0'}, None, AG512),
    (4, 528, {'FT_RNN_B3': '0'}, None, F('bwd<4,16,16,0,16,-1>', 1024, 33, 'S')),
]
# hand-off / layout switches: name -> (switches, bit-equal to the base form)
HANDOFF = {
    'LOCAL=0': ({'FT_RNN_LOCAL': '0'}, True),
    'XCDALIGN=0': ({'FT_RNN_XCDALIGN': '0'}, True),
    'XCDMAP=0': ({'FT_RNN_XCDMAP': '0'}, True),
    'SIG=0': ({'FT_RNN_SIG': '0'}, True),
    'GRANULES=0': ({'FT_RNN_GRANULES': '0'}, True),
    'FAST_CELL=0': ({'FT_RNN_FAST_CELL': '0'}, False),
    'LOCAL=0,GRANULES=0': ({'FT_RNN_LOCAL': '0', 'FT_RNN_GRANULES': '0'}, True),
    'MB=16': ({'FT_RNN_MB': '16'}, True),
}
GRAN4_BASE = {'FT_RNN_FWD_UB16': '0'}            # the form FT_RNN_GRAN4 addresses
GRAN4_ENVS = {g: dict(GRAN4_BASE, FT_RNN_GRAN4=g) for g in ('1', '0')}
HANDOFF_WIDTHS = [(3, 64), (3, 256), (4, 128), (4, 256), (4, 512)]
HANDOFF_BT = [(21, 9, False), (33, 12, True), (5, 2, False)]
VARIANT_BT = [(21, 9, False), (33, 12, True), (5, 2, False), (5, 12, True)]

LINE = re.compile(r'\[ft_rnn\] (\w+<[-\d,]+>) block (\d+) total (\d+) nchunks (\d+): (\w+) layout, (\d+) workgroups per XCD '
                  r'slot, demand ([\d.]+) -> (\w+); hand-off ([\w-]+), cell (\w+)')


def rows_per_wg(nd, B, env):
    if env.get('FT_RNN_MB') == '16':
        return 16
    g16, g8 = nd * -(-B // 16), nd * -(-B // 8)
    return 8 if g16 < 8 and g8 <= 8 and g8 > g16 else 16


def spread_only(env):
    return any(env.get(k) == '0' for k in ('FT_RNN_XCDALIGN', 'FT_RNN_XCDMAP', 'FT_RNN_SIG'))


def has_granules(tag):
    v = [int(x) for x in tag[tag.index('<') + 1:-1].split(',')]
    if tag.startswith('fwd<'):
        return v[2] == 1 and v[4] <= 2
    if tag.startswith('bwd<'):
        return v[3] == 1 and v[2] <= 8
    return False


def expect(form, nd, B, env):
    """what the admitted debug line of a launch must say"""
    rows = rows_per_wg(nd, B, env) if ',R' in form['tag'] else 16
    tag = form['tag'].replace('R', str(rows))
    layout = 'spread' if form['layout'] == 'S' or spread_only(env) else 'aligned'
    groups = nd * -(-B // rows)
    local = layout == 'aligned' and env.get('FT_RNN_LOCAL') != '0'
    gran = has_granules(tag) and env.get('FT_RNN_GRANULES') != '0'
    return dict(tag=tag, block=form['threads'], nchunks=form['nchunks'], total=groups * form['nchunks'], layout=layout,
                groups=groups, handoff=('local-granules' if gran else 'local-flags') if local else 'agent',
                cell='exact' if env.get('FT_RNN_FAST_CELL') == '0' else 'fast', rows=rows, admitted=B <= form['fits'])


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


def forms_of(G, H, env):
    """(forward, BPTT) expectation of (G, H) under the form switches in env"""
    fwd, bwd = DEFAULT[(G, H)]
    for (g, h, e, f, b) in VARIANTS:
        if (g, h) == (G, H) and all(env.get(k) == v for k, v in e.items()) and \
                not any(k in env and k not in e for k in ('FT_RNN_B3', 'FT_RNN_FWD_NW4', 'FT_RNN_FWD_UB16', RS)):
            fwd, bwd = f or fwd, b or bwd
    if env.get('FT_RNN_SIG') == '0' and bwd['tag'].startswith('bwd_rs'):       # no per-wave signals: all-gather
        bwd = {256: AG256, 512: AG512}[H]
    return fwd, bwd


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
