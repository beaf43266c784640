"""The forms of the persistent recurrences (csrc/ft_rnn_persist.hip, planned by csrc/ft_rnn_plan.h), restated by hand: what
tests/test_gpu_rnn_forms.py demands of the launches on the GPU and tests/test_rnn_plan_cpu.py of ft_rnn_plan without one.
An independent reference: nothing here calls the library.

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
  fwd<3,8,1,16,2,16>             the 16-unit, 2-block form is the LSTM's (wide requires G == 4)"""


def F(tag, threads, nchunks, layout='A', fits=99):
    """fits: the largest batch whose grid fits the chip (demand <= 1 in the spread layout); a larger one is REFUSED the
    persistent form -- one refused launch on the counters -- and runs on the per-step kernels.  99: every batch up to 64.
    (48 on the 34- and 33-chunk spread forms: a fourth batch group makes 8 x 34 / 8 = 34 or 8 x 33 / 8 = 33 one-per-CU
    workgroups per XCD slot, more than its 32 CUs.)"""
    return dict(tag=tag, threads=threads, nchunks=nchunks, layout=layout, fits=fits)


# (G, H) -> default forms
DEFAULT = {
    (3, 16): (F('fwd<3,4,0,8,1,16>', 256, 2), F('bwd<3,4,8,0,16,-1>', 256, 1)),
    (3, 48): (F('fwd<3,4,0,8,1,16>', 256, 6), F('bwd<3,4,8,0,16,-1>', 256, 3)),
    (3, 64): (F('fwd<3,4,1,8,1,16>', 256, 8), F('bwd<3,4,8,1,16,-1>', 256, 4)),
    (3, 128): (F('fwd<3,4,1,8,1,16>', 256, 16), F('bwd<3,8,8,1,16,-1>', 512, 8)),
    (3, 256): (F('fwd<3,8,1,16,1,R>', 512, 16), F('bwd<3,8,8,1,R,-1>', 512, 16)),
    (3, 272): (F('fwd<3,8,0,8,1,16>', 512, 34, 'S', 48), F('bwd<3,8,8,0,16,-1>', 512, 17)),
    (3, 512): (F('fwd<3,8,1,8,2,16>', 512, 64, 'S', 32), F('bwd_rs<3,8,4,16,-1,-1>', 512, 32)),
    (3, 704): (F('fwd<3,8,0,8,1,16>', 512, 88, 'S', 16), F('bwd<3,16,16,1,16,-1>', 1024, 44, 'S', 32)),
    (4, 16): (F('fwd<4,4,0,8,1,16>', 256, 2), F('bwd<4,4,8,1,16,-1>', 256, 1)),
    (4, 64): (F('fwd<4,4,1,8,1,16>', 256, 8), F('bwd<4,4,8,1,16,-1>', 256, 4)),
    (4, 128): (F('fwd<4,4,1,8,1,16>', 256, 16), F('bwd<4,8,8,1,16,-1>', 512, 8)),
    (4, 256): (F('fwd<4,4,1,8,2,16>', 256, 32), F('bwd_rs<4,8,2,16,-1,-1>', 512, 16)),
    (4, 512): (F('fwd<4,8,1,16,2,R>', 512, 32), F('bwd_rs<4,8,4,R,-1,-1>', 512, 32)),
    (4, 528): (F('fwd<4,8,0,8,1,16>', 512, 66, 'S', 16), F('bwd<4,16,16,1,16,-1>', 1024, 33, 'S', 48)),
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
    (4, 528, {'FT_RNN_B3': '0'}, None, F('bwd<4,16,16,0,16,-1>', 1024, 33, 'S', 48)),
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
HANDOFF_WIDTHS = [(3, 64), (3, 256), (4, 128), (4, 256), (4, 512)]


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
