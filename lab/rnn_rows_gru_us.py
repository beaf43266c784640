"""us per dependent step of the 256-wide GRU's persistent forward and all-gather BPTT, 16 against 8 batch rows per
workgroup (FT_RNN_MB toggled in-process, runs interleaved), with the bit-equality of the two forms and the groups that
ran XCD-local.    python lab/rnn_rows_gru_us.py [B] [T] [reps]"""
import os, statistics, sys, torch
sys.path.insert(0, '.')
from forwardtacotron_amd import hip as H
dev = 'cuda'
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
T = int(sys.argv[2]) if len(sys.argv) > 2 else 841
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
Hh = 256
g = torch.Generator().manual_seed(0)
xp = (torch.randn(T, B, 6 * Hh, generator=g) * 0.1).to(dev)
whh = [(torch.randn(3 * Hh, Hh, generator=g) * 0.05).to(dev) for _ in range(2)]
bhh = [torch.zeros(3 * Hh, device=dev) for _ in range(2)]
dout = (torch.randn(T, B, 2 * Hh, generator=g) * 0.1).to(dev)
wt = [H.transpose2d(w) for w in whh]


def timed(f):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); r = f(); e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / T, r


us = {mb: ([], []) for mb in (16, 8)}
res = {}
for rep in range(reps + 1):
    for mb in (16, 8):
        os.environ['FT_RNN_MB'] = str(mb)
        m0 = H.rnn_mode_counts()
        tf, (out, gates) = timed(lambda: H.gru_fwd(xp, whh[0], whh[1], bhh[0], bhh[1], Hh, True))
        tb, (dxp, dhp) = timed(lambda: H.gru_bwd(dout, out, gates, wt[0], wt[1], Hh))
        m1 = H.rnn_mode_counts()
        if rep == 0:                         # warm-up: keep the results and the group modes
            res[mb] = ((out, gates, dxp, dhp), (m1[0] - m0[0], m1[1] - m0[1]))
            continue
        us[mb][0].append(tf)
        us[mb][1].append(tb)
H.check_rnn_status()
same = [torch.equal(a, b) for a, b in zip(res[8][0], res[16][0])]
for mb in (16, 8):
    f, b = us[mb]
    print(f'GRU-256 B{B} T{T} MB={mb:2d}: fwd {statistics.median(f):.3f} us/step (min {min(f):.3f} max {max(f):.3f}) | '
          f'bwd {statistics.median(b):.3f} (min {min(b):.3f} max {max(b):.3f}) | groups local/agent {res[mb][1]}', flush=True)
print('bit-equal out/gates/dxp/dhp:', same)
print('persistent/refused', H.rnn_counters())
