"""The C-ABI calls of fixed scenarios as text, to show that a host-side change changed nothing.

    python tools/call_trace.py --out FILE [--only A,B,C,D,E,F,G]

Every launch of the package goes through _lib.call(name, *args).  For the duration of a scenario this tool replaces that
function and writes one line per call: the entry name, then its arguments as _lib.PROTOS types them -- scalars
verbatim, pointers as 0 (null) or 1, and a `void*` argument whose name contains `stream` as the ordinal of that
handle's first appearance in the scenario (s0, s1, ...).  torch.cuda.Stream.wait_stream is replaced for the same time and
writes `wait sA <- sB` with the same ordinals; consecutive waits of one stream with no call between them commute and are
written sorted (the train step's final join walks a set of streams, whose order follows the handles' addresses).  What the lines pin down is therefore which entries ran, in which order,
on which stream, behind which stream joins, with which sizes, seeds and switches; behind each scenario follows one line per returned
tensor (`= key sha256-of-its-bytes`), which pins down the result.  Run it on two commits with FT_LIB pointing at one
build of the same C sources and `diff` the two files: an empty diff is the proof.

NOT traced: whatever bypasses _lib.call -- _lib.query (workspace sizes, counters), the process-wide switches set
through _lib.lib() (ft_set_gemm_precision, ft_rnn_set_persistent) and torch's own work (copies, allocations, the few
element-wise torch ops of the models' host code).  A changed precision mode shows in the entries the GEMM-backed calls
pick and in the hashes.

It uses only the package's public surface, tests/helpers.py and the committed fixtures.  Scenarios (all under
torch.manual_seed(0)):

  A  ForwardTacotron, tiny config, generate_batch.npz: generate of one item; generate_batch with x_len on the host, on the
     device, and with FT_GEN_OVERLAP=0; eval forward under no_grad (the CBHG and BatchNormConv eval bodies)
  B  FastPitch, tiny config, fastpitch_generate_batch.npz, fp32: the same (head widths 4 and 8: the byte-mask routes)
  C  FastPitch at production widths, one layer per stack, x_len [40, 13, 1, 27, 40]: generate_batch in fp32 and bf16, each
     with FT_ATTN_LENS unset and =0 (all three attention routes)
  D  the same model in training mode, B = 2, Tx = 16: forward and backward of the summed outputs in fp32 (per-operation
     nodes), bf16 (the C-issued composite) and bf16 with FT_FFT_COMPOSITE=0 (TransformerFn's Python loop)
  E  ForwardTacotron, tiny_model.npz: two TrainStep.step calls from fresh weights -> the loss terms and every parameter;
     under the default switches, under each input of test_step_schedule_variants_give_the_same_update and under
     FT_PRED_STAGE_FIRST=1 (with =0 among the former: late weight gradients on and off whatever the admission arithmetic
     says at these widths)
  F  MultiForwardTacotron, tiny_multi.npz: the same, default switches
  G  FastPitch, the same two steps: tiny_fastpitch.npz in fp32 (one node per operation: every side launch on its own) and
     with FT_TRANSFORMER_NODE=1 (TransformerFn's Python loop: a block's launches batched); scenario D's model and batch in
     bf16 (the composite) and with FT_FFT_SUMS_STREAM=1 on top

Needs a GPU: there is no CPU fallback.
"""
import argparse
import contextlib
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from forwardtacotron_amd import _lib, data  # noqa: E402
from helpers import TINY, TINY_FP, TINY_MULTI, TRAIN_CFG, TRAIN_CFG_MULTI, fp_state, load_npz, sub  # noqa: E402

X_LEN = [40, 13, 1, 27, 40]


class Trace:
    """the lines of one output file; `scenario` swaps _lib.call for the time of one scenario"""

    def __init__(self):
        self.lines, self.streams, self.calls, self.waits = [], {}, 0, 0

    def _call(self, name, *args):
        out = [name]
        for (ctype, arg), v in zip(_lib.PROTOS[name][1], args):
            if ctype.replace(' ', '') == 'void*' and 'stream' in arg:
                out.append(self._ordinal(v))
            elif ctype.endswith('*'):
                out.append('0' if v is None or v == 0 else '1')
            else:
                out.append(repr(v.value if hasattr(v, 'value') else v))
        self.lines.append(' '.join(out))
        self.calls += 1
        return self._real(name, *args)

    def _ordinal(self, handle):
        return self.streams.setdefault(handle or 0, f's{len(self.streams)}')

    @contextlib.contextmanager
    def scenario(self, title):
        self.lines.append(f'## {title}')
        self.streams, self.calls, self.waits = {}, 0, 0
        real_wait = torch.cuda.Stream.wait_stream

        def wait_stream(waiter, waited):
            self.lines.append(f'wait {self._ordinal(waiter.cuda_stream)} <- {self._ordinal(waited.cuda_stream)}')
            self.waits += 1
            return real_wait(waiter, waited)

        self._real, _lib.call = _lib.call, self._call
        torch.cuda.Stream.wait_stream = wait_stream
        try:
            yield
            torch.cuda.synchronize()
        finally:
            _lib.call = self._real
            torch.cuda.Stream.wait_stream = real_wait
        print(f'{title}: {self.calls} calls, {self.waits} stream waits')

    def result(self, out):
        for k in sorted(out):
            if torch.is_tensor(out[k]):
                t = out[k].detach().cpu().contiguous()
                self.lines.append(f'= {k} {tuple(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}')


def canonical(lines):
    """the lines with every run of consecutive `wait sA <- ...` lines of one waiter sorted"""
    out, run = [], []
    for line in lines + ['']:
        if run and not (line.startswith('wait ') and line.split()[1] == run[0].split()[1]):
            out += sorted(run)
            run = []
        (run if line.startswith('wait ') else out).append(line)
    return out[:-1]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)


def inference(tr, tag, m, x, x_len, alpha):
    """generate of one item and the three generate_batch calls of scenarios A and B"""
    with tr.scenario(f'{tag} generate, item 2 alone'):
        tr.result(m.generate(x[2:3, :int(x_len[2])].contiguous(), alpha=alpha))
    with tr.scenario(f'{tag} generate_batch, x_len on the host'):
        tr.result(m.generate_batch(x, x_len, alpha=alpha))
    with tr.scenario(f'{tag} generate_batch, x_len on the device'):
        tr.result(m.generate_batch(x, x_len.cuda(), alpha=alpha))
    with env(FT_GEN_OVERLAP='0'), tr.scenario(f'{tag} generate_batch, FT_GEN_OVERLAP=0'):
        tr.result(m.generate_batch(x, x_len, alpha=alpha))


def scenario_a(tr):
    from forwardtacotron_amd.model import ForwardTacotron
    G = load_npz('generate_batch.npz')
    m = ForwardTacotron(**TINY)
    m.load_state_dict(sub(G, 'sd/'))
    m = m.cuda()
    inference(tr, 'A', m, torch.from_numpy(G['x']).cuda(), torch.from_numpy(G['x_len']), float(G['alpha']))
    batch = data.to_device(data.synthetic_batch(B=3, Tmax=9, n_mels=TINY['n_mels'], max_dur=4, seed=2), 'cuda')
    m.eval()
    with torch.no_grad(), tr.scenario('A eval forward'):
        tr.result(m(batch))


def scenario_b(tr):
    from forwardtacotron_amd.fastpitch import FastPitch
    G = load_npz('fastpitch_generate_batch.npz')
    m = FastPitch(**TINY_FP)
    m.load_state_dict(fp_state(G, 'sd/'))
    m = m.cuda()
    inference(tr, 'B', m, torch.from_numpy(G['x']).cuda(), torch.from_numpy(G['x_len']), float(G['alpha']))


def production_fastpitch():
    """data.FASTPITCH_MODEL with one layer per stack and durations of a few frames per token"""
    from forwardtacotron_amd.fastpitch import FastPitch
    cfg = dict(data.FASTPITCH_MODEL, durpred_layers=1, pitch_layers=1, energy_layers=1, prenet_layers=1, postnet_layers=1)
    torch.manual_seed(0)
    m = FastPitch(**cfg)
    with torch.no_grad():
        m.dur_pred.lin.weight.mul_(3.0)
        m.dur_pred.lin.bias.fill_(2.5)
    return cfg, m.cuda()


def scenario_c(tr):
    cfg, m = production_fastpitch()
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(len(X_LEN), max(X_LEN), dtype=torch.long)
    for b, L in enumerate(X_LEN):
        x[b, :L] = torch.randint(1, cfg['num_chars'], (L,), generator=g)
    x, x_len = x.cuda(), torch.tensor(X_LEN)
    for mode in ('fp32', 'bf16'):
        m.matmul_dtype = mode
        with tr.scenario(f'C generate_batch {mode}'):
            tr.result(m.generate_batch(x, x_len, alpha=0.9))
        with env(FT_ATTN_LENS='0'), tr.scenario(f'C generate_batch {mode}, FT_ATTN_LENS=0'):
            tr.result(m.generate_batch(x, x_len, alpha=0.9))


def scenario_d(tr):
    from forwardtacotron_amd import hip
    cfg, m = production_fastpitch()
    batch = data.to_device(data.synthetic_batch(B=2, Tmax=16, n_mels=cfg['n_mels'], max_dur=6, seed=3), 'cuda')
    m.train()
    for mode, switches in (('fp32', {}), ('bf16', {}), ('bf16', {'FT_FFT_COMPOSITE': '0'})):
        m.matmul_dtype = mode
        m.zero_grad(set_to_none=True)
        torch.manual_seed(0)            # the dropout seeds
        title = f'D forward + backward {mode}' + ''.join(f', {k}={v}' for k, v in switches.items())
        with env(**switches), tr.scenario(title):
            out = m(batch)
            with hip.gemm_precision(mode):      # as trainer.TrainStep extends the mode over the backward
                sum(out[k].sum() for k in ('mel', 'mel_post', 'dur', 'pitch', 'energy')).backward()
            tr.result(out)
            tr.result({f'grad/{k}': p.grad for k, p in m.named_parameters() if p.grad is not None})


def train_steps(tr, title, make, batch, cfg, switches=None):
    """two TrainStep.step calls of a fresh model (make() -> a model on the device) under `switches`"""
    from forwardtacotron_amd.trainer import TrainStep
    switches = switches or {}
    with env(**switches):
        torch.manual_seed(0)            # the dropout seeds
        m = make()
        ts = TrainStep(m, lr=2e-3, train_cfg=cfg)
        with tr.scenario(title + ''.join(f', {k}={v}' for k, v in switches.items())):
            for i in (1, 2):
                out = ts.step({k: v.clone().cuda() for k, v in batch.items()})
                tr.result({f'step{i}/{k}': v for k, v in out.items()})
            ts.check()
            tr.result({f'param/{k}': p for k, p in m.named_parameters()})
        ts.close()


# the inputs of tests/test_gpu_trainer.py::test_step_schedule_variants_give_the_same_update, then the predictors first
STEP_SWITCHES = [{}, {'FT_PRED_BWD_EARLY': '1'}, {'FT_STAGED_BACKWARD': '0'}, {'FT_PRED_STAGE_FIRST': '0'},
                 {'FT_WGRAD_LATE': '0'}, {'FT_WGRAD_CUS': '0'}, {'FT_BIAS_GRADS_SIDE': '0'}, {'FT_WGRAD_DEFER': '0'},
                 {'FT_PRED_STAGE_FIRST': '1'}]


def scenario_e(tr):
    from forwardtacotron_amd.model import ForwardTacotron
    M = load_npz('tiny_model.npz')

    def make():
        m = ForwardTacotron(**TINY)
        m.load_state_dict(sub(M, 'sd/'))
        return m.cuda()
    for switches in STEP_SWITCHES:
        train_steps(tr, 'E train steps', make, sub(M, 'batch/'), TRAIN_CFG, switches)


def scenario_f(tr):
    from forwardtacotron_amd.multi_model import MultiForwardTacotron
    M = load_npz('tiny_multi.npz')

    def make():
        m = MultiForwardTacotron(**TINY_MULTI)
        m.load_state_dict(sub(M, 'sd/'))
        return m.cuda()
    train_steps(tr, 'F train steps', make, sub(M, 'batch/'), TRAIN_CFG_MULTI)


def scenario_g(tr):
    from forwardtacotron_amd.fastpitch import FastPitch
    Z = load_npz('tiny_fastpitch.npz')

    def tiny():
        m = FastPitch(**TINY_FP)
        m.load_state_dict(fp_state(Z, 'sd/'))
        return m.cuda()
    train_steps(tr, 'G train steps tiny fp32', tiny, sub(Z, 'batch/'), TRAIN_CFG)
    train_steps(tr, 'G train steps tiny fp32', tiny, sub(Z, 'batch/'), TRAIN_CFG, {'FT_TRANSFORMER_NODE': '1'})
    cfg = production_fastpitch()[0]
    batch = data.synthetic_batch(B=2, Tmax=16, n_mels=cfg['n_mels'], max_dur=6, seed=3)

    def wide():
        m = production_fastpitch()[1]
        m.matmul_dtype = 'bf16'
        return m
    train_steps(tr, 'G train steps bf16 composite', wide, batch, TRAIN_CFG)
    train_steps(tr, 'G train steps bf16 composite', wide, batch, TRAIN_CFG, {'FT_FFT_SUMS_STREAM': '1'})


SCENARIOS = {'A': scenario_a, 'B': scenario_b, 'C': scenario_c, 'D': scenario_d, 'E': scenario_e, 'F': scenario_f,
             'G': scenario_g}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', required=True)
    ap.add_argument('--only', default='A,B,C,D,E,F,G')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('call_trace: needs an MI355X (no CPU fallback)')
    _lib.lib()
    tr = Trace()
    for key in a.only.split(','):
        torch.manual_seed(0)
        SCENARIOS[key](tr)
    with open(a.out, 'w') as f:
        f.write('\n'.join(canonical(tr.lines)) + '\n')
    print(f'{a.out}: {len(tr.lines)} lines')


if __name__ == '__main__':
    main()
