"""The gradient sink's host-side schedule (forwardtacotron_amd.gradsink) without a device: which compute runs on which
stream, which stream waits for which, and when the reducer hears of a slot.  The sink needs three things of torch.cuda
-- the current stream, a stream context and Stream.wait_stream -- and gets fakes that write an event log:
('wait', waiter, waited), ('switch', stream) on entering a stream context, ('run', tag, current stream), ('copy', number
of segments, current) for the one kernel the copy form launches, and ('announce', index, current) from on_write.
Every scenario asserts the whole log and the sink's sets after every phase; the logs were recorded on the code as it
was before the sink had a module of its own (five hand-written copies of the bookkeeping) and must stay as they are."""
import contextlib
import itertools

import pytest
import torch

from forwardtacotron_amd import gradsink
from forwardtacotron_amd.gradsink import GradSink, Policy, emit, emit_copies


class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(('wait', self.name, other.name))

    def __repr__(self):
        return self.name


class FakeCuda:
    def __init__(self, log, names):
        self.log = log
        self.streams = {n: FakeStream(n, log) for n in names}
        self.cur = self.streams[names[0]]

    def current_stream(self):
        return self.cur

    @contextlib.contextmanager
    def stream(self, s):
        self.log.append(('switch', s.name))
        prev, self.cur = self.cur, s
        try:
            yield
        finally:
            self.cur = prev


class Bench:
    """a sink over `n` two-element parameters with the fakes in place: main is current, side is the sink's stream"""

    def __init__(self, monkeypatch, n, installed=True, **policy):
        self.log = []
        self.cuda = FakeCuda(self.log, ['main', 'side', 'pred'])
        self.main, self.side, self.pred = (self.cuda.streams[k] for k in ('main', 'side', 'pred'))
        monkeypatch.setattr(gradsink, '_cuda', self.cuda)
        monkeypatch.setattr(gradsink.H, 'copy_segments',
                            lambda src, dst: self.log.append(('copy', len(src), self.cuda.cur.name)))
        self.ws = [torch.zeros(2) for _ in range(n)]
        self.views = [torch.zeros(2) for _ in range(n)]
        self.got = {}                                   # tag -> what compute was handed
        self.reducer_streams = set()
        self.sink = GradSink({w.data_ptr(): (i, v) for i, (w, v) in enumerate(zip(self.ws, self.views))},
                             stream=self.side, on_write=lambda i: self.log.append(('announce', i, self.cuda.cur.name)),
                             reducer_streams=self.reducer_streams)
        self.sink.set_policy(**policy)
        self.sink.begin_step()
        if installed:
            gradsink.install(self.sink)

    def run(self, tag):
        def compute(out):
            self.got[tag] = out
            self.log.append(('run', tag, self.cuda.cur.name))
        return compute

    def take(self):
        """the events since the last look"""
        out, self.log[:] = list(self.log), []
        return out

    def sets(self):
        """(written, held, queued, late, kept, used) -- the sets as they are, the lists by length"""
        s = self.sink
        return (set(s.written), set(s.held), len(s.pending), len(s.late), len(s.keep), {st.name for st in s.used})


@pytest.fixture
def bench(monkeypatch):
    made = []

    def make(n, **kw):
        made.append(Bench(monkeypatch, n, **kw))
        return made[-1]
    yield make
    gradsink.install(None)


ROWS8, ROWS4 = torch.zeros(8, 3), torch.zeros(4, 3)


def test_the_four_routes_in_one_deferring_step(bench):
    b = bench(4, defer=True, late_ok=True, inline_rows=4)
    assert emit(b.ws[0], b.run(0), (ROWS8,)) is None
    assert emit(b.ws[1], b.run(1), (ROWS8,), late=True) is None
    assert emit(b.ws[2], b.run(2), (ROWS8,), heavy='light') is None
    assert b.take() == [] and b.sets() == ({0, 1, 2}, {0, 1, 2}, 2, 1, 0, set())
    assert emit(b.ws[3], b.run(3), (ROWS4,)) is None
    assert b.take() == [('run', 3, 'main'), ('announce', 3, 'main')]
    assert b.sets() == ({0, 1, 2, 3}, {0, 1, 2}, 2, 1, 0, {'main'})
    assert [b.sink.owes(i) for i in range(4)] == [True, True, True, False]
    b.sink.flush_all()
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 0, 'side'), ('run', 2, 'side'),
                        ('announce', 0, 'main'), ('announce', 2, 'main'), ('run', 1, 'main'), ('announce', 1, 'main')]
    assert b.sets() == ({0, 1, 2, 3}, set(), 0, 0, 3, {'main'})
    assert all(b.got[i] is b.views[i] for i in range(4))
    b.sink.begin_step()
    assert b.sets() == (set(), set(), 0, 0, 0, set())


def test_recurrent_shape_flush_around_a_launch_from_another_stream(bench):
    """emissions from two streams; flush_begin -> the recurrence's launch -> flush_end on the second stream: one wait per
    (flush, emitting stream) in first-seen order, the computes in queue order BEHIND the launch, the announcements only
    after the last compute -- on the flusher's stream, and `used` hears nothing of them"""
    b = bench(4, defer=True)
    emit(b.ws[0], b.run(0), (ROWS8,))
    with b.cuda.stream(b.pred):
        emit(b.ws[1], b.run(1), (ROWS8,))
    emit(b.ws[2], b.run(2), (ROWS8,))
    assert b.take() == [('switch', 'pred')] and b.sets() == ({0, 1, 2}, {0, 1, 2}, 3, 0, 0, set())
    with b.cuda.stream(b.pred):
        pend = gradsink.flush_begin()
        assert b.sets() == ({0, 1, 2}, {0, 1, 2}, 0, 0, 0, set())
        b.run('bptt')(None)
        gradsink.flush_end(pend)
    assert b.take() == [('switch', 'pred'), ('wait', 'side', 'main'), ('wait', 'side', 'pred'), ('run', 'bptt', 'pred'),
                        ('switch', 'side'), ('run', 0, 'side'), ('run', 1, 'side'), ('run', 2, 'side'),
                        ('announce', 0, 'pred'), ('announce', 1, 'pred'), ('announce', 2, 'pred')]
    assert b.sets() == ({0, 1, 2}, set(), 0, 0, 3, set())
    assert gradsink.flush_begin() is None                   # nothing queued: no join, and flush_end takes it
    gradsink.flush_end(None)
    emit(b.ws[3], b.run(3), (ROWS8,))
    b.sink.flush_all()
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 3, 'side'), ('announce', 3, 'main')]
    assert b.sets() == ({0, 1, 2, 3}, set(), 0, 0, 4, set())


def test_fastpitch_shape_one_by_one_and_batched(bench):
    b = bench(15)
    emit(b.ws[0], b.run(0), (ROWS8,))
    emit(b.ws[1], b.run(1), (ROWS8,))
    emit(b.ws[2], b.run(2), (ROWS8,), heavy='light')        # not deferring: a bias sum stays where it is emitted
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 0, 'side'), ('announce', 0, 'main'),
                        ('wait', 'side', 'main'), ('switch', 'side'), ('run', 1, 'side'), ('announce', 1, 'main'),
                        ('run', 2, 'main'), ('announce', 2, 'main')]
    assert b.sets() == ({0, 1, 2}, set(), 0, 0, 2, {'main'})
    with gradsink.batched_side_launches():
        for i in range(3, 15):                              # six weight gradients, six bias sums
            emit(b.ws[i], b.run(i), (ROWS8,), heavy=True if i % 2 else 'light')
        assert b.take() == [] and b.sets() == (set(range(15)), set(range(3, 15)), 12, 0, 2, {'main'})
    assert b.take() == ([('wait', 'side', 'main'), ('switch', 'side')] + [('run', i, 'side') for i in range(3, 15)]
                        + [('announce', i, 'main') for i in range(3, 15)])
    assert b.sets() == (set(range(15)), set(), 0, 0, 14, {'main'})
    assert b.sink.policy == Policy()


def test_batching_inside_a_deferring_sink_changes_nothing(bench):
    b = bench(2, defer=True)
    with gradsink.batched_side_launches():
        emit(b.ws[0], b.run(0), (ROWS8,))
    assert b.take() == [] and b.sets() == ({0}, {0}, 1, 0, 0, set())
    assert b.sink.policy == Policy(defer=True)
    emit(b.ws[1], b.run(1), (ROWS8,))
    assert b.take() == [] and b.sets() == ({0, 1}, {0, 1}, 2, 0, 0, set())


def test_several_parameters_from_one_launch_and_the_copy_form(bench):
    b = bench(6)
    assert emit([b.ws[0], b.ws[1]], b.run('a'), (ROWS8,)) == [None, None]
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 'a', 'side'), ('announce', 0, 'main'),
                        ('announce', 1, 'main')]
    assert b.got['a'][0] is b.views[0] and b.got['a'][1] is b.views[1]
    assert b.sets() == ({0, 1}, set(), 0, 0, 1, {'main'})
    # one of the slots is taken: EVERY output comes back as a fresh tensor, nothing is claimed or announced
    outs = emit([b.ws[1], b.ws[2]], b.run('b'), (ROWS8,))
    assert b.take() == [('run', 'b', 'main')] and b.sets() == ({0, 1}, set(), 0, 0, 1, {'main'})
    assert all(torch.is_tensor(o) for o in outs) and outs[0] is b.got['b'][0] and outs[1] is b.got['b'][1]
    assert outs[1] is not b.views[2] and outs[1].shape == b.ws[2].shape
    assert emit([b.ws[2], b.ws[3]], b.run('c'), (ROWS8,), heavy='light') == [None, None]     # inline: not deferring
    assert b.take() == [('run', 'c', 'main'), ('announce', 2, 'main'), ('announce', 3, 'main')]
    vals = [torch.ones(2), torch.ones(2), torch.ones(2)]
    outs = emit_copies([b.ws[4], b.ws[0], b.ws[5]], vals)   # the taken slot's value is handed back
    assert outs[0] is None and outs[1] is vals[1] and outs[2] is None
    assert b.take() == [('copy', 2, 'main'), ('announce', 4, 'main'), ('announce', 5, 'main')]
    assert emit_copies([b.ws[4]], vals[:1]) == vals[:1] and b.take() == []
    assert b.sets() == (set(range(6)), set(), 0, 0, 1, {'main'})


def test_several_parameters_queued_in_a_deferring_sink(bench):
    b = bench(2, defer=True)
    assert emit([b.ws[0], b.ws[1]], b.run('a'), (ROWS8,), heavy='light') == [None, None]
    assert b.take() == [] and b.sets() == ({0, 1}, {0, 1}, 1, 0, 0, set())
    b.sink.flush_all()
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 'a', 'side'), ('announce', 0, 'main'),
                        ('announce', 1, 'main')]
    assert b.sets() == ({0, 1}, set(), 0, 0, 1, set())


def test_claim_and_announce_used_directly(bench):
    """as BatchNormConvFn (a kernel that writes the slots itself) and the FastPitch composite (claims for a whole stack,
    one C call, then hold / wrote_on / announce) use them, and the step's final join"""
    b = bench(3)
    e0 = gradsink.claim(b.ws[0])
    assert e0[0] == 0 and e0[1] is b.views[0] and gradsink.claim(b.ws[0]) is None
    assert gradsink.claim(torch.zeros(2)) is None           # not a parameter of the sink
    assert b.take() == [] and b.sets() == ({0}, set(), 0, 0, 0, set())
    gradsink.installed().announce([0])
    assert b.take() == [('announce', 0, 'main')] and b.sets() == ({0}, set(), 0, 0, 0, {'main'})
    assert b.sink.claim(b.ws[1], owed=True)[0] == 1 and b.sink.owes(1) and not b.sink.owes(0)
    assert b.sets() == ({0, 1}, {1}, 0, 0, 0, {'main'})
    b.sink.hold(('operands',))
    b.sink.wrote_on(b.side)
    b.sink.wrote_on(b.pred, tell_reducer=True)
    assert b.reducer_streams == {b.pred}
    with b.cuda.stream(b.pred):
        b.sink.announce([1], ())
    assert b.take() == [('switch', 'pred'), ('announce', 1, 'pred')]
    assert b.sets() == ({0, 1}, set(), 0, 0, 1, {'main', 'side', 'pred'})
    b.sink.join(b.main)
    assert b.take() == [('wait', 'main', 'side'), ('wait', 'main', 'pred')]
    assert b.sets() == ({0, 1}, set(), 0, 0, 0, {'main', 'side', 'pred'})


def test_no_sink_installed(bench):
    b = bench(2, installed=False)
    out = emit(b.ws[0], b.run(0), (ROWS8,))
    assert torch.is_tensor(out) and out is b.got[0] and out is not b.views[0] and out.shape == b.ws[0].shape
    outs = emit([b.ws[0], b.ws[1]], b.run(1), (ROWS8,), heavy='light')
    assert len(outs) == 2 and outs[0] is b.got[1][0] and outs[1] is b.got[1][1]
    vals = [torch.ones(2)]
    assert emit_copies([b.ws[0]], vals)[0] is vals[0]
    assert gradsink.claim(b.ws[0]) is None and gradsink.flush_begin() is None and gradsink.installed() is None
    gradsink.flush_end(None)
    with gradsink.batched_side_launches():
        emit(b.ws[0], b.run(2), (ROWS8,))
    assert b.take() == [('run', 0, 'main'), ('run', 1, 'main'), ('run', 2, 'main')]
    assert b.sets() == (set(), set(), 0, 0, 0, set())


def test_a_second_emitter_gets_a_fresh_tensor(bench):
    b = bench(1, defer=True)
    assert emit(b.ws[0], b.run(0), (ROWS8,)) is None
    out = emit(b.ws[0], b.run(1), (ROWS8,))
    assert torch.is_tensor(out) and out is b.got[1] and out is not b.views[0]
    assert b.take() == [('run', 1, 'main')] and b.sets() == ({0}, {0}, 1, 0, 0, set())


def test_edges_of_the_policy(bench):
    # late=True with late_ok off: an ordinary queued side launch
    b = bench(1, defer=True)
    emit(b.ws[0], b.run(0), (ROWS8,), late=True)
    assert b.take() == [] and b.sets() == ({0}, {0}, 1, 0, 0, set())
    # late_ok without defer: launched on the side stream at once
    b = bench(1, late_ok=True)
    emit(b.ws[0], b.run(0), (ROWS8,), late=True)
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 0, 'side'), ('announce', 0, 'main')]
    # FT_BIAS_GRADS_SIDE=0: a bias sum stays inline in a deferring sink
    b = bench(1, defer=True, bias_side=False)
    emit(b.ws[0], b.run(0), (ROWS8,), heavy='light')
    assert b.take() == [('run', 0, 'main'), ('announce', 0, 'main')] and b.sets() == ({0}, set(), 0, 0, 0, {'main'})
    # 'light' without deps: inline
    b = bench(1, defer=True)
    emit(b.ws[0], b.run(0), heavy='light')
    assert b.take() == [('run', 0, 'main'), ('announce', 0, 'main')] and b.sets() == ({0}, set(), 0, 0, 0, {'main'})
    # inline_ok=False at a row count at and below inline_rows: to the side stream all the same
    b = bench(2, inline_rows=8)
    emit(b.ws[0], b.run(0), (ROWS8,), inline_ok=False)
    emit(b.ws[1], b.run(1), (ROWS4,), inline_ok=False)
    assert b.take() == [('wait', 'side', 'main'), ('switch', 'side'), ('run', 0, 'side'), ('announce', 0, 'main'),
                        ('wait', 'side', 'main'), ('switch', 'side'), ('run', 1, 'side'), ('announce', 1, 'main')]
    # ... and with inline_ok at exactly inline_rows: inline
    b = bench(1, inline_rows=8)
    emit(b.ws[0], b.run(0), (ROWS8,))
    assert b.take() == [('run', 0, 'main'), ('announce', 0, 'main')]
    # a sink without a side stream does everything inline
    b = bench(1)
    b.sink.stream = None
    emit(b.ws[0], b.run(0), (ROWS8,))
    assert b.take() == [('run', 0, 'main'), ('announce', 0, 'main')]


def test_a_sink_used_without_a_trainer_has_the_default_policy():
    assert GradSink({}).policy == Policy(inline_rows=0, defer=False, late_ok=False, bias_side=True)


# route(): one letter per outcome -- I inline, N side stream now, Q side stream queued, L late.  A row is the eight
# combinations of (inline_ok, rows, has_deps) in the order of COLS, at inline_rows = 4; the rows are keyed by
# (defer, late_ok, bias_side), then (heavy, late).
COLS = [(ok, rows, deps) for ok in (False, True) for rows in (4, 8) for deps in (False, True)]
_NO_DEFER = {(True, False): 'NNNNNINN', (True, True): 'NNNNNINN', (False, False): 'IIIIIIII', (False, True): 'IIIIIIII',
             ('light', False): 'IIIIIIII', ('light', True): 'IIIIIIII'}
ROUTES = {
    (False, False, False): _NO_DEFER,
    (False, False, True): _NO_DEFER,
    (False, True, False): _NO_DEFER,
    (False, True, True): _NO_DEFER,
    (True, False, False): {(True, False): 'QQQQQIQQ', (True, True): 'QQQQQIQQ', (False, False): 'IIIIIIII',
                           (False, True): 'IIIIIIII', ('light', False): 'IIIIIIII', ('light', True): 'IIIIIIII'},
    (True, False, True): {(True, False): 'QQQQQIQQ', (True, True): 'QQQQQIQQ', (False, False): 'IIIIIIII',
                          (False, True): 'IIIIIIII', ('light', False): 'IQIQIIIQ', ('light', True): 'IQIQIIIQ'},
    (True, True, False): {(True, False): 'QQQQQIQQ', (True, True): 'LLLLLLLL', (False, False): 'IIIIIIII',
                          (False, True): 'LLLLLLLL', ('light', False): 'IIIIIIII', ('light', True): 'LLLLLLLL'},
    (True, True, True): {(True, False): 'QQQQQIQQ', (True, True): 'LLLLLLLL', (False, False): 'IIIIIIII',
                         (False, True): 'LLLLLLLL', ('light', False): 'IQIQIIIQ', ('light', True): 'LLLLLLLL'},
}
LETTER = {'I': gradsink.INLINE, 'N': gradsink.SIDE_NOW, 'Q': gradsink.SIDE_QUEUED, 'L': gradsink.LATE}


def test_route_over_the_full_product_of_its_inputs():
    assert len(ROUTES) == 8 and all(len(t) == 6 and all(len(r) == 8 for r in t.values()) for t in ROUTES.values())
    n = 0
    for defer, late_ok, bias_side in itertools.product((False, True), repeat=3):
        policy = Policy(inline_rows=4, defer=defer, late_ok=late_ok, bias_side=bias_side)
        for heavy, late in itertools.product((True, False, 'light'), (False, True)):
            row = ROUTES[(defer, late_ok, bias_side)][(heavy, late)]
            for (ok, rows, deps), letter in zip(COLS, row):
                got = gradsink.route(heavy, late, ok, rows, deps, policy)
                assert got == LETTER[letter], (policy, heavy, late, ok, rows, deps, got)
                n += 1
    assert n == 384
