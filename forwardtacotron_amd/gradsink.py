"""The gradient sink of the train step: who writes which parameter's gradient, on which stream, and when the all-reduce
hears about it.  Installed by trainer.TrainStep; absent = plain autograd semantics."""
# Every parameter of the model receives exactly one gradient contribution per backward pass, so the weight-gradient
# kernels can write STRAIGHT into the trainer's flat gradient buffer (no temporary, no AccumulateGrad add) and the
# backward returns None for that input.  Weight gradients are off the critical data-gradient chain, so with a sink the
# GEMM-shaped ones are issued on a second HIP stream and overlap the latency-bound persistent recurrences; the trainer
# joins that stream before the optimiser.
#
# A slot's life: open -> claimed (`claim`: taken, and owed if its launch comes later) -> issued -> announced (`announce`:
# no longer owed, the reducer is told) -> joined (`join`, the end of the step).  Everything else here -- the emit forms,
# the queue of a deferring sink, the late list -- is built from those two primitives, and `route` alone decides which
# way an emission goes.
from typing import NamedTuple, Optional

import torch
from torch import cuda as _cuda      # the three things the sink needs of it: current_stream, stream(), Stream.wait_stream

from . import hip as H

INLINE, SIDE_NOW, SIDE_QUEUED, LATE = 'inline', 'side-now', 'side-queued', 'late'


class Policy(NamedTuple):
    """what a step lets the sink do (GradSink.set_policy, once per step)"""
    # weight-gradient GEMMs whose operands have at most this many rows stay on the CURRENT stream (0: none do).
    # ForwardTacotron sets it to its token-side row count: those gradients (prenet, predictors) only become
    # computable at the very end of the backward, right after the first LSTM's four big weight gradients landed
    # on the side stream -- left there they queue behind them while the main stream has nothing left to do
    # (1.9 ms of a 28.4 ms step); on the main stream the two tails overlap.  FastPitch, whose whole token side
    # is launch-bound, is faster with everything on the side stream and leaves it at 0.
    inline_rows: int = 0
    # defer = True: side-stream weight gradients are not launched where they are emitted but queued, and launched
    # in one go right before the next recurrence's BPTT kernel (flush_begin / flush_end) -- the persistent recurrences
    # leave most of the chip idle, while between them the main stream's own GEMM / BatchNorm chain wants it all
    defer: bool = False
    # late_ok: weight gradients emitted with late=True are not sent to the side stream but run on the step's MAIN stream at
    # the very end of the backward (flush_all) -- with the predictors' stage out of the tail the main stream finishes its
    # chain 0.8 ms before the side stream has worked off the LSTM's four weight gradients; one of the four rebalances the two.
    late_ok: bool = False
    # FT_BIAS_GRADS_SIDE: 'light' emissions (bias-gradient column sums) join the queued side-stream launches
    bias_side: bool = True


def route(heavy, late: bool, inline_ok: bool, rows: int, has_deps: bool, policy: Policy) -> str:
    """Which way an emission goes.  heavy: True (a GEMM-shaped weight gradient), False, or 'light' -- a small reduction
    (bias gradient) that nothing on the step's critical stream waits for: it joins the queued side-stream launches of a
    deferring sink (22 column sums + finalizes = 0.4 ms of the ForwardTacotron step's main stream) and stays inline
    otherwise.  rows: the row count of the first operand (see Policy.inline_rows; inline_ok=False: exempt from it)."""
    if late and policy.late_ok and policy.defer:
        return LATE
    if heavy == 'light':
        heavy = policy.defer and has_deps and policy.bias_side
    if not heavy or (inline_ok and has_deps and rows <= policy.inline_rows):
        return INLINE
    return SIDE_QUEUED if policy.defer else SIDE_NOW


class GradSink:
    """Facts about the schedule that callers rely on (none of them is a promise to keep):
    - a side launch that is NOT deferred is announced with the EMITTING stream current: `used` and the reducer record
      the emitting stream, not the side stream.  The side stream is covered because the trainer registers it with the
      reducer and `join` always waits for it.
    - flush_end announces after the last compute, outside the side-stream context (the reducer sees the flusher's stream),
      and records nothing in `used`.
    - late gradients run on the stream that is current where flush_all is called.
    - 'light' emissions go to the side stream only when deferring AND with deps.
    - a second emitter of one parameter finds the slot taken and gets a fresh tensor (autograd accumulates it); of several
      parameters emitted together, one taken slot makes ALL of them fresh tensors."""

    def __init__(self, views, stream=None, on_write=None, reducer_streams=None):
        self.views = views              # {param.data_ptr(): (index, grad view tensor)}
        self.stream = stream            # side stream for weight-gradient GEMMs (None: current stream)
        self.on_write = on_write        # callback(index) -> lets the bucketed all-reduce count arrivals
        # the set of streams a gradient bucket's all-reduce waits for (None: no reducer); see wrote_on
        self.reducer_streams = reducer_streams
        self.policy = Policy()
        self.written = set()            # slots taken this step
        self.held = set()               # claimed, not yet issued: the sink owes them (the all-reduce must wait)
        self.pending = []               # queued side launches: (compute, views, deps, indices, emitting stream)
        self.late = []                  # (compute, views, deps, indices), see Policy.late_ok
        self.used = set()               # streams gradient writes were issued on this step
        # operands of side-stream launches, kept REFERENCED until the step has joined the side stream.  record_stream only
        # keeps their memory from being recycled; it does not keep autograd from ADDING INTO them: a gradient tensor handed
        # to two consumers (LayerNorm's dx for branch and residual, AddBackward's grad for both addends) is accumulated
        # in place -- on the emitting stream -- as soon as it is uniquely owned, i.e. right after the conv / linear node
        # whose weight gradient is still reading it on the side stream has returned (seen as rare wrong conv2 weight
        # gradients in MultiFastPitch's predictors).  A live reference makes autograd add out of place instead.
        self.keep = []

    def set_policy(self, inline_rows: int = 0, defer: bool = False, late_ok: bool = False, bias_side: bool = True) -> None:
        self.policy = Policy(int(inline_rows), bool(defer), bool(late_ok), bool(bias_side))

    def begin_step(self) -> None:
        for s in (self.written, self.held, self.pending, self.late, self.used, self.keep):
            s.clear()

    # -- the two primitives ---------------------------------------------------------------------------------------
    def open_slot(self, w: torch.Tensor):
        """(index, view) of w's slot if it has one that is still untaken this step, else None; takes nothing"""
        ent = self.views.get(w.data_ptr())
        return None if ent is None or ent[0] in self.written else ent

    def claim(self, w: torch.Tensor, owed: bool = False):
        """(index, view) of w's slot in the flat gradient buffer, now taken -- or None if w has no slot or it was taken
        earlier this step.  owed: the launch comes later; the reducer hears about the slot only through announce."""
        ent = self.open_slot(w)
        if ent is None:
            return None
        self.written.add(ent[0])
        if owed:
            self.held.add(ent[0])
        return ent

    def announce(self, idxs, streams=None) -> None:
        """The writes of these slots have been issued, on `streams` (None: on the current one).  The one place that tells
        the reducer -- which itself notes the stream that is current HERE."""
        # Autograd only joins the streams on which it accumulated a leaf gradient itself, and the sink's parameters never
        # get there, so whoever applies the gradients must wait for every stream recorded here (a predictor's backward
        # runs on the predictor side stream).
        self.used.update((_cuda.current_stream(),) if streams is None else streams)
        for i in idxs:
            self.held.discard(i)
            if self.on_write is not None:
                self.on_write(i)

    # -- what outsiders may ask and tell ----------------------------------------------------------------------------
    def owes(self, idx: int) -> bool:
        """claimed but not yet issued: the sink announces it itself"""
        return idx in self.held

    def hold(self, obj) -> None:
        """keep `obj` (operands of launches on another stream) referenced until the step has joined (see `keep`)"""
        self.keep.append(obj)

    def wrote_on(self, stream, tell_reducer: bool = False) -> None:
        """`stream` also carried gradient writes: the step's join waits for it and, with tell_reducer, so does every
        bucket's all-reduce from now on"""
        self.used.add(stream)
        if tell_reducer and self.reducer_streams is not None:
            self.reducer_streams.add(stream)

    def join(self, cur) -> None:
        """end of the backward: `cur` waits for the side stream and every stream gradients were written on"""
        cur.wait_stream(self.stream)
        for st in self.used:               # e.g. the predictors' side stream: its backward wrote gradients too
            if st != cur and st != self.stream:
                cur.wait_stream(st)
        self.keep.clear()                  # joined: nothing reads the side launches' operands any more

    # -- emission ---------------------------------------------------------------------------------------------------
    def _emit(self, ws, many: bool, compute, deps, heavy, late: bool, inline_ok: bool) -> None:
        rows = deps[0].numel() // deps[0].shape[-1] if deps else 0
        how = route(heavy if self.stream is not None else False, late, inline_ok, rows, bool(deps), self.policy)
        ents = [self.claim(w, owed=how in (SIDE_QUEUED, LATE)) for w in ws]
        idxs = tuple(e[0] for e in ents)
        views = [e[1] for e in ents] if many else ents[0][1]
        if how == INLINE:
            compute(views)
            self.announce(idxs)
        elif how == LATE:
            self.late.append((compute, views, deps, idxs))
        elif how == SIDE_QUEUED:
            # The operands are complete once the EMITTING stream gets here, and the flush may run on another stream (a
            # predictor's recurrence on its side stream flushes gradients the main stream emitted): the item remembers its
            # stream and the flush makes the side stream wait for that stream's position AT FLUSH TIME -- one join per
            # (flush, emitting stream), however many items; a variant with one event per item measured 1.2 ms slower.
            self.pending.append((compute, views, deps, idxs, _cuda.current_stream()))
        else:
            here = _cuda.current_stream()
            self.stream.wait_stream(here)
            with _cuda.stream(self.stream):
                compute(views)
            # the operands stay referenced until the step has joined the side stream (`keep`): nothing can recycle or
            # overwrite them under the side stream, and no record_stream bookkeeping is needed
            self.keep.append(deps)
            self.announce(idxs, (here,))

    # -- the queue of a deferring sink ------------------------------------------------------------------------------
    def flush_begin(self):
        """First half of a flush: joins the side stream with the emitting streams NOW (so that it does not wait for
        whatever the caller launches next) and hands back the queued launches; flush_end issues them.  A recurrence's
        backward calls flush_begin, launches its BPTT kernel, then flush_end: the persistent kernel (all of whose workgroups
        must become co-resident) is dispatched before the GEMMs that would otherwise fill every CU's registers first."""
        if not self.pending:
            return None
        pend, self.pending = self.pending, []
        seen = []
        for item in pend:
            if item[4] not in seen:
                seen.append(item[4])
                self.stream.wait_stream(item[4])
        return pend

    def flush_end(self, pend) -> None:
        if not pend:
            return
        with _cuda.stream(self.stream):
            for compute, views, deps, _, _ in pend:
                compute(views)
                self.keep.append(deps)
        for item in pend:
            self.announce(item[3], ())

    def flush_all(self) -> None:
        """issue every queued side-stream weight gradient, then the ones kept for the end of the main stream's chain"""
        self.flush_end(self.flush_begin())
        late, self.late = self.late, []
        for compute, views, deps, idxs in late:
            compute(views)
            self.keep.append(deps)
            self.announce(idxs)


# ---------------------------------------------------------------------------------------------------
# The installed sink: autograd Functions reach it through this process-wide slot.
# ---------------------------------------------------------------------------------------------------
_SINK: Optional[GradSink] = None


def install(sink: Optional[GradSink]) -> None:
    global _SINK
    _SINK = sink


def installed() -> Optional[GradSink]:
    return _SINK


def emit(w, compute, deps=(), heavy=True, late: bool = False, inline_ok: bool = True):
    """Produces the gradient of parameter `w`, or of a list of parameters whose gradients one launch produces together:
    compute(out) must overwrite `out` (same shape as w; a list of them for a list).  Without a sink, or with one of the
    slots taken: returns fresh tensors (autograd accumulates them).  With a sink: writes the flat-buffer views -- where
    and when `route` says -- and returns None (a list of them).  deps: the operands, deps[0] the one whose rows count."""
    many = isinstance(w, (list, tuple))
    ws = w if many else (w,)
    sink = _SINK
    if sink is None or any(sink.open_slot(x) is None for x in ws):
        outs = [torch.empty_like(x) for x in ws]
        compute(outs if many else outs[0])
        return outs if many else outs[0]
    sink._emit(ws, many, compute, deps, heavy, late, inline_ok)
    return [None] * len(ws) if many else None


def emit_copies(ws, values):
    """Small vector gradients that a fused kernel already produced in `values`: one copy launch for all the slots the sink
    still has open; the others come back as they are."""
    sink = _SINK
    ents = [sink.claim(w) if sink is not None else None for w in ws]
    todo = [(e, v) for e, v in zip(ents, values) if e is not None]
    if todo:
        H.copy_segments([v for _, v in todo], [e[1] for e, _ in todo])
        sink.announce([e[0] for e, _ in todo])
    return [v if e is None else None for e, v in zip(ents, values)]


def claim(w: torch.Tensor):
    """GradSink.claim on the installed sink (None without one): for a kernel that writes the slot itself, on the current
    stream; the caller announces the index once that kernel is issued"""
    return _SINK.claim(w) if _SINK is not None else None


def flush_begin():
    """GradSink.flush_begin of the installed sink (None: no sink, or nothing queued)"""
    return _SINK.flush_begin() if _SINK is not None else None


def flush_end(pend) -> None:
    if pend:
        _SINK.flush_end(pend)


class batched_side_launches:
    """`with batched_side_launches():` -- the side-stream weight gradients (and 'light' bias-gradient sums) emitted inside
    are queued and issued together at the end: ONE stream join and ONE stream switch for the lot instead of one per
    parameter (a FastPitch step emitted 88 of them one by one: 3.2 ms of host time in torch's stream calls).  No-op
    without a sink or when the sink defers already (recurrent models flush before their BPTT kernels instead)."""

    def __enter__(self):
        self.sink = _SINK if _SINK is not None and not _SINK.policy.defer else None
        if self.sink is not None:
            self.sink.policy = self.sink.policy._replace(defer=True)
        return self

    def __exit__(self, *exc):
        if self.sink is not None:
            self.sink.flush_end(self.sink.flush_begin())
            self.sink.policy = self.sink.policy._replace(defer=False)
        return False
