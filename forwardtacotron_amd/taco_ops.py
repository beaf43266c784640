"""Differentiable ops of the Tacotron teacher's training forward (Tacotron.forward_train).

As in ops.py each op is a torch.autograd.Function whose forward and backward are sequences of hand-written gfx950
kernels; the two recurrences here have their backward in csrc/ft_taco_train.hip.  Without a
gradient sink installed (the teacher has no flat-buffer TrainStep) gradsink.emit returns fresh tensors and autograd
accumulates them into .grad, so the reference's own optimiser loop works on the result as it stands.
"""
import torch
from torch.autograd import Function

from . import _lib
from . import hip as H
from .gradsink import emit, emit_copies
from .hip import _p, _stream

_F4 = 4


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


class ZoneoutLSTMFn(Function):
    """nn.LSTMCell over the S steps of a time-major x [S,B,L] from zero states, with Decoder.zoneout on h
    (models/tacotron.py:119-122, 152-166): h_s = m_s h_{s-1} + (1 - m_s) cell(x_s, (h_{s-1}, c_{s-1})).h, the cell state
    is not zoned.  m = 1 where ft_dropout's mask of (p, seed) over [S,B,L] is 0; p = 0 zones nothing.  -> h [S,B,L]."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, p, seed):
        x = _c(x)
        xp = H.linear_fwd(x, w_ih, b_ih)                                    # [S,B,4L]
        gates, c, h = H.taco_lstm_zone_fwd(xp, w_hh, b_hh, float(p), int(seed))
        ctx.save_for_backward(x, gates, c, h, w_ih, w_hh, b_ih, b_hh)
        ctx.p, ctx.seed = float(p), int(seed)
        return h

    @staticmethod
    def backward(ctx, dout):
        x, gates, c, h, w_ih, w_hh, b_ih, b_hh = ctx.saved_tensors
        S, B, L = h.shape
        rows, G = S * B, 4 * L
        dxp = H.taco_lstm_zone_bwd(_c(dout), gates, c, H.transpose2d(w_hh), ctx.p, ctx.seed)
        dx = H.linear_bwd_data(dxp, w_ih) if ctx.needs_input_grad[0] else None
        dw_ih = emit(w_ih, lambda out: H.linear_bwd_weight_raw(dxp.data_ptr(), G, x.data_ptr(), L, out, rows, L, G),
                     (dxp, x))
        dw_hh = emit(w_hh, lambda out: H.linear_bwd_weight_raw(dxp.data_ptr(), G, h.data_ptr(), L, out, rows, L, G, B=B,
                                                               T=S, x_shift=-1, dy_tm=True, x_tm=True), (dxp, h))
        db_ih = emit(b_ih, lambda out: H.colsum_raw(dxp.data_ptr(), G, out, rows, G), (dxp,), heavy='light')
        db_hh = emit(b_hh, lambda out: H.colsum_raw(dxp.data_ptr(), G, out, rows, G), (dxp,), heavy='light')
        return dx, dw_ih, dw_hh, db_ih, db_hh, None, None


class TacoAttendFn(Function):
    """The teacher-forced attention recurrence (ft_taco_attend) with its BPTT (ft_taco_attend_bwd).
    pre [S,B,128] is the decoder prenet's output; P = pre W_ih[:, 256:]^T + b_ih is formed here so that
    attn_rnn.weight_ih gets ONE gradient [768,384]: columns :256 from the recurrence, 256: from this projection.
    -> (hist [S,B,512] of [context | h_attn], attn [B,S,Tx]); attn is returned non-differentiable (the reference's trainer
    only scores it, taco_trainer.py:100)."""

    @staticmethod
    def forward(ctx, ep, epq, pre, w_ih, b_ih, w_hh, b_hh, W, bW, cw, L, bL, v):
        ep, epq, pre = _c(ep), _c(epq), _c(pre)
        B, Tx, D = ep.shape
        S = pre.shape[0]
        w_pre = H.slice_cols(w_ih.detach()[None], D, w_ih.shape[1] - D)[0]      # W_ih[:, 256:]
        P = H.linear_fwd(pre, w_pre, b_ih)                                      # [S,B,768]
        attn = torch.empty(B, S, Tx, device=ep.device, dtype=torch.float32)
        hist = torch.empty(S, B, 2 * D, device=ep.device, dtype=torch.float32)
        _lib.call('ft_taco_attend', _p(ep), _p(epq), _p(P), _p(w_ih), w_ih.shape[1], _p(w_hh), _p(b_hh), _p(W), _p(bW),
                  _p(cw), _p(L), _p(bL), _p(v), _p(attn), _p(hist), B, Tx, S,
                  *H.scratch('ft_taco_attend_workspace', B, Tx, device=ep.device), _stream())
        ctx.save_for_backward(ep, epq, pre, P, w_pre, hist, attn, w_ih, b_ih, w_hh, b_hh, W, bW, cw, L, bL, v)
        ctx.mark_non_differentiable(attn)
        return hist, attn

    @staticmethod
    def backward(ctx, dhist, _dattn):
        ep, epq, pre, P, w_pre, hist, attn, w_ih, b_ih, w_hh, b_hh, W, bW, cw, L, bL, v = ctx.saved_tensors
        S, B, G = P.shape
        D = ep.shape[2]
        Cp = w_pre.shape[1]
        g = H.taco_attend_bwd(ep, epq, P, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v, hist, attn, _c(dhist))
        dP = g['dP']
        dpre = H.linear_bwd_data(dP, w_pre) if ctx.needs_input_grad[2] else None

        def wih_grad(out):
            dw_pre = torch.empty(G, Cp, device=dP.device, dtype=torch.float32)
            H.linear_bwd_weight_raw(dP.data_ptr(), G, pre.data_ptr(), Cp, dw_pre, S * B, Cp, G)
            H.copy_segments([H.concat_cols(g['dw_ih_ctx'][None], dw_pre[None], None, 1, G)], [out])

        dw_ih = emit(w_ih, wih_grad, (dP, pre))
        db_ih = emit(b_ih, lambda out: H.colsum_raw(dP.data_ptr(), G, out, S * B, G), (dP,), heavy='light')
        small = emit_copies([w_hh, b_hh, W, bW, cw, L, bL, v],
                            [g['dw_hh'], g['db_hh'], g['dW'], g['dbW'], g['dcw'], g['dL'], g['dbL'], g['dv'].view_as(v)])
        return (g['dep'], g['depq'], dpre, dw_ih, db_ih, *small)


class PreNetLayerFn(Function):
    """One PreNet layer (models/tacotron.py:29-45): dropout(relu(x W^T + b), p) over the last dim, with ft_dropout's
    counter-based mask of (p, seed) over the output in its storage order; p = 0 draws nothing."""

    @staticmethod
    def forward(ctx, x, w, b, p, seed):
        x = _c(x)
        y = H.linear_fwd(x, w, b, relu=True)
        if p > 0:
            y = H.dropout(y, float(p), int(seed))
        ctx.save_for_backward(x, y, w, b)
        ctx.p = float(p)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, w, b = ctx.saved_tensors
        out_f, in_f = w.shape
        rows = x.numel() // in_f
        dz = H.relu_dropout_bwd(_c(dy), y, ctx.p)
        dx = H.linear_bwd_data(dz, w) if ctx.needs_input_grad[0] else None
        dw = emit(w, lambda out: H.linear_bwd_weight_raw(dz.data_ptr(), out_f, x.data_ptr(), in_f, out, rows, in_f,
                                                         out_f), (dz, x))
        db = emit(b, lambda out: H.colsum_raw(dz.data_ptr(), out_f, out, rows, out_f), (dz,), heavy='light')
        return dx, dw, db, None, None


class MelProjFn(Function):
    """mel_proj restricted to the n_mels * r rows the [:, :, :r] slice keeps (models/tacotron.py:169-170): x [S,B,L] ->
    [S,B,r*n_mels] in the order k * n_mels + n; the weight gradient is scattered back into the full [n_mels*max_r, L]
    shape, exact zeros in the dropped rows."""

    @staticmethod
    def forward(ctx, x, w, n_mels, max_r, r):
        x = _c(x)
        wp = H.bt_transpose(w.detach().reshape(n_mels, max_r, -1), True)[:r].reshape(r * n_mels, -1)
        ctx.save_for_backward(x, wp, w)
        ctx.dims = (int(n_mels), int(max_r), int(r))
        return H.linear_fwd(x, wp)

    @staticmethod
    def backward(ctx, dy):
        x, wp, w = ctx.saved_tensors
        n_mels, max_r, r = ctx.dims
        dy = _c(dy)
        L = x.shape[-1]
        rows = x.numel() // L
        dx = H.linear_bwd_data(dy, wp) if ctx.needs_input_grad[0] else None

        def wgrad(out):
            dwp = torch.empty_like(wp)
            H.linear_bwd_weight_raw(dy.data_ptr(), r * n_mels, x.data_ptr(), L, dwp, rows, L, r * n_mels)
            H.taco_mel_scatter(dwp, out, n_mels, max_r, r)

        return dx, emit(w, wgrad, (dy, x)), None, None, None


class AddFn(Function):
    """x + y (the decoder's residual adds)"""

    @staticmethod
    def forward(ctx, x, y):
        x, y = _c(x), _c(y)
        out = torch.empty_like(x)
        _lib.call('ft_taco_add', _p(x), _p(y), _p(out), x.numel(), _stream())
        return out

    @staticmethod
    def backward(ctx, dout):
        return dout, dout
