"""One statement of the Tacotron decoder's per-step math, from raw operands (no state dict), generic over dtype and
device: the reference of the kernel-level tests of csrc/ft_taco.hip (tests/test_gpu_taco_kernels.py) and the per-step
body of tests/taco_cpu.py (forward) and tests/taco_gen_cpu.py (generate), whose golden tests tie it to the reference's
recorded fixtures.

  attend step   h = GRUCell(ctx W_ih[:, :D]^T + P[s], h)      P[s] = prenet half of the input projection + b_ih
                loc = conv1d([cum, att], cw, padding 15); e = v . tanh(W h + bW + ep + L loc + bL)
                att = softmax_Tx(e); cum += att; ctx = att @ epq              history row = [ctx | h]
  generate step P[s] = W_ih[:, D:] relu(W2 relu(W1 f + b1) + b2) + b_ih, f = the last frame of step s-1 (zeros at 0)
                attend step; x = Wi [ctx | h] + bi; x += LSTMCell1(x); x += LSTMCell2(x)
                frames s*r + k, k < r: channel n = (Wm x)[n * 20 + k]
"""
import torch
import torch.nn.functional as F

MAX_R = 20


def gru_cell(gx, h, w_hh, b_hh):
    """gates r, z, n; h' = (1 - z) n + z h"""
    Hd = h.shape[1]
    gh = h @ w_hh.t() + b_hh
    r = torch.sigmoid(gx[:, :Hd] + gh[:, :Hd])
    z = torch.sigmoid(gx[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
    n = torch.tanh(gx[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
    return (1 - z) * n + z * h


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """gate order i, f, g, o -> (h', c')"""
    g = x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    i, f, gg, o = g.chunk(4, dim=1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def attend_state(ep):
    """zero (h, ctx, cum, att) for ep [B,Tx,D]"""
    B, Tx, D = ep.shape
    return ep.new_zeros(B, D), ep.new_zeros(B, D), ep.new_zeros(B, Tx), ep.new_zeros(B, Tx)


def attend_step(state, Ps, ep, epq, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v):
    """one step: state (h, ctx, cum, att), Ps [B,3D] -> the next state"""
    h, ctx, cum, att = state
    D = w_hh.shape[1]
    h = gru_cell(ctx @ w_ih[:, :D].t() + Ps, h, w_hh, b_hh)
    loc = F.conv1d(torch.stack([cum, att], 1), cw, padding=cw.shape[2] // 2).transpose(1, 2)
    e = torch.tanh((h @ W.t() + bW)[:, None, :] + ep + loc @ L.t() + bL) @ v
    att = torch.softmax(e, dim=1)
    cum = cum + att
    ctx = (att[:, None, :] @ epq)[:, 0]
    return h, ctx, cum, att


def attend(ep, epq, P, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v):
    """ep, epq [B,Tx,D], P [S,B,3D] (b_ih included), w_ih [3D, >= D] (only [:, :D] is used), v [D]
    -> attn [B,S,Tx], hist [S,B,2D] with rows [context | h]"""
    state = attend_state(ep)
    attns, hist = [], []
    for s in range(P.shape[0]):
        state = attend_step(state, P[s], ep, epq, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v)
        attns.append(state[3])
        hist.append(torch.cat([state[1], state[0]], 1))
    return torch.stack(attns, 1), torch.stack(hist, 0)


def gen_steps(ep, epq, fc1_w, fc1_b, fc2_w, fc2_b, w_ih, b_ih, w_hh, b_hh, W, bW, cw, L, bL, v, rnn_in_w, rnn_in_b,
              lstm1, lstm2, mel_w, r, S, stop_threshold=None):
    """B = 1: ep, epq [1,Tx,D]; lstm1, lstm2 = (w_ih, w_hh, b_ih, b_hh); mel_w [n_mels * 20, L]
    -> (P [S',3D], hist [S',2D], attn [S',Tx], frames [S'*r, n_mels], smax [S'] the largest of each step's n_mels * r
    values).  S' = S, or with stop_threshold (a tensor or a number) the step count after the first step s with every
    value below it and s * r > 10, tested on the host step by step as the reference does."""
    D = w_hh.shape[1]
    Ld = lstm1[1].shape[1]
    n_mels = mel_w.shape[0] // MAX_R
    state = attend_state(ep)
    h1 = c1 = h2 = c2 = ep.new_zeros(1, Ld)
    f = ep.new_zeros(1, n_mels)
    Ps, hist, attns, frames = [], [], [], []
    for s in range(S):
        p = torch.relu(f @ fc1_w.t() + fc1_b)
        p = torch.relu(p @ fc2_w.t() + fc2_b)
        Pr = p @ w_ih[:, D:D + p.shape[1]].t() + b_ih
        state = attend_step(state, Pr, ep, epq, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v)
        hrow = torch.cat([state[1], state[0]], 1)
        xm = hrow @ rnn_in_w.t() + rnn_in_b
        h1, c1 = lstm_cell(xm, h1, c1, *lstm1)
        xm = xm + h1
        h2, c2 = lstm_cell(xm, h2, c2, *lstm2)
        xm = xm + h2
        mel = (xm @ mel_w.t()).view(1, n_mels, MAX_R)[:, :, :r]
        f = mel[:, :, -1]
        Ps.append(Pr[0])
        hist.append(hrow[0])
        attns.append(state[3][0])
        frames.append(mel[0].t())
        if stop_threshold is not None and bool((mel < stop_threshold).all()) and s * r > 10:   # host sync per step
            break
    frames = torch.cat(frames, 0)
    smax = frames.reshape(len(Ps), -1).amax(1)
    return torch.stack(Ps), torch.stack(hist), torch.stack(attns), frames, smax
