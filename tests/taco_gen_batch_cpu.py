"""Restatement of Tacotron.generate_batch (forwardtacotron_amd/tacotron.py) from the math with stock torch ops, for the
tests (float64 on the host): the BATCHED decoder loop under the masking rule, on tests/taco_step_cpu.py's cells, with
the encoder and the postnet run with lengths.  tests/test_tacotron_generate_batch_cpu.py holds it to the reference's
generate of every sentence ALONE (tests/golden/tacotron_generate_batch.npz): that is the proof that the masking rule
equals "the item alone".

  masking rule, n = x_len[b]   energies e[b, t] for t < n only (-inf past it), softmax over t < n; attention and
                               cumulative exact zeros at t >= n, so the location conv (zero padding 15) sees at the
                               item's end what it sees at a sequence end; context = sum over t < n of p[t] eq[b, t]
                               (ep / eq rows at t >= n are replaced by NaN-free zeros and carry weight 0)
  stop rule, per item          s_out[b] = s + 1 at the first s with s * r > 10 and all 80 r values < stop_threshold;
                               S if there is none.  Stopped items are stepped on; their later slots are masked.
  CBHG with lengths            every stage that reads across time gets zeros at t >= n (what the item alone reads from
                               its zero padding) and the two GRU directions run over the item's own n rows
"""
import math

import torch
import torch.nn.functional as F

import taco_cpu as R
import taco_step_cpu as K

PAD_VALUE = -11.5129


def _mask(lens, T):
    """[B,T] bool: t < lens[b]"""
    return torch.arange(T)[None, :] < lens[:, None]


def cbhg_lens(x, lens, P, pre, Kb, num_highways):
    """x [B,C,T], zero at t >= lens[b] -> [B,T,2*channels], zero at t >= lens[b]"""
    B, _, T = x.shape
    m = _mask(lens, T)[:, None, :].to(x.dtype)
    bank = torch.cat([R._bnconv(x, P, f'{pre}conv1d_bank.{k}.', True) for k in range(Kb)], 1)
    prev = torch.cat([torch.full_like(bank[:, :, :1], -math.inf), bank[:, :, :-1]], 2)
    y = torch.maximum(bank, prev) * m
    y = R._bnconv(y, P, pre + 'conv_project1.', True) * m
    y = (R._bnconv(y, P, pre + 'conv_project2.', False) + x) * m
    y = y.transpose(1, 2) @ P[pre + 'pre_highway.weight'].t()
    for i in range(num_highways):
        hp = f'{pre}highways.{i}.'
        a = torch.relu(y @ P[hp + 'W1.weight'].t() + P[hp + 'W1.bias'])
        g = torch.sigmoid(y @ P[hp + 'W2.weight'].t() + P[hp + 'W2.bias'])
        y = g * a + (1 - g) * y
    rp = pre + 'rnn.'
    Hd = P[rp + 'weight_hh_l0'].shape[1]
    out = y.new_zeros(B, T, 2 * Hd)
    for b in range(B):
        n = int(lens[b])
        yb = y[b:b + 1, :n]
        out[b, :n, :Hd] = R._gru_seq(yb, P[rp + 'weight_ih_l0'], P[rp + 'weight_hh_l0'], P[rp + 'bias_ih_l0'],
                                     P[rp + 'bias_hh_l0'], False)[0]
        out[b, :n, Hd:] = R._gru_seq(yb, P[rp + 'weight_ih_l0_reverse'], P[rp + 'weight_hh_l0_reverse'],
                                     P[rp + 'bias_ih_l0_reverse'], P[rp + 'bias_hh_l0_reverse'], True)[0]
    return out


def attend_step_masked(state, Ps, ep, epq, valid, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v):
    """taco_step_cpu.attend_step under the masking rule; valid [B,Tx] bool"""
    h, ctx, cum, att = state
    D = w_hh.shape[1]
    h = K.gru_cell(ctx @ w_ih[:, :D].t() + Ps, h, w_hh, b_hh)
    loc = F.conv1d(torch.stack([cum, att], 1), cw, padding=cw.shape[2] // 2).transpose(1, 2)
    e = torch.tanh((h @ W.t() + bW)[:, None, :] + ep + loc @ L.t() + bL) @ v
    att = torch.softmax(e.masked_fill(~valid, -math.inf), dim=1)
    cum = cum + att
    ctx = (att[:, None, :] @ epq)[:, 0]
    return h, ctx, cum, att


def gen_steps_batch(ep, epq, lens, fc1_w, fc1_b, fc2_w, fc2_b, w_ih, b_ih, w_hh, b_hh, W, bW, cw, L, bL, v, rnn_in_w,
                    rnn_in_b, lstm1, lstm2, mel_w, r, S, stop_threshold=None):
    """ep, epq [B,Tx,D] (rows at t >= lens[b] are ignored), lens int64 [B]
    -> (attn [B,S',Tx], frames [B,S'*r,n_mels], smax [B,S'], s_out [B] int64); S' = max(s_out), every item is stepped
    for S' steps, stopped or not."""
    B, Tx, D = ep.shape
    Ld = lstm1[1].shape[1]
    n_mels = mel_w.shape[0] // K.MAX_R
    valid = _mask(lens, Tx)
    ep = ep.masked_fill(~valid[:, :, None], 0.0)
    epq = epq.masked_fill(~valid[:, :, None], 0.0)
    state = K.attend_state(ep)
    h1 = c1 = h2 = c2 = ep.new_zeros(B, Ld)
    f = ep.new_zeros(B, n_mels)
    s_out = torch.full((B,), S, dtype=torch.int64)
    attns, frames = [], []
    for s in range(S):
        p = torch.relu(f @ fc1_w.t() + fc1_b)
        p = torch.relu(p @ fc2_w.t() + fc2_b)
        Pr = p @ w_ih[:, D:D + p.shape[1]].t() + b_ih
        state = attend_step_masked(state, Pr, ep, epq, valid, w_ih, w_hh, b_hh, W, bW, cw, L, bL, v)
        xm = torch.cat([state[1], state[0]], 1) @ rnn_in_w.t() + rnn_in_b
        h1, c1 = K.lstm_cell(xm, h1, c1, *lstm1)
        xm = xm + h1
        h2, c2 = K.lstm_cell(xm, h2, c2, *lstm2)
        xm = xm + h2
        mel = (xm @ mel_w.t()).view(B, n_mels, K.MAX_R)[:, :, :r]
        f = mel[:, :, -1]
        attns.append(state[3])
        frames.append(mel.transpose(1, 2))
        if stop_threshold is not None and s * r > 10:
            below = (mel < stop_threshold).reshape(B, -1).all(1)
            s_out = torch.where(below & (s_out > s), torch.full_like(s_out, s + 1), s_out)
            if int(s_out.max()) <= s + 1:
                break
    frames = torch.cat(frames, 1)
    smax = frames.reshape(B, len(attns), -1).amax(2)
    Sm = int(s_out.max())
    return torch.stack(attns, 1)[:, :Sm], frames[:, :Sm * r], smax[:, :Sm], s_out


def generate_batch(P, x, x_len, cfg, r, steps, speaker_emb=None, stop_threshold=None):
    """-> dict(mel, linear [B,80,Tm], attn [B,Sm,Tx], mel_len, steps_out, smax [B,Sm]) as tensors of P's dtype, padded as
    Tacotron.generate_batch pads.  x [B,Tx]; x_len int64 [B]; speaker_emb [B, speaker_emb_dim] when that is > 0."""
    dt = P['encoder.embedding.weight'].dtype
    thr = torch.tensor(cfg['stop_threshold'] if stop_threshold is None else stop_threshold, dtype=torch.float32)
    B, Tx = x.shape
    S = math.ceil(int(steps) / r)
    valid = _mask(x_len, Tx)

    y = P['encoder.embedding.weight'][x]
    y = torch.relu(y @ P['encoder.pre_net.fc1.weight'].t() + P['encoder.pre_net.fc1.bias'])
    y = torch.relu(y @ P['encoder.pre_net.fc2.weight'].t() + P['encoder.pre_net.fc2.bias'])
    y = y * valid[:, :, None].to(dt)
    enc = cbhg_lens(y.transpose(1, 2), x_len, P, 'encoder.cbhg.', cfg['encoder_k'], cfg['num_highways'])
    if cfg.get('speaker_emb_dim', 0) > 0:
        semb = speaker_emb.to(dtype=dt)
        enc = torch.cat([enc, semb[:, None, :].expand(B, Tx, semb.shape[1])], 2)
    ep = enc @ P['encoder_proj.weight'].t()
    eq = enc @ P['encoder_proj_query.weight'].t()

    attn, frames, smax, s_out = gen_steps_batch(
        ep, eq, x_len, P['decoder.prenet.fc1.weight'], P['decoder.prenet.fc1.bias'], P['decoder.prenet.fc2.weight'],
        P['decoder.prenet.fc2.bias'], P['decoder.attn_rnn.weight_ih'], P['decoder.attn_rnn.bias_ih'],
        *R.attend_weights(P)[1:], P['decoder.rnn_input.weight'], P['decoder.rnn_input.bias'],
        R.lstm_weights(P, 'decoder.res_rnn1.'), R.lstm_weights(P, 'decoder.res_rnn2.'),
        P['decoder.mel_proj.weight'], r, S, stop_threshold=thr)
    Sm = attn.shape[1]
    mel_len = s_out * r
    fm = _mask(mel_len, Sm * r)
    mel_cl = frames * fm[:, :, None].to(dt)
    post = cbhg_lens(mel_cl.transpose(1, 2), mel_len, P, 'postnet.', cfg['postnet_k'], cfg['num_highways'])
    lin = post @ P['post_proj.weight'].t()
    pad = lambda t: t.masked_fill(~fm[:, :, None], PAD_VALUE).transpose(1, 2).contiguous()
    attn = attn * _mask(s_out, Sm)[:, :, None].to(dt)
    return dict(mel=pad(mel_cl), linear=pad(lin), attn=attn, mel_len=mel_len, steps_out=s_out, smax=smax)
