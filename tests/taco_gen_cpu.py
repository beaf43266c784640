"""Restatement of Tacotron.generate (forwardtacotron_amd/tacotron.py, models/tacotron.py:283-349) from the math with
stock torch ops, for the tests (float64 on the host) and as the fp32 stock-ops baseline of
tools/bench_taco_generate.py (on the device, with the reference's per-step stop test and its host sync).  It reads a
state_dict by name and runs on whatever device / dtype that state_dict's tensors have.  The encoder, the cell
equations and the postnet are tests/taco_cpu.py's.

  step s    (at most S = ceil(steps / r) steps; input frame: the last frame of step s-1, zeros at s = 0)
            p = relu(relu(f W1^T + b1) W2^T + b2)                                  (eval: no dropout)
            h = GRUCell([ctx, p], h); LSA; ctx = att @ eq                           (as taco_cpu.forward)
            x = Wi [ctx, h] + bi; x += LSTMCell1(x); x += LSTMCell2(x)             (eval: no zoneout)
            frames s*r + k, k < r: channel n = (Wm x)[n * 20 + k]
            stop after step s when all 80 r values are < stop_threshold and s*r > 10
  after     postnet CBHG over the generated frames -> post_proj
"""
import math

import torch
import torch.nn.functional as F

import taco_cpu as R


def generate(P, x, cfg, r, steps, speaker_emb=None, stop_threshold=None):
    """-> (mel_outputs [80, S_out*r], linear [80, S_out*r], attn [S_out, Tx], S_out) as tensors of P's dtype.
    cfg: encoder_k, postnet_k, num_highways, speaker_emb_dim, stop_threshold (stop_threshold overrides it).
    x [1, Tx]; speaker_emb [1, speaker_emb_dim] when speaker_emb_dim > 0."""
    dt = P['encoder.embedding.weight'].dtype
    dev = P['encoder.embedding.weight'].device
    thr = torch.tensor(cfg['stop_threshold'] if stop_threshold is None else stop_threshold, dtype=torch.float32,
                       device=dev)
    x = x.to(dev)
    Tx = x.shape[1]
    S = math.ceil(int(steps) / r)

    y = P['encoder.embedding.weight'][x]
    y = torch.relu(y @ P['encoder.pre_net.fc1.weight'].t() + P['encoder.pre_net.fc1.bias'])
    y = torch.relu(y @ P['encoder.pre_net.fc2.weight'].t() + P['encoder.pre_net.fc2.bias'])
    enc = R.cbhg(y.transpose(1, 2), P, 'encoder.cbhg.', cfg['encoder_k'], cfg['num_highways'])
    if cfg.get('speaker_emb_dim', 0) > 0:
        semb = speaker_emb.to(device=dev, dtype=dt)
        enc = torch.cat([enc, semb[:, None, :].expand(1, Tx, semb.shape[1])], 2)
    ep = enc @ P['encoder_proj.weight'].t()
    eq = enc @ P['encoder_proj_query.weight'].t()

    D = P['decoder.attn_rnn.weight_hh'].shape[1]
    w_ih, b_ih = P['decoder.attn_rnn.weight_ih'], P['decoder.attn_rnn.bias_ih']
    w_hh, b_hh = P['decoder.attn_rnn.weight_hh'], P['decoder.attn_rnn.bias_hh']
    Wc = P['decoder.attn_net.conv.weight']
    Lw, Lb = P['decoder.attn_net.L.weight'], P['decoder.attn_net.L.bias']
    Ww, Wb = P['decoder.attn_net.W.weight'], P['decoder.attn_net.W.bias']
    v = P['decoder.attn_net.v.weight'][0]
    Wm = P['decoder.mel_proj.weight']
    Ld = P['decoder.res_rnn1.weight_hh'].shape[1]
    n_mels = Wm.shape[0] // R.MAX_R

    zeros = dict(device=dev, dtype=dt)
    h, ctx = torch.zeros(1, D, **zeros), torch.zeros(1, D, **zeros)
    cum, att = torch.zeros(1, Tx, **zeros), torch.zeros(1, Tx, **zeros)
    h1 = c1 = h2 = c2 = torch.zeros(1, Ld, **zeros)
    f = torch.zeros(1, n_mels, **zeros)
    attns, frames = [], []
    for s in range(S):
        p = torch.relu(f @ P['decoder.prenet.fc1.weight'].t() + P['decoder.prenet.fc1.bias'])
        p = torch.relu(p @ P['decoder.prenet.fc2.weight'].t() + P['decoder.prenet.fc2.bias'])
        h = R._gru_cell(torch.cat([ctx, p], 1) @ w_ih.t() + b_ih, h, w_hh, b_hh)
        loc = F.conv1d(torch.stack([cum, att], 1), Wc, padding=Wc.shape[2] // 2).transpose(1, 2)
        e = torch.tanh((h @ Ww.t() + Wb)[:, None, :] + ep + loc @ Lw.t() + Lb) @ v
        att = torch.softmax(e, dim=1)
        cum = cum + att
        ctx = (att[:, None, :] @ eq)[:, 0]
        xm = torch.cat([ctx, h], 1) @ P['decoder.rnn_input.weight'].t() + P['decoder.rnn_input.bias']
        h1, c1 = R._lstm_cell(xm, h1, c1, P, 'decoder.res_rnn1.')
        xm = xm + h1
        h2, c2 = R._lstm_cell(xm, h2, c2, P, 'decoder.res_rnn2.')
        xm = xm + h2
        mel = (xm @ Wm.t()).view(1, n_mels, R.MAX_R)[:, :, :r]
        frames.append(mel)
        attns.append(att)
        f = mel[:, :, -1]
        if bool((mel < thr).all()) and s * r > 10:          # host sync per step, as the reference
            break
    mel_out = torch.cat(frames, 2)
    post = R.cbhg(mel_out, P, 'postnet.', cfg['postnet_k'], cfg['num_highways'])
    linear = (post @ P['post_proj.weight'].t()).transpose(1, 2)
    return mel_out[0], linear[0], torch.cat(attns, 0), len(frames)
