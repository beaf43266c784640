"""Restatement of Tacotron.generate (forwardtacotron_amd/tacotron.py, models/tacotron.py:283-349) from the math with
stock torch ops, for the tests (float64 on the host) and as the fp32 stock-ops baseline of
tools/bench_taco_generate.py (on the device, with the reference's per-step stop test and its host sync).  It reads a
state_dict by name and runs on whatever device / dtype that state_dict's tensors have.  The per-step math is
tests/taco_step_cpu.py's gen_steps; the encoder and the postnet are tests/taco_cpu.py's.

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

import taco_cpu as R
import taco_step_cpu as K


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

    _, _, attn, frames, _ = K.gen_steps(
        ep, eq, P['decoder.prenet.fc1.weight'], P['decoder.prenet.fc1.bias'], P['decoder.prenet.fc2.weight'],
        P['decoder.prenet.fc2.bias'], P['decoder.attn_rnn.weight_ih'], P['decoder.attn_rnn.bias_ih'],
        *R.attend_weights(P)[1:], P['decoder.rnn_input.weight'], P['decoder.rnn_input.bias'],
        R.lstm_weights(P, 'decoder.res_rnn1.'), R.lstm_weights(P, 'decoder.res_rnn2.'),
        P['decoder.mel_proj.weight'], r, S, stop_threshold=thr)
    mel_out = frames.t()[None].contiguous()
    post = R.cbhg(mel_out, P, 'postnet.', cfg['postnet_k'], cfg['num_highways'])
    linear = (post @ P['post_proj.weight'].t()).transpose(1, 2)
    return mel_out[0], linear[0], attn, attn.shape[0]
