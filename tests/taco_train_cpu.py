"""Restatement of the Tacotron teacher's TRAINING forward (Tacotron.forward_train), written from the math with stock
torch ops and differentiable by torch autograd: tests/taco_cpu.py with batch-statistics BatchNorm (and the updated
running statistics), the four CBHG dropout sites and the two zoneout sites.  float64 on the host it is the gradient
oracle of tests/test_gpu_tacotron_train.py; tests/test_tacotron_train_cpu.py ties it to the reference model.

masks: multipliers (0 or 1/(1-p)) in the storage order of the package's sites --
  'enc1' [B,Tx,256], 'enc2' [B,Tx,128]                     encoder.pre_net fc1, fc2
  'enc_bank' [B,Tx,K*128], 'enc_proj1' [B,Tx,128]          encoder.cbhg behind the pooled bank / behind conv_project1
  'dec1' [S,B,256], 'dec2' [S,B,128]                       decoder.prenet (time-major)
  'zone1', 'zone2' [S,B,L]                                 1 where the step is ZONED (h keeps its previous value), else 0
  'post_bank' [B,T,K*dims], 'post_proj1' [B,T,256]         postnet
a missing key leaves its site off.
"""
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

import taco_cpu as C
import taco_step_cpu as K

BN_EPS = 1e-5
BN_MOMENTUM = 0.1
MAX_R = K.MAX_R

SITE_MASKS = {'encoder.pre_net.fc1': 'enc1', 'encoder.pre_net.fc2': 'enc2', 'encoder.cbhg.bank': 'enc_bank',
              'encoder.cbhg.conv_project1': 'enc_proj1', 'decoder.prenet.fc1': 'dec1', 'decoder.prenet.fc2': 'dec2',
              'decoder.res_rnn1': 'zone1', 'decoder.res_rnn2': 'zone2', 'postnet.bank': 'post_bank',
              'postnet.conv_project1': 'post_proj1'}


def _bn_train(y, P, pre, stats):
    """BatchNorm1d in training mode on y [B,C,T]: batch statistics (biased variance) normalise; the running statistics
    move by momentum 0.1 towards the batch mean and the UNBIASED batch variance"""
    n = y.shape[0] * y.shape[2]
    mean = y.mean(dim=(0, 2))
    var = y.var(dim=(0, 2), unbiased=False)
    with torch.no_grad():
        stats[pre + 'running_mean'] = (1 - BN_MOMENTUM) * P[pre + 'running_mean'] + BN_MOMENTUM * mean
        stats[pre + 'running_var'] = (1 - BN_MOMENTUM) * P[pre + 'running_var'] + BN_MOMENTUM * var * (n / max(n - 1, 1))
    scale = P[pre + 'weight'] / torch.sqrt(var + BN_EPS)
    return (y - mean[None, :, None]) * scale[None, :, None] + P[pre + 'bias'][None, :, None]


def _bnconv(x, P, pre, relu, stats):
    # an even kernel gives T + 1 positions: the reference normalises all of them (batch statistics over T + 1) and
    # truncates afterwards (common_layers.py:54-57, 106)
    w = P[pre + 'conv.weight']
    y = F.conv1d(x, w, padding=w.shape[2] // 2)
    if relu:
        y = torch.relu(y)
    return _bn_train(y, P, pre + 'bnorm.', stats)[:, :, :x.shape[2]]


def _mask(y, m):
    """y [B,C,T] times a channels-last mask [B,T,C] (None: site off)"""
    return y if m is None else y * m.to(y.device, y.dtype).transpose(1, 2)


def cbhg(x, P, pre, Kb, num_highways, stats, m_bank=None, m_proj1=None):
    """x [B,C,T] -> [B,T,2*channels], training mode"""
    bank = torch.cat([_bnconv(x, P, f'{pre}conv1d_bank.{k}.', True, stats) for k in range(Kb)], 1)
    prev = torch.cat([torch.full_like(bank[:, :, :1], -math.inf), bank[:, :, :-1]], 2)
    y = _mask(torch.maximum(bank, prev), m_bank)
    y = _mask(_bnconv(y, P, pre + 'conv_project1.', True, stats), m_proj1)
    y = _bnconv(y, P, pre + 'conv_project2.', False, stats) + x
    y = y.transpose(1, 2) @ P[pre + 'pre_highway.weight'].t()
    for i in range(num_highways):
        hp = f'{pre}highways.{i}.'
        a = torch.relu(y @ P[hp + 'W1.weight'].t() + P[hp + 'W1.bias'])
        g = torch.sigmoid(y @ P[hp + 'W2.weight'].t() + P[hp + 'W2.bias'])
        y = g * a + (1 - g) * y
    rp = pre + 'rnn.'
    f = C._gru_seq(y, P[rp + 'weight_ih_l0'], P[rp + 'weight_hh_l0'], P[rp + 'bias_ih_l0'], P[rp + 'bias_hh_l0'], False)
    b = C._gru_seq(y, P[rp + 'weight_ih_l0_reverse'], P[rp + 'weight_hh_l0_reverse'], P[rp + 'bias_ih_l0_reverse'],
                   P[rp + 'bias_hh_l0_reverse'], True)
    return torch.cat([f, b], 2)


def forward(P: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor], cfg: dict, r: int,
            masks: Optional[Dict[str, torch.Tensor]] = None):
    """-> (mel_outputs [B,80,S*r], linear [B,80,S*r], attn [B,S,Tx], stats): stats holds the updated running_mean /
    running_var of every BatchNorm by state_dict name.  cfg: encoder_k, postnet_k, num_highways, speaker_emb_dim."""
    masks = masks or {}
    dt = P['encoder.embedding.weight'].dtype
    dev = P['encoder.embedding.weight'].device
    mk = lambda name: masks[name].to(dev, dt) if name in masks else None
    x = batch['x'].to(dev)
    mel = batch['mel'].to(device=dev, dtype=dt)
    B, Tx = x.shape
    steps = mel.shape[2]
    S = math.ceil(steps / r)
    stats = {}

    y = P['encoder.embedding.weight'][x]
    y = torch.relu(y @ P['encoder.pre_net.fc1.weight'].t() + P['encoder.pre_net.fc1.bias'])
    if 'enc1' in masks:
        y = y * mk('enc1')
    y = torch.relu(y @ P['encoder.pre_net.fc2.weight'].t() + P['encoder.pre_net.fc2.bias'])
    if 'enc2' in masks:
        y = y * mk('enc2')
    enc = cbhg(y.transpose(1, 2), P, 'encoder.cbhg.', cfg['encoder_k'], cfg['num_highways'], stats, mk('enc_bank'),
               mk('enc_proj1'))
    if cfg.get('speaker_emb_dim', 0) > 0:
        semb = batch['speaker_emb'].to(device=dev, dtype=dt)
        enc = torch.cat([enc, semb[:, None, :].expand(B, Tx, semb.shape[1])], 2)
    ep = enc @ P['encoder_proj.weight'].t()
    eq = enc @ P['encoder_proj_query.weight'].t()

    D = P['decoder.attn_rnn.weight_hh'].shape[1]
    w_ih, b_ih = P['decoder.attn_rnn.weight_ih'], P['decoder.attn_rnn.bias_ih']
    n_mels = mel.shape[1]
    Pg = []
    for i in range(S):
        f = mel[:, :, i * r - 1] if i > 0 else mel.new_zeros(B, n_mels)
        p = torch.relu(f @ P['decoder.prenet.fc1.weight'].t() + P['decoder.prenet.fc1.bias'])
        if 'dec1' in masks:
            p = p * mk('dec1')[i]
        p = torch.relu(p @ P['decoder.prenet.fc2.weight'].t() + P['decoder.prenet.fc2.bias'])
        if 'dec2' in masks:
            p = p * mk('dec2')[i]
        Pg.append(p @ w_ih[:, D:].t() + b_ih)
    attn, hist = K.attend(ep, eq, torch.stack(Pg, 0), *C.attend_weights(P))
    l1, l2 = C.lstm_weights(P, 'decoder.res_rnn1.'), C.lstm_weights(P, 'decoder.res_rnn2.')
    Ld = l1[1].shape[1]
    z1 = mk('zone1') if 'zone1' in masks else mel.new_zeros(S, B, Ld)
    z2 = mk('zone2') if 'zone2' in masks else mel.new_zeros(S, B, Ld)
    h1 = c1 = h2 = c2 = mel.new_zeros(B, Ld)
    frames = []
    for i in range(S):
        xm = hist[i] @ P['decoder.rnn_input.weight'].t() + P['decoder.rnn_input.bias']
        hn, c1 = K.lstm_cell(xm, h1, c1, *l1)
        h1 = h1 * z1[i] + hn * (1 - z1[i])
        xm = xm + h1
        hn, c2 = K.lstm_cell(xm, h2, c2, *l2)
        h2 = h2 * z2[i] + hn * (1 - z2[i])
        xm = xm + h2
        frames.append((xm @ P['decoder.mel_proj.weight'].t()).view(B, n_mels, MAX_R)[:, :, :r])
    mel_out = torch.cat(frames, 2)
    post = cbhg(mel_out, P, 'postnet.', cfg['postnet_k'], cfg['num_highways'], stats, mk('post_bank'), mk('post_proj1'))
    linear = (post @ P['post_proj.weight'].t()).transpose(1, 2)
    return mel_out, linear, attn, stats


def site_shapes(cfg: dict, B: int, Tx: int, S: int, r: int, lstm_dims: int, postnet_dims: int) -> Dict[str, tuple]:
    """shape of every site's tensor in the package's storage order, by site name"""
    T = S * r
    return {'encoder.pre_net.fc1': (B, Tx, 256), 'encoder.pre_net.fc2': (B, Tx, 128),
            'encoder.cbhg.bank': (B, Tx, cfg['encoder_k'] * 128), 'encoder.cbhg.conv_project1': (B, Tx, 128),
            'decoder.prenet.fc1': (S, B, 256), 'decoder.prenet.fc2': (S, B, 128),
            'decoder.res_rnn1': (S, B, lstm_dims), 'decoder.res_rnn2': (S, B, lstm_dims),
            'postnet.bank': (B, T, cfg['postnet_k'] * postnet_dims), 'postnet.conv_project1': (B, T, 256)}


def masks_from_seeds(seeds: Dict[str, Optional[int]], probs: Dict[str, float], shapes: Dict[str, tuple]):
    """the masks argument of forward() from a model's last_seeds: dropout sites keep * 1/(1-p), zoneout sites 1 where
    ft_dropout's mask is 0; sites whose seed is None are left out"""
    import numpy as np
    import dropout_cpu
    out = {}
    for site, key in SITE_MASKS.items():
        seed = seeds.get(site)
        if seed is None:
            continue
        m = dropout_cpu.site_mask(seed, shapes[site], probs[site])
        if key.startswith('zone'):
            m = (m == 0).astype(np.float64)
        out[key] = torch.from_numpy(m)
    return out
