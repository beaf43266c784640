"""Float64 numpy restatement of the speaker-embedding definition ("Speaker embedding", steps 2-8):
increase-only volume, partial slices, zero extension, centred power mel, the three-layer LSTM, relu(linear), the two
normalisations and the speaker means.  It imports nothing of the package: the slice rule, the mel basis (mel_cpu's) and
the recurrence are written out here.  tests/test_voice_encoder_cpu.py holds it to torch.nn.LSTM and scipy.signal.stft;
tests/test_gpu_speaker.py compares the kernels with it.

The seeded fixture of both test files is fixture(): production widths, default nn.LSTM / nn.Linear initialisation, five
wavs of 1, 25600, 31519, 31520 and 50000 samples (1, 1, 1, 2 and 3 partials)."""
import functools
import math
from fractions import Fraction

import numpy as np

import mel_cpu as M

CFG = dict(sr=16000, n_fft=400, hop=160, n_mels=40, pf=160, target_dBFS=-30.0, hidden=256, embedding=256, layers=3)
LENGTHS = (1, 25600, 31519, 31520, 50000)
COUNTS = (1, 1, 1, 2, 3)
LOUD_ITEM = 1                       # scaled above -30 dBFS: its gain is 1
SPEAKERS = ('p225', 'p226', 'p225', 'p227', 'p226')          # counts 2, 2, 1


# ---------------------------------------------------------------------------------------------------
def partial_slices(n, rate=1.3, min_coverage=0.75, sr=16000, hop=160, pf=160):
    """resemblyzer's compute_partial_slices -> (wav slices, mel slices); the coverage test in exact rationals"""
    n_frames = int(math.ceil((n + 1) / hop))
    frame_step = int(round((sr / rate) / hop))
    steps = max(1, n_frames - pf + frame_step + 1)
    mel = [(i, i + pf) for i in range(0, steps, frame_step)]
    wav = [(a * hop, b * hop) for a, b in mel]
    start, stop = wav[-1]
    if Fraction(n - start, stop - start) < Fraction(min_coverage) and len(mel) > 1:
        mel, wav = mel[:-1], wav[:-1]
    return wav, mel


def gain(w, target_dBFS=-30.0):
    """10^(target / 20) / sqrt(mean(w^2)) if that is above 1, else 1; 1 for an all-zero wav"""
    ms = float(np.mean(np.asarray(w, dtype=np.float64) ** 2))
    if ms == 0.0:
        return 1.0
    g = 10.0 ** (target_dBFS / 20.0) / math.sqrt(ms)
    return g if g > 1.0 else 1.0


def dft(n_fft):
    """windowed DFT matrices (periodic Hann) float64: cos [F, n_fft], -sin [F, n_fft]"""
    k = np.arange(n_fft)
    ang = 2 * np.pi * np.outer(np.arange(1 + n_fft // 2), k) / n_fft
    win = M.hann(n_fft, n_fft)
    return np.cos(ang) * win, -np.sin(ang) * win


def extend(w, stop):
    """zero-extended to the end of the last kept wav slice if that lies past the wav, else whole"""
    w = np.asarray(w)
    return np.concatenate([w, np.zeros(stop - len(w), dtype=w.dtype)]) if stop > len(w) else w


def power_mel(w, cfg=CFG):
    """[1 + len(w) // hop, n_mels] float64: centred frames with zero padding, |X|^2, Slaney basis, no log"""
    c, s = dft(cfg['n_fft'])
    fr = M.frame(M.pad_signal(w, cfg['n_fft']), cfg['n_fft'], cfg['hop'])
    re, im = fr @ c.T, fr @ s.T
    return (re * re + im * im) @ M.mel_basis(cfg['sr'], cfg['n_fft'], cfg['n_mels'], 0, cfg['sr'] / 2).T


def power_mel_fp32(w, cfg=CFG):
    """the same through stock torch in float32 on the CPU (frames x DFT matrices, torch.matmul): the route whose error
    against float64 scales the device tolerance"""
    import torch
    c, s = (torch.from_numpy(a.astype(np.float32)) for a in dft(cfg['n_fft']))
    fr = torch.from_numpy(M.frame(np.pad(np.asarray(w, dtype=np.float32), cfg['n_fft'] // 2), cfg['n_fft'], cfg['hop']))
    re, im = fr @ c.T, fr @ s.T
    B = torch.from_numpy(M.mel_basis(cfg['sr'], cfg['n_fft'], cfg['n_mels'], 0, cfg['sr'] / 2).astype(np.float32))
    out = (re * re + im * im) @ B.T
    assert out.dtype == torch.float32
    return out.numpy()


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def lstm(x, state, layers, prefix='lstm.'):
    """nn.LSTM(batch_first=True) from zero states, float64: x [N, T, I] -> (out of the last layer [N, T, H], h_last [N, H])"""
    x = np.asarray(x, dtype=np.float64)
    for l in range(layers):
        w_ih, w_hh, b_ih, b_hh = (np.asarray(state[f'{prefix}{n}_l{l}'], dtype=np.float64)
                                  for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
        Hd = w_hh.shape[1]
        h = np.zeros((x.shape[0], Hd))
        c = np.zeros((x.shape[0], Hd))
        out = np.zeros((x.shape[0], x.shape[1], Hd))
        for t in range(x.shape[1]):
            g = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
            i, f, gg, o = (g[:, k * Hd:(k + 1) * Hd] for k in range(4))
            c = sigmoid(f) * c + sigmoid(i) * np.tanh(gg)
            h = sigmoid(o) * np.tanh(c)
            out[:, t] = h
        x = out
    return x, x[:, -1]


def embed_utterance(w, state, cfg=CFG, rate=1.3, min_coverage=0.75, normalize_volume=True):
    """every stage of one wav in float64: gain, mel (of the zero-extended scaled wav), wav / mel slices, partials
    [k, pf, n_mels], h_last, raw = relu(linear), raw_norm, partial_embeds, mean_norm (before the last division), embed"""
    w = np.asarray(w, dtype=np.float64)
    g = gain(w, cfg['target_dBFS']) if normalize_volume else 1.0
    wav_sl, mel_sl = partial_slices(len(w), rate, min_coverage, cfg['sr'], cfg['hop'], cfg['pf'])
    mel = power_mel(extend(w * g, wav_sl[-1][1]), cfg)
    parts = np.stack([mel[a:b] for a, b in mel_sl])
    _, h_last = lstm(parts, state, cfg['layers'])
    lw, lb = (np.asarray(state[k], dtype=np.float64) for k in ('linear.weight', 'linear.bias'))
    raw = np.maximum(h_last @ lw.T + lb, 0.0)
    raw_norm = np.linalg.norm(raw, axis=1)
    pe = raw / raw_norm[:, None]
    mean = pe.mean(axis=0)
    return dict(gain=g, mel=mel, wav_slices=wav_sl, mel_slices=mel_sl, partials=parts, h_last=h_last, raw=raw,
                raw_norm=raw_norm, partial_embeds=pe, mean_norm=float(np.linalg.norm(mean)),
                embed=mean / np.linalg.norm(mean))


def mean_speaker_embs(embed, speakers):
    """({name: row} in order of first appearance, [S, E] float64): sum / count / 2-norm per speaker"""
    embed = np.asarray(embed, dtype=np.float64)
    names = {}
    for s in speakers:
        names.setdefault(s, len(names))
    out = np.zeros((len(names), embed.shape[1]))
    for name, r in names.items():
        m = embed[[b for b, s in enumerate(speakers) if s == name]].sum(axis=0) / sum(s == name for s in speakers)
        out[r] = m / np.linalg.norm(m)
    return names, out


# ---------------------------------------------------------------------------------------------------
def make_wav(seed, n, level, sr=16000):
    """a few harmonics of a seeded fundamental plus noise, float32, scaled to an rms of `level`"""
    rng = np.random.default_rng([seed, n])
    t = np.arange(n) / sr
    f0 = 110.0 + 20.0 * seed
    y = sum(a * np.cos(2 * np.pi * f0 * (h + 1) * t + rng.uniform(0, 6.28)) for h, a in enumerate((1.0, 0.5, 0.3, 0.2)))
    y = y + 0.1 * rng.standard_normal(n)
    return (y * (level / np.sqrt(np.mean(y ** 2)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(seed=0):
    """-> dict(wavs: five float32 arrays, state: {key: float32 numpy array} in resemblyzer's layout).  Shared: read-only."""
    import torch
    torch.manual_seed(seed)
    lstm_m = torch.nn.LSTM(CFG['n_mels'], CFG['hidden'], CFG['layers'], batch_first=True)
    lin = torch.nn.Linear(CFG['hidden'], CFG['embedding'])
    state = {f'lstm.{k}': v.detach().numpy().copy() for k, v in lstm_m.state_dict().items()}
    state.update({f'linear.{k}': v.detach().numpy().copy() for k, v in lin.state_dict().items()})
    wavs = [make_wav(b, n, 0.2 if b == LOUD_ITEM else 0.004 * (b + 1)) for b, n in enumerate(LENGTHS)]
    for a in list(state.values()) + wavs:
        a.setflags(write=False)
    return dict(wavs=wavs, state=state)


@functools.lru_cache(maxsize=None)
def reference(seed=0):
    """the float64 stages of every wav of fixture(seed), computed once and shared: do not write to them"""
    fx = fixture(seed)
    return [embed_utterance(w, fx['state']) for w in fx['wavs']]
