"""CPU restatement of the per-token pitch / energy targets (forwardtacotron_amd/pitch_energy.py), written from the
contract of train_tacotron.py:24-93 in float64: frame energies ||exp(mel[:, t])||_2, per-token means over the duration
segments (pitch: zeros and values outside [fmin, fmax] dropped), the zip(range(mel_len), ...) cut-off, and the
per-speaker normalisation over the nonzero token pitches.  Test-side only."""
import numpy as np


def frame_energy(mel: np.ndarray) -> np.ndarray:
    """mel [n_mels, T] (log) -> float64 [T]"""
    e = np.exp(np.asarray(mel, dtype=np.float64))
    return np.sqrt((e * e).sum(axis=0))


def token_values(mel, mel_len, pitch, dur, fmin, fmax):
    """one item -> (pitch [x_len], energy [x_len]) float64, or None if the durations do not sum to mel_len"""
    dur = np.asarray(dur, dtype=np.int64)
    if int(dur.sum()) != int(mel_len):
        return None
    energy = frame_energy(mel)
    pitch = np.asarray(pitch, dtype=np.float64)
    cum = np.concatenate([[0], np.cumsum(dur)])
    p_tok = np.zeros(len(dur))
    e_tok = np.zeros(len(dur))
    lo, hi = float(np.float32(fmin)), float(np.float32(fmax))       # numpy compares the fp32 pitch in fp32
    for j in range(min(int(mel_len), len(dur))):
        a, b = cum[j], cum[j + 1]
        v = pitch[a:b]
        v = v[(v != 0.) & (v >= lo) & (v <= hi)]
        p_tok[j] = v.mean() if len(v) else 0.
        e = energy[a:b]
        e_tok[j] = e.mean() if len(e) else 0.
    return p_tok, e_tok


def speaker_stats(pitches):
    """list of per-item token pitches -> (mean, std) float64 over the nonzero values (population std);
    std = 1e10 unless std > 0, mean NaN if no value is nonzero"""
    nz = np.concatenate([np.asarray(v, np.float64)[np.asarray(v) != 0] for v in pitches])
    if len(nz) == 0:
        return float('nan'), 1e10
    mean = nz.mean()
    std = np.sqrt(((nz - mean) ** 2).mean())
    return mean, (std if std > 0 else 1e10)


def normalize(v, mean, std):
    """(v - mean) / std where v != 0, 0 elsewhere"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v != 0, (v - mean) / std, 0.)
