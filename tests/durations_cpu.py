"""CPU restatement of duration extraction (forwardtacotron_amd/durations.py), written from the math: the shifted and
clamped attention, a float64 min-plus DP over the monotonic paths (right, down, diagonal; an edge weighs the cost of
the cell it enters; ties: diagonal, then down, then right), each frame to the last token its row visits, and the
statistics of duration_extraction_pipe.py.  Test-side only."""
import numpy as np
import torch


def frame_silent(mel: np.ndarray, threshold: float) -> np.ndarray:
    """mel [n_mels, Tm] -> bool [Tm]: channel mean (torch's own reduction) below the threshold"""
    return (torch.from_numpy(np.ascontiguousarray(mel, dtype=np.float32)).mean(dim=0) < threshold).numpy()


def shifted_attention(att: np.ndarray, mel: np.ndarray, x: np.ndarray, threshold: float, shift: float,
                      sil_ids) -> np.ndarray:
    """fp32 attention after the silence shift (only if at least two frames are silent) and the clamp"""
    a = np.array(att, dtype=np.float32, copy=True)
    sil = frame_silent(mel, threshold)
    if sil.sum() >= 2:
        tok = np.isin(x, np.asarray(sil_ids))
        sh = np.where(tok, np.float32(shift), -np.float32(shift)).astype(np.float32)
        a[sil] = a[sil] + sh[None, :]
    return np.clip(a, np.float32(0.), np.float32(1.))


def min_path(cost: np.ndarray):
    """cost [Tm, Tx] float64 -> (distance of the last cell, back-pointer codes [Tm, Tx]: 0 diag, 1 down, 2 right);
    swept by anti-diagonals, every cell min(predecessors) + its cost, the start's own cost not counted"""
    Tm, Tx = cost.shape
    d = np.full((Tm, Tx), np.inf)
    code = np.full((Tm, Tx), 3, dtype=np.int8)
    d[0, 0] = 0.
    for s in range(1, Tm + Tx - 1):
        j = np.arange(max(0, s - Tm + 1), min(s, Tx - 1) + 1)
        i = s - j
        diag = np.where((i > 0) & (j > 0), d[np.maximum(i - 1, 0), np.maximum(j - 1, 0)], np.inf)
        down = np.where(i > 0, d[np.maximum(i - 1, 0), j], np.inf)
        right = np.where(j > 0, d[i, np.maximum(j - 1, 0)], np.inf)
        best, c = diag, np.zeros(len(j), dtype=np.int8)
        c = np.where(down < best, 1, c)
        best = np.minimum(best, down)
        c = np.where(right < best, 2, c).astype(np.int8)
        best = np.minimum(best, right)
        d[i, j] = best + cost[i, j]
        code[i, j] = c
    return d[-1, -1], code


def backtrack(code: np.ndarray):
    """the path's cells from (0,0) to (Tm-1, Tx-1)"""
    i, j = code.shape[0] - 1, code.shape[1] - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        c = code[i, j]
        if i == 0:
            c = 2
        elif j == 0:
            c = 1
        if c == 0:
            i, j = i - 1, j - 1
        elif c == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    return path[::-1]


def path_cost(path, cost: np.ndarray) -> float:
    """the distance of a path, summed in path order from the start (the start's own cost not counted)"""
    s = 0.
    for (i, j) in path[1:]:
        s = s + float(cost[i, j])
    return s


def is_monotone(path, Tm: int, Tx: int) -> bool:
    if path[0] != (0, 0) or path[-1] != (Tm - 1, Tx - 1):
        return False
    return all((i1 - i0, j1 - j0) in ((0, 1), (1, 0), (1, 1)) for (i0, j0), (i1, j1) in zip(path, path[1:]))


def durations_from_path(path, Tx: int) -> np.ndarray:
    last = {}
    for i, j in path:
        last[i] = j
    dur = np.zeros(Tx, dtype=np.int64)
    for j in last.values():
        dur[j] += 1
    return dur


def align_score(att: np.ndarray) -> float:
    """loc part of utils/metrics.py:attention_score at r = 1 for one cropped item (fp32 like the reference)"""
    Tm = att.shape[0]
    am = np.argmax(att, axis=1)
    n = int(np.sum(np.abs(np.diff(am)) <= 1))
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float32(n) / np.float32(Tm - 1))


def max_consecutive_ones(dur: np.ndarray) -> int:
    best = run = 0
    for v in dur:
        run = run + 1 if v == 1 else 0
        best = max(best, run)
    return best


def extract(x, mel, att, threshold, shift, sil_ids):
    """one item: x [Tx], mel [n_mels, Tm], att [Tm, Tx] -> dict(dur, cost, att_score, align_score, path, ...)"""
    a = shifted_attention(att, mel, x, threshold, shift, sil_ids)
    cost = (np.float32(1.) - a).astype(np.float64)
    dist, code = min_path(cost)
    path = backtrack(code)
    dur = durations_from_path(path, att.shape[1])
    sil = frame_silent(mel, threshold)
    vals = [float(a[i, j]) for i, j in path if not sil[i]]
    return dict(dur=dur, cost=dist, path=path, cost_matrix=cost,
                att_score=sum(vals) / len(vals) if vals else float('nan'), align_score=align_score(att),
                max_duration=int(dur.max()), max_consecutive_ones=max_consecutive_ones(dur))
