"""Per-token pitch / energy on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_align_features.py [--batch 32] [--iters 20] [--warmup 3] [--seed 0] [--batches 8]

token_values_ms: one TokenValues.extract_batch (one ft_token_values launch) on a seeded batch of B items with
Tx ~ U[120, 180] tokens and Tm ~ U[700, 900] frames (80 mel channels), HIP events, mean over --iters after --warmup;
bytes: the mel, raw pitch and durations read plus the two outputs written.  normalize_ms: normalize_pitch over the
token pitches of all B items (three launches and one host read of the statistics).
extract_durations_s / create_align_features_s: the two passes over the same --batches batches, host clock around each
whole call (files written to a temporary directory).  The teacher is a stub whose align() returns the batch's
precomputed attention, so the difference between the two is the added pitch / energy stage (raw-pitch reads, the
launch, the per-speaker normalisation and the extra files), not the teacher.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_align import make_batch, timed  # noqa: E402
from forwardtacotron_amd.durations import DurationExtractor, extract_durations  # noqa: E402
from forwardtacotron_amd.pitch_energy import TokenValues, create_align_features, normalize_pitch  # noqa: E402


class _Stub(torch.nn.Module):
    def __init__(self, attn):
        super().__init__()
        self.attn, self.r = attn, 1
        self.decoder = torch.nn.Module()
        self.decoder.prenet = torch.nn.Module()

    def align(self, batch):
        return self.attn[batch['item_id'][0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--batches', type=int, default=8)
    a = ap.parse_args()
    attn, x, x_len, mel, mel_len = make_batch(a.batch, a.seed)
    ext = DurationExtractor(silence_threshold=-11., silence_prob_shift=0.25)
    dur = ext.extract_batch(attn, x, x_len, mel, mel_len).durations
    rng = np.random.default_rng(a.seed)
    pitch = torch.from_numpy(rng.uniform(60., 400., (a.batch, mel.shape[2])).astype(np.float32)).cuda()
    pitch_len = mel_len.clone()
    x_len_d, mel_len_d, pitch_len_d = x_len.cuda(), mel_len.cuda(), pitch_len.cuda()
    res = TokenValues.extract_batch(mel, mel_len_d, pitch, pitch_len_d, dur, x_len_d, 30., 600.)
    assert not res.status.cpu().numpy().any()
    ms = timed(lambda: TokenValues.extract_batch(mel, mel_len_d, pitch, pitch_len_d, dur, x_len_d, 30., 600.,
                                                 check=False), a.iters, a.warmup)
    tok = torch.cat([res.pitch[b, :int(x_len[b])] for b in range(a.batch)])
    norm_ms = timed(lambda: normalize_pitch(tok.clone()), a.iters, a.warmup)
    bytes_ = 4 * mel.shape[1] * int(mel_len.sum()) + 4 * int(mel_len.sum()) + 8 * dur.numel() + 8 * dur.numel()

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'raw_pitch'))
        batches, stub = [], {}
        for k in range(a.batches):
            ids = [f'b{k}_{b}' for b in range(a.batch)]
            for b, i in enumerate(ids):
                np.save(os.path.join(tmp, 'raw_pitch', f'{i}.npy'), pitch[b, :int(mel_len[b])].cpu().numpy())
            stub[ids[0]] = attn
            batches.append({'x': x, 'mel': mel, 'x_len': x_len, 'mel_len': mel_len, 'item_id': ids,
                            'speaker_name': ['speaker'] * a.batch})
        model = _Stub(stub)
        extract_durations(model, batches[:1], os.path.join(tmp, 'warm'), extractor=ext)
        create_align_features(model, batches[:1], os.path.join(tmp, 'warm'), os.path.join(tmp, 'raw_pitch'),
                              os.path.join(tmp, 'warm_p'), os.path.join(tmp, 'warm_e'), 30., 600., extractor=ext)
        torch.cuda.synchronize()
        t = time.perf_counter()
        extract_durations(model, batches, os.path.join(tmp, 'alg1'), extractor=ext)
        dur_s = time.perf_counter() - t
        t = time.perf_counter()
        create_align_features(model, batches, os.path.join(tmp, 'alg2'), os.path.join(tmp, 'raw_pitch'),
                              os.path.join(tmp, 'pp'), os.path.join(tmp, 'pe'), 30., 600., extractor=ext)
        caf_s = time.perf_counter() - t

    print(json.dumps({
        'metric': 'align_features', 'batch': a.batch, 'mean_x_len': float(x_len.float().mean()),
        'mean_mel_len': float(mel_len.float().mean()), 'token_values_ms': round(ms, 4),
        'token_values_bytes': bytes_, 'token_values_gb_per_s': round(bytes_ / ms / 1e6, 2),
        'normalize_ms': round(norm_ms, 4), 'normalize_values': int(tok.numel()),
        'batches': a.batches, 'extract_durations_s': round(dur_s, 4), 'create_align_features_s': round(caf_s, 4),
    }))


if __name__ == '__main__':
    main()
