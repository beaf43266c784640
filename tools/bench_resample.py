"""Sample-rate conversion in front of the audio front end, on an LJSpeech-shaped batch: prints one JSON line per source rate.

    python tools/bench_resample.py [--batch 32] [--iters 50] [--warmup 5] [--rounds 7] [--seed 0] [--no-scipy]

A seeded batch of B wavs of about 6.5 s (the items of tools/bench_mel.py, generated at the source rate; the lengths
vary by +-15 %), already on the device, given at 48000 Hz and at 44100 Hz to a DSP of 22050 Hz
(forwardtacotron_amd/audio.py).  Reported per source rate (HIP events, mean over --iters after --warmup):
  resample_batch_ms     the public call end to end, inputs on the device (the gather into the padded batch included)
  kernel_ms             ft_resample_poly_ragged alone on the gathered batch, and kernel_GBps = the bytes the algorithm
                        needs (every input sample read once, every output sample written once: 4 (sum len + sum
                        out_len)) over that time; kernel_pct_hbm_peak = that rate over the 8.0 TB/s HBM3E peak (spec).
                        The batch (about 40 MB in, 18 MB out) fits the 256 MiB Infinity Cache, which back-to-back
                        iterations re-hit: an achieved rate, not HBM traffic.  kernel_GMACs = multiply-adds per second
  preprocess_ms / preprocess_src_ms   DSP.preprocess_batch of the same audio given at 22050 Hz (the resampled wavs, as a
                        list of device tensors) and given at the source rate with source_sr, in --rounds alternating
                        rounds of --iters calls in this one process: median (min) over the rounds
  scipy_ms              for scale: scipy.signal.resample_poly over the same wavs, one after the other on the CPU of this
                        host (float32 in, one pass, one thread of numpy), where scipy is present
  max_abs_diff_scipy    device result against scipy's float64 result on the first wav
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd.audio import DSP, resample_ratio  # noqa: E402
import mel_cpu as R  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def make_batch(B, seed, sr, seconds=6.5):
    rng = np.random.default_rng(seed)
    wavs = []
    for b in range(B):
        n = int(sr * seconds * rng.uniform(0.85, 1.15))
        lead, tail = int(rng.integers(2000, 12000)) * sr // 22050, int(rng.integers(2000, 12000)) * sr // 22050
        wavs.append(R.make_item(seed * 1000 + b, lead, n - lead - tail, tail, sr))
    return wavs


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-scipy', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample: needs an MI355X (no CPU fallback)')
    dsp = DSP.from_config({'dsp': R.CFG})
    for src in (48000, 44100):
        host = make_batch(a.batch, a.seed, src)
        wavs = [torch.from_numpy(y).cuda() for y in host]
        up, down = resample_ratio(src, dsp.sample_rate)
        res = {'source_sr': src, 'up': up, 'down': down, 'batch': len(wavs)}
        res['resample_batch_ms'] = timed(lambda: dsp.resample_batch(wavs, src), a.iters, a.warmup)

        wav, lens, Lmax = dsp._rs_input(wavs, None)[:3]
        tab, half = dsp._rs_table(up, down)
        ldy = (-((-Lmax * up) // down) + 3) // 4 * 4
        res['kernel_ms'] = timed(lambda: H.resample_poly_ragged(wav, lens, Lmax, tab, up, down, half, ldy), a.iters, a.warmup)
        out = dsp.resample_batch(wavs, src)
        n_in, n_out = int(lens.sum()), int(out['wav_len'].sum())
        res['seconds_of_audio'] = round(n_out / dsp.sample_rate, 1)
        res['kernel_GBps'] = 4.0 * (n_in + n_out) / res['kernel_ms'] / 1e6
        res['kernel_pct_hbm_peak'] = 100.0 * res['kernel_GBps'] / HBM_PEAK_GBPS
        res['kernel_GMACs'] = n_out * ((2 * half + 1) / up) / res['kernel_ms'] / 1e6

        out_len = out['wav_len'].cpu().tolist()
        at_target = [out['wav'][b, :out_len[b]].clone() for b in range(len(wavs))]
        plain, with_src = [], []
        for _ in range(a.rounds):
            plain.append(timed(lambda: dsp.preprocess_batch(at_target), a.iters, a.warmup))
            with_src.append(timed(lambda: dsp.preprocess_batch(wavs, source_sr=src), a.iters, a.warmup))
        res['preprocess_ms'], res['preprocess_ms_min'] = statistics.median(plain), min(plain)
        res['preprocess_src_ms'], res['preprocess_src_ms_min'] = statistics.median(with_src), min(with_src)

        if not a.no_scipy:
            try:
                from scipy.signal import resample_poly
            except ImportError:
                resample_poly = None
            if resample_poly is not None:
                resample_poly(host[0], up, down)
                t0 = time.perf_counter()
                for y in host:
                    resample_poly(y, up, down)
                res['scipy_ms'] = 1e3 * (time.perf_counter() - t0)
                res['scipy_over_resample_batch'] = res['scipy_ms'] / res['resample_batch_ms']
                ref = resample_poly(host[0].astype(np.float64), up, down)
                res['max_abs_diff_scipy'] = float(np.abs(at_target[0].cpu().numpy() - ref).max())
        print(json.dumps({k: (float(f'{v:.4g}') if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == '__main__':
    main()
