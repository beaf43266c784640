"""Raw pitch (pYIN) behind the audio front end, on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_pitch.py [--batch 32] [--iters 20] [--warmup 3] [--seed 0] [--no-cpu]

The seeded batch of tools/bench_resample.py at 22050 Hz (B wavs of about 6.5 s, lengths +-15 %; 32 wavs are about 210 s
of audio), already on the device, through pitch.LibrosaPitchExtractor of the shipped config (30-600 Hz, frame 2048, hop
256).  Reported (HIP events, mean over --iters after --warmup):
  extract_batch_ms    the public call end to end, inputs on the device (the gather into the padded batch included)
  cmnd_ms             ft_pyin_cmnd alone on the gathered batch; cmnd_Gpairs = the subtract + fma pairs the definition needs
                      (frames * (pmax + 1) * W) and cmnd_TFLOPs = 3 flops per pair over that time -- the achieved fp32
                      rate; cmnd_pct_fp32_peak = that over the 157.3 TFLOP/s vector fp32 peak (spec).  The kernel also
                      computes the lags of its last block of four and the padding frames' zeros; they are not counted
  observe_ms          ft_pyin_observe alone
  viterbi_ms          ft_pyin_viterbi alone, and viterbi_us_per_step = that over the frames of the LONGEST item: every
                      item is one workgroup on its own CU, the launch lasts as long as the longest recursion plus its
                      backtracking
  pyin64_ms_per_wav   for scale only: the float64 TEST RESTATEMENT (tests/pyin_cpu.py pyin64, numpy, one thread) on the
                      first wav.  It is not librosa.pyin and says nothing about librosa's speed
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd.pitch import LibrosaPitchExtractor  # noqa: E402
from bench_resample import make_batch, timed  # noqa: E402

FP32_PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-cpu', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pitch: needs an MI355X (no CPU fallback)')
    ext = LibrosaPitchExtractor(fmin=30, fmax=600, sample_rate=22050, frame_length=2048, hop_length=256)
    tb = ext.tables
    host = make_batch(a.batch, a.seed, 22050)
    wavs = [torch.from_numpy(y).cuda() for y in host]
    res = {'batch': len(wavs), 'seconds_of_audio': round(sum(len(y) for y in host) / 22050, 1)}
    res['extract_batch_ms'] = timed(lambda: ext.extract_batch(wavs), a.iters, a.warmup)

    wav, lens, Lmax = ext._gather(wavs)
    Tmax = 1 + Lmax // tb['hop_length']
    st = ext.stages(wav, lens, Lmax)
    frames = st['frames'].cpu().numpy()
    res['frames'], res['frames_longest'] = int(frames.sum()), int(frames.max())
    res['cmnd_ms'] = timed(lambda: H.pyin_cmnd(wav, lens, Lmax, tb['frame_length'], tb['hop_length'], tb['pmin'],
                                               tb['pmax'], Tmax), a.iters, a.warmup)
    pairs = float(frames.sum()) * (tb['pmax'] + 1) * tb['W']
    res['cmnd_Gpairs'] = pairs / 1e9
    res['cmnd_TFLOPs'] = 3.0 * pairs / res['cmnd_ms'] / 1e9
    res['cmnd_pct_fp32_peak'] = 100.0 * res['cmnd_TFLOPs'] / FP32_PEAK_TFLOPS
    res['observe_ms'] = timed(lambda: H.pyin_observe(st['dn'], st['frames'], tb, ext._dev), a.iters, a.warmup)
    res['viterbi_ms'] = timed(lambda: H.pyin_viterbi(st['lo_v'], st['lo_u'], st['frames'], tb, ext._dev), a.iters,
                              a.warmup)
    res['viterbi_us_per_step'] = 1e3 * res['viterbi_ms'] / res['frames_longest']
    res['voiced_frames'] = int((st['pitch'] > 0).sum())
    if not a.no_cpu:
        import pyin_cpu as R
        t0 = time.perf_counter()
        ref = R.pyin64(host[0], tb)
        res['pyin64_ms_per_wav'] = 1e3 * (time.perf_counter() - t0)
        got = st['pitch'][0, :int(frames[0])].cpu().numpy()
        res['frames_equal_pyin64_wav0'] = f'{int((got == ref["pitch"].astype(np.float32)).sum())}/{len(got)}'
    print(json.dumps({k: (float(f'{v:.4g}') if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


if __name__ == '__main__':
    main()
