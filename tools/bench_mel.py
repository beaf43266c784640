"""The audio front end on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_mel.py [--batch 32] [--iters 20] [--warmup 3] [--seed 0] [--no-torch]

A seeded batch of B wavs of about 6.5 s at 22050 Hz (quiet noise, a body of two cosines plus noise, quiet noise; the
lengths vary by +-15 %) already on the device runs through DSP.preprocess_batch (forwardtacotron_amd/audio.py): two
ft_wav_trim_peak launches, ft_wav_pack, the DFT GEMM, ft_mel_project.  Reported (HIP events, mean over --iters after
--warmup):
  preprocess_batch_ms   the public call end to end, inputs on the device (the gather into the padded batch included)
  trim_peak_ms / pack_ms / dft_gemm_ms / mel_project_ms   each stage alone, and for the three HBM-bound kernels the
                        bytes the algorithm needs (computed from the shapes: trim_peak reads every sample once and
                        writes two floats per 512 of them; pack reads the trimmed samples and writes the packed buffer
                        and the wav output; mel_project reads the valid rows of the spectrum and writes the mel) over
                        that time as *_GBps; the GEMM's rate as dft_gemm_TFLOPs (2 * rows * n_fft * 2Fp).  The byte
                        counts are algorithmic lower bounds (the block statistics that the second trim launch reads
                        back, sized from the longest item, and pack's reads of the per-item scalars are left out), and
                        the batch (about 18 MB of samples, 86 MB of spectrum) fits the 256 MiB Infinity Cache, which
                        back-to-back iterations re-hit: the rates are achieved bandwidth, not HBM traffic
  torch_ms              the stock-torch restatement of the tests (tests/mel_cpu.torch_preprocess: torch.stft + matmul,
                        fp32, one wav after the other with the host reads its trimming needs) on the same GPU
  max_abs_log_mel_diff  the two routes compared on this batch
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd.audio import DSP, MEL_PAD_VALUE  # noqa: E402
import mel_cpu as R  # noqa: E402


def make_batch(B, seed, sr=22050, seconds=6.5):
    rng = np.random.default_rng(seed)
    wavs = []
    for b in range(B):
        n = int(sr * seconds * rng.uniform(0.85, 1.15))
        lead, tail = int(rng.integers(2000, 12000)), int(rng.integers(2000, 12000))
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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--no-torch', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mel: needs an MI355X (no CPU fallback)')
    dsp = DSP.from_config({'dsp': R.CFG})
    wavs = [torch.from_numpy(y).cuda() for y in make_batch(a.batch, a.seed)]
    B = len(wavs)
    hop, n_fft, Fp, n_mels = dsp.hop_length, dsp.n_fft, dsp.Fp, dsp.n_mels

    res = {'batch': B, 'seconds_of_audio': round(sum(w.numel() for w in wavs) / R.CFG['sample_rate'], 1)}
    res['preprocess_batch_ms'] = timed(lambda: dsp.preprocess_batch(wavs), a.iters, a.warmup)

    # the stages alone, on the buffers of one call
    wav, lens, Lmax = dsp._wavs(wavs)
    ld = wav.shape[1]
    Tmax, Tcap = 1 + Lmax // hop, (ld + n_fft + hop - 1) // hop
    rows = B * Tcap
    tp = H.wav_trim_peak(wav, lens, Lmax, True, dsp.trim_silence_top_db, 0, hop)
    packed, _ = H.wav_pack(wav, tp, Tcap * hop, n_fft, False)

    def gemm():
        return H.linear_fwd_as(packed, hop, dsp.gl.w_fwd, rows, n_fft)

    spec = gemm()
    res['trim_peak_ms'] = timed(lambda: H.wav_trim_peak(wav, lens, Lmax, True, dsp.trim_silence_top_db, 0, hop),
                                a.iters, a.warmup)
    res['pack_ms'] = timed(lambda: H.wav_pack(wav, tp, Tcap * hop, n_fft, False), a.iters, a.warmup)
    res['dft_gemm_ms'] = timed(gemm, a.iters, a.warmup)
    res['mel_project_ms'] = timed(lambda: H.mel_project(spec, Fp, Tcap, tp['mel_len'], dsp.mel_w, dsp.mel_meta, n_mels,
                                                        B, Tmax, True, MEL_PAD_VALUE), a.iters, a.warmup)
    n_in = int(lens.sum())
    n_trim, n_frames = int(tp['wav_len'].sum()), int(tp['mel_len'].sum())
    bytes_trim = 4 * n_in + 8 * (n_in // 512)
    bytes_pack = 4 * n_trim + 4 * packed.numel() + 4 * B * ld
    bytes_mel = 4 * n_frames * 2 * Fp + 4 * B * n_mels * Tmax
    res['trim_peak_GBps'] = bytes_trim / res['trim_peak_ms'] / 1e6
    res['pack_GBps'] = bytes_pack / res['pack_ms'] / 1e6
    res['mel_project_GBps'] = bytes_mel / res['mel_project_ms'] / 1e6
    res['dft_gemm_TFLOPs'] = 2.0 * rows * n_fft * 2 * Fp / res['dft_gemm_ms'] / 1e9
    res['frames'] = n_frames
    res['gemm_rows'] = rows

    if not a.no_torch:
        basis = torch.from_numpy(R.mel_basis(R.CFG['sample_rate'], n_fft, n_mels, R.CFG['fmin'], R.CFG['fmax'])).float().cuda()
        res['torch_ms'] = timed(lambda: [R.torch_preprocess(w, R.CFG, basis) for w in wavs], a.iters, a.warmup)
        out = dsp.preprocess_batch(wavs)
        worst = 0.0
        for b, w in enumerate(wavs):
            s, e, _, mel = R.torch_preprocess(w, R.CFG, basis)
            assert (s, e) == (int(out['trim_start'][b]), int(out['trim_end'][b])), (b, s, e)
            worst = max(worst, float((out['mel'][b, :, :mel.shape[1]] - mel).abs().max()))
        res['max_abs_log_mel_diff'] = worst
        res['speedup_vs_torch'] = res['torch_ms'] / res['preprocess_batch_ms']
    print(json.dumps({k: (float(f'{v:.4g}') if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
