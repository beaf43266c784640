"""Speaker embeddings (speaker.VoiceEncoder.embed_batch) on an LJSpeech-shaped batch: prints one JSON line.

    python tools/bench_speaker_emb.py [--batch 32] [--iters 100] [--warmup 5] [--rounds 5] [--seed 0]

The seeded batch of tools/bench_resample.py at 22050 Hz (B wavs of about 6.5 s, lengths +-15 %), already on the device,
through VoiceEncoder() with its default (seeded) initialisation and source_sr=22050.  Reported (HIP events, mean over
--iters after --warmup; the two end-to-end figures and the stock-torch route are taken in --rounds alternating rounds and
given as the median with [min, max]):
  embed_batch_ms        the public call end to end with host lengths (gather, resampling, every launch)
  embed_batch_16k_ms    the same on the batch already at 16 kHz (no resampling launch)
  partials              the partial count P of the batch (rows of the recurrences); chunks of speaker.PARTIAL_CHUNK
  stage times           each stage alone on the intermediates of one call: new_kernels_ms (ft_spk_gain, ft_spk_pack,
                        ft_spk_mel_power, ft_spk_gather_partials, ft_spk_segment_mean_norm, listed one by one too),
                        gemm_ms (the DFT GEMM, the three input projections, the embedding GEMM), recurrence_ms (the three
                        ft_lstm_fwd_uni), and their shares of the sum
  us_per_step           recurrence_ms over the 3 * 160 dependent steps of one chunk (times the number of chunks)
  torch_lstm_ms         for comparison: stock float32 torch.nn.LSTM + Linear + relu + the two normalisations on the same
                        GPU, fed the same gathered partials [P, 160, 40]; torch_max_abs_diff = its embeddings against ours
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from forwardtacotron_amd import hip as H  # noqa: E402
from forwardtacotron_amd import speaker as S  # noqa: E402
from forwardtacotron_amd.audio import resample_len  # noqa: E402
from bench_resample import make_batch, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_speaker_emb: needs an MI355X (no CPU fallback)')
    torch.manual_seed(a.seed)
    enc = S.VoiceEncoder().to('cuda')
    host = make_batch(a.batch, a.seed, 22050)
    wavs = [torch.from_numpy(y).cuda() for y in host]
    res = {'batch': len(wavs), 'seconds_of_audio': round(sum(len(y) for y in host) / 22050, 1)}

    st = enc.stages(wavs, source_sr=22050)
    lens16 = [resample_len(len(y), 22050, 16000) for y in host]
    wav16, len16 = st['wav'], torch.tensor(lens16)
    P = int(st['table'].shape[0])
    chunk = max(1, int(S.PARTIAL_CHUNK))
    res['partials'], res['chunks'] = P, -(-P // chunk)
    assert int(st['n_partials'].sum()) == P

    B, rows = st['mel'].shape[:2]
    pf, hop, n_fft, Hd = enc.partials_n_frames, enc.hop, enc.n_fft, enc.hidden
    w_fwd, mel_w, mel_meta = enc._tables(wav16.device)
    Fp = w_fwd.shape[0] // 2
    step, cov = S.frame_step_of(enc.sampling_rate, hop, 1.3), S.coverage_fraction(0.75)
    L = max(lens16)
    lens_d, gain, frames = st['wav_len'], st['gain'], st['frames']
    t = lambda fn: timed(fn, a.iters, a.warmup)
    k = {}
    k['spk_gain_ms'] = t(lambda: H.spk_gain(wav16, lens_d, L, 10.0 ** -1.5, hop, pf, step, cov[0], cov[1], True))
    k['spk_pack_ms'] = t(lambda: H.spk_pack(wav16, lens_d, L, gain, rows * hop, n_fft))
    packed = H.spk_pack(wav16, lens_d, L, gain, rows * hop, n_fft)
    g = {'dft_gemm_ms': t(lambda: H.linear_fwd_as(packed, hop, w_fwd, B * rows, n_fft))}
    spec = H.linear_fwd_as(packed, hop, w_fwd, B * rows, n_fft)
    k['spk_mel_power_ms'] = t(lambda: H.spk_mel_power(spec, Fp, rows, frames, mel_w, mel_meta, enc.n_mels, B))
    mel = st['mel'].view(B * rows, enc.n_mels)
    k['spk_gather_ms'] = g['proj_gemm_ms'] = g['embed_gemm_ms'] = 0.0
    rec = 0.0
    for p0 in range(0, P, chunk):
        Pc = min(chunk, P - p0)
        k['spk_gather_ms'] += t(lambda: H.spk_gather_partials(mel, rows, frames, st['table'], p0, Pc, pf, B))
        x = H.spk_gather_partials(mel, rows, frames, st['table'], p0, Pc, pf, B)
        for layer in range(enc.num_layers):
            w_ih, w_hh, b_ih, b_hh = (getattr(enc.lstm, f'{n}_l{layer}') for n in
                                      ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'))
            g['proj_gemm_ms'] += t(lambda: H.linear_fwd(x, w_ih, b_ih))
            xp = H.linear_fwd(x, w_ih, b_ih)
            rec += t(lambda: H.lstm_fwd_uni(xp, w_hh, b_hh, Hd))
            x, _ = H.lstm_fwd_uni(xp, w_hh, b_hh, Hd)
        g['embed_gemm_ms'] += t(lambda: H.linear_fwd(x[pf - 1], enc.linear.weight, enc.linear.bias, relu=True))
    k['spk_segment_ms'] = t(lambda: H.spk_segment_mean_norm(st['raw'], None, st['offsets'], st['n_partials'], True))
    H.check_rnn_status()
    res.update(k)
    res.update(g)
    res['new_kernels_ms'], res['gemm_ms'], res['recurrence_ms'] = sum(k.values()), sum(g.values()), rec
    total = res['new_kernels_ms'] + res['gemm_ms'] + rec
    for name in ('new_kernels', 'gemm', 'recurrence'):
        res[f'{name}_share_pct'] = 100.0 * res[f'{name}_ms'] / total
    res['us_per_step'] = 1e3 * rec / (res['chunks'] * enc.num_layers * pf)
    res['rnn_launches_persistent_perstep'] = list(H.rnn_counters())

    # stock torch on the same GPU, float32, fed the same partials
    parts = torch.cat(st['partials'], dim=1).transpose(0, 1).contiguous()           # [P, pf, n_mels]

    def stock():
        with torch.no_grad():
            _, (h, _) = enc.lstm(parts)
            e = torch.relu(enc.linear(h[-1]))
            e = e / e.norm(dim=1, keepdim=True)
            out = torch.stack([e[lo:hi].mean(dim=0) for lo, hi in zip(offs[:-1], offs[1:])])
            return out / out.norm(dim=1, keepdim=True)
    offs = st['offsets'].cpu().tolist()
    arms = {'embed_batch_ms': lambda: enc.embed_batch(wavs, source_sr=22050),
            'embed_batch_16k_ms': lambda: enc.embed_batch(wav16, wav_len=len16), 'torch_lstm_ms': stock}
    runs = {name: [] for name in arms}
    for _ in range(max(1, a.rounds)):                   # alternating: a drift of the box shows up in every arm alike
        for name, fn in arms.items():
            runs[name].append(timed(fn, a.iters, a.warmup))
    for name, v in runs.items():
        res[name] = float(np.median(v))
        res[name + '_min_max'] = [float(f'{min(v):.4g}'), float(f'{max(v):.4g}')]
    res['ours_without_mel_ms'] = k['spk_gather_ms'] + g['proj_gemm_ms'] + g['embed_gemm_ms'] + rec + k['spk_segment_ms']
    res['torch_max_abs_diff'] = float((stock() - st['embed']).abs().max())
    print(json.dumps({k_: (float(f'{v:.4g}') if isinstance(v, float) else v) for k_, v in res.items()}), flush=True)


if __name__ == '__main__':
    main()
