"""CPU: the float64 restatement of the speaker-embedding definition (tests/voice_encoder_cpu.py) against independent
routes -- torch.nn.LSTM in float64, scipy.signal.stft -- the slice rule's table in its three forms (the restatement, the
package's host function, the C function the kernels apply on the device), the volume rule, the module's state-dict layout
and checkpoint loading, and the condition on the seeded fixture that the GPU test relies on."""
import numpy as np
import pytest
import torch

import voice_encoder_cpu as R

# n, slices, last wav stop
TABLE = [(1, 1, 25600), (25600, 1, 25600), (31519, 1, 25600), (31520, 2, 37920), (37920, 2, 37920), (40000, 2, 37920),
         (50000, 3, 50240), (104000, 7, 99520)]


@pytest.mark.parametrize('n,count,stop', TABLE)
def test_slice_table(n, count, stop):
    from forwardtacotron_amd import hip as H, speaker as S
    wav, mel = R.partial_slices(n)
    assert (len(wav), wav[-1][1]) == (count, stop)
    assert all(b - a == 160 and (wa, wb) == (a * 160, b * 160) for (a, b), (wa, wb) in zip(mel, wav))
    assert [a for a, _ in mel] == [77 * i for i in range(count)]
    pw, pm = S.compute_partial_slices(n)
    assert [(s.start, s.stop) for s in pw] == wav and [(s.start, s.stop) for s in pm] == mel
    assert S.partial_count(n, 160, 160, 77, (3, 4)) == count
    assert H.spk_slices(n, 160, 160, 77, 3, 4) == (count, mel[-1][1])


def test_coverage_boundary_is_exact():
    """31520 samples cover exactly 0.75 of the second slice (kept: the test is `<`); one sample fewer drops it"""
    assert (31520 - 77 * 160) * 4 == 3 * 25600
    assert len(R.partial_slices(31520)[0]) == 2 and len(R.partial_slices(31519)[0]) == 1
    # a min_coverage that is no small fraction is compared as the nearest one with a denominator below 2^20
    from forwardtacotron_amd import speaker as S
    assert S.coverage_fraction(0.75) == (3, 4) and S.coverage_fraction(1.0) == (1, 1) and S.coverage_fraction(0.0) == (0, 1)
    num, den = S.coverage_fraction(0.7)
    assert den <= 1 << 20 and abs(num / den - 0.7) < 1e-12


def test_three_forms_of_the_slice_rule_agree():
    """the restatement, the package's host function and the kernels' function, production and shrunk configuration,
    every length around every boundary"""
    from forwardtacotron_amd import hip as H, speaker as S
    for sr, hop, pf, top in ((16000, 160, 160, 120000), (1600, 16, 16, 2000)):
        step = S.frame_step_of(sr, hop, 1.3)
        assert step == int(round((sr / 1.3) / hop))
        ns = range(1, top) if top <= 2000 else sorted(set(
            [1, 2, top] + [k * hop * step + pf * hop * 3 // 4 + d for k in range(0, 9) for d in range(-hop - 2, hop + 3)]
            + [k * hop + d for k in range(150, 330) for d in (-1, 0, 1)]))
        for n in ns:
            if n < 1:
                continue
            wav, mel = R.partial_slices(n, 1.3, 0.75, sr, hop, pf)
            assert S.partial_count(n, hop, pf, step, (3, 4)) == len(mel), n
            assert H.spk_slices(n, hop, pf, step, 3, 4) == (len(mel), mel[-1][1]), n


def test_shrunk_configuration():
    """sr = 1600, hop = 16, partials of 16 frames: frame_step = round(1600 / 1.3 / 16) = 77"""
    wav, mel = R.partial_slices(1, sr=1600, hop=16, pf=16)
    assert (wav, mel) == ([(0, 256)], [(0, 16)])
    wav, mel = R.partial_slices(3000, sr=1600, hop=16, pf=16)          # 188 frames, steps 250: i = 0, 77, 154, 231
    assert [a for a, _ in mel] == [0, 77, 154] and wav[-1] == (154 * 16, 170 * 16)   # the fourth covers 0 of its span
    from forwardtacotron_amd.speaker import VoiceEncoder
    enc = VoiceEncoder(sampling_rate=1600, partials_n_frames=16, model_hidden_size=16, model_embedding_size=8,
                       model_num_layers=2, mel_n_channels=8)
    assert (enc.n_fft, enc.hop) == (40, 16)
    assert enc.dft_matrix().shape == (2 * 24, 40) and enc.mel_basis().shape == (8, 21)


def test_lstm_restatement_against_torch_float64():
    torch.manual_seed(3)
    m = torch.nn.LSTM(40, 256, 3, batch_first=True).double()
    x = torch.randn(3, 12, 40, dtype=torch.float64)
    with torch.no_grad():
        out, (h, _) = m(x)
    state = {f'lstm.{k}': v.numpy() for k, v in m.state_dict().items()}
    got, h_last = R.lstm(x.numpy(), state, 3)
    assert np.abs(got - out.numpy()).max() < 1e-12 and np.abs(h_last - h[-1].numpy()).max() < 1e-12


def test_power_mel_against_scipy_stft():
    signal = pytest.importorskip('scipy.signal')
    w = R.fixture()['wavs'][1][:8000].astype(np.float64)
    _, _, Z = signal.stft(w, window=signal.get_window('hann', 400, fftbins=True), nperseg=400, noverlap=240, nfft=400,
                          boundary='zeros', padded=False, return_onesided=True, scaling='spectrum')
    Z = Z * signal.get_window('hann', 400, fftbins=True).sum()          # undo scipy's spectrum scaling
    want = (np.abs(Z) ** 2).T @ R.M.mel_basis(16000, 400, 40, 0, 8000).T
    got = R.power_mel(w)
    assert got.shape == (1 + 8000 // 160, 40)
    n = min(len(got), len(want))
    assert n >= 50 and np.abs(got[:n] - want[:n]).max() <= 1e-10 * np.abs(want).max()


def test_volume_rule():
    rng = np.random.default_rng(0)
    w = rng.standard_normal(4000)
    quiet, loud = w * (0.001 / np.sqrt(np.mean(w ** 2))), w * (0.5 / np.sqrt(np.mean(w ** 2)))
    assert abs(R.gain(quiet) - 10 ** -1.5 / 0.001) < 1e-9                       # raised to -30 dBFS
    assert abs(np.sqrt(np.mean((quiet * R.gain(quiet)) ** 2)) - 10 ** -1.5) < 1e-12
    assert R.gain(loud) == 1.0                                                  # increase only
    assert R.gain(np.zeros(100)) == 1.0                                         # deliberate: no division by zero
    fx = R.fixture()
    gains = [R.gain(w) for w in fx['wavs']]
    assert gains[R.LOUD_ITEM] == 1.0 and all(g > 1.0 for b, g in enumerate(gains) if b != R.LOUD_ITEM)


def test_state_dict_layout_and_checkpoint_round_trip(tmp_path):
    from forwardtacotron_amd._lib import FtError
    from forwardtacotron_amd.speaker import VoiceEncoder
    enc = VoiceEncoder()
    keys = [f'lstm.{n}_l{l}' for l in range(3) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')]
    assert list(enc.state_dict()) == keys + ['linear.weight', 'linear.bias']
    assert enc.lstm.weight_ih_l0.shape == (1024, 40) and enc.linear.weight.shape == (256, 256)
    fx = R.fixture()
    state = {k: torch.from_numpy(v.copy()) for k, v in fx['state'].items()}
    assert set(state) == set(enc.state_dict())
    full = dict(state, similarity_weight=torch.tensor([10.0]), similarity_bias=torch.tensor([-5.0]))
    path = tmp_path / 'pretrained.pt'
    torch.save({'model_state': full}, path)
    got = VoiceEncoder.from_checkpoint(path)
    assert all(torch.equal(got.state_dict()[k], state[k]) for k in state)
    torch.save(state, tmp_path / 'bare.pt')                                     # a bare state dict
    bare = VoiceEncoder.from_checkpoint(tmp_path / 'bare.pt')
    assert all(torch.equal(bare.state_dict()[k], state[k]) for k in state)
    del full['linear.bias']
    torch.save({'model_state': full}, tmp_path / 'short.pt')
    with pytest.raises(FtError, match='linear.bias'):
        VoiceEncoder.from_checkpoint(tmp_path / 'short.pt')
    with pytest.raises(FtError):                                                # CPU parameters: no fallback
        got.embed_utterance(np.zeros(100, np.float32))
    with pytest.raises(FtError):
        got.embed_batch([np.zeros(100, np.float32)], trim_long_silences=True)


def test_fixture_condition_norms_are_far_from_zero():
    """every partial's |relu(linear(h_last))| and every utterance's mean norm is at least 1e-2, so that the divisions of
    the definition can neither hide nor inflate an error of the kernels; the partial counts are the documented ones"""
    ref = R.reference()
    assert tuple(len(r['mel_slices']) for r in ref) == R.COUNTS
    assert tuple(len(w) for w in R.fixture()['wavs']) == R.LENGTHS
    for b, r in enumerate(ref):
        print(b, 'raw norms', r['raw_norm'], 'mean norm', r['mean_norm'])
        assert r['raw_norm'].min() >= 1e-2 and r['mean_norm'] >= 1e-2
        assert abs(np.linalg.norm(r['embed']) - 1.0) < 1e-12
    names, means = R.mean_speaker_embs(np.stack([r['embed'] for r in ref]), R.SPEAKERS)
    assert names == {'p225': 0, 'p226': 1, 'p227': 2} and np.abs(np.linalg.norm(means, axis=1) - 1).max() < 1e-12
