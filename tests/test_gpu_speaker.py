"""GPU: speaker.VoiceEncoder (csrc/ft_speaker.hip, the DFT and projection GEMMs, ft_lstm_fwd_uni at H = 256) against the
float64 restatement tests/voice_encoder_cpu.py, on its seeded fixture: production widths, default initialisation, five
wavs of 1, 25600, 31519, 31520 and 50000 samples = 1, 1, 1, 2, 3 partials (P = 8); item 1 is louder than -30 dBFS.

Bounds, all a priori (every figure is printed before it is asserted):
  gain       relative, the fp32 bound of an n-term sum of squares gamma_n = n u / (1 - n u), u = 2^-24, halved by the square
             root, plus 4 u for the division, the root and the final rounding;
  power mel  max error / the item's largest value <= 2.01 x the same figure of an fp32 stock-torch route (frames x DFT
             matrices, torch.matmul on the CPU) against float64;
  embeddings every component of partial_embeds and embed within 1e-4 (unit vectors: absolute), the figure the recurrences
             and the full-size parity are held to; batch against single and device against host lengths 2e-4 (triangle);
  means      the device's own fp32 embeddings through float64: a <= 3-term sum (2 u per term), the division by the
             count (u), the root of an E-term sum of squares ((E + 2) u / 2), the last division (u), on components of at
             most 1: (E / 2 + 16) u."""
import numpy as np
import pytest
import torch

import voice_encoder_cpu as R
from poison import poison as _poison

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MEL_FACTOR = 2.01
EMB_TOL = 1e-4


@pytest.fixture(scope='module')
def fx():
    return R.fixture()


@pytest.fixture(scope='module')
def enc(fx):
    from forwardtacotron_amd.speaker import VoiceEncoder
    m = VoiceEncoder()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in fx['state'].items()})
    return m.to('cuda')


@pytest.fixture(scope='module')
def clean(enc, fx):
    """the stages of the clean batch with host lengths, computed once (read-only)"""
    st = enc.stages(fx['wavs'])
    torch.cuda.synchronize()
    return st


def _np(t):
    return t.detach().cpu().numpy()


def _padded(wavs, fill=0.0, extra=0):
    L = max(len(w) for w in wavs) + extra
    pad = np.full((len(wavs), L), fill, dtype=np.float32)
    for b, w in enumerate(wavs):
        pad[b, :len(w)] = w
    return pad


def test_gain_and_slice_table(clean, fx):
    ref = R.reference()
    gain, n_partials, frames = _np(clean['gain']), _np(clean['n_partials']), _np(clean['frames'])
    assert n_partials.dtype == np.int64 and tuple(n_partials) == R.COUNTS == tuple(clean['host_counts'])
    assert gain[R.LOUD_ITEM] == 1.0
    for b, (w, r) in enumerate(zip(fx['wavs'], ref)):
        n = len(w)
        bound = 0.5 * n * U / (1 - n * U) + 4 * U
        err = abs(float(gain[b]) - r['gain']) / r['gain']
        print(f'item {b}: n {n} gain {gain[b]:.6g} relative error {err:.3e} bound {bound:.3e}')
        assert err <= bound
        assert int(frames[b]) == r['mel_slices'][-1][1]
    table = _np(clean['table'])
    want = [(b, a) for b, r in enumerate(ref) for a, _ in r['mel_slices']]
    assert table.dtype == np.int32 and [tuple(row) for row in table] == want
    assert list(_np(clean['offsets'])) == [0, 1, 2, 3, 5, 8]
    assert list(_np(clean['partial_item'])) == [0, 1, 2, 3, 3, 4, 4, 4]


def test_power_mel_against_float64(clean, fx):
    ref = R.reference()
    mel, frames = _np(clean['mel']), _np(clean['frames'])
    figures = []
    for b, (w, r) in enumerate(zip(fx['wavs'], ref)):
        fr = int(frames[b])
        want = r['mel'][:fr]
        z = R.extend(w.astype(np.float64) * r['gain'], r['wav_slices'][-1][1])
        scale = np.abs(want).max()
        e_ref = np.abs(R.power_mel_fp32(z)[:fr] - want).max() / scale
        e_dev = np.abs(mel[b, :fr].astype(np.float64) - want).max() / scale
        print(f'item {b}: power-mel error {e_dev:.3e} of the maximum, fp32 stock-torch route {e_ref:.3e}, ratio '
              f'{e_dev / e_ref:.2f}')
        assert np.isfinite(mel[b]).all() and not mel[b, fr:].any(), 'rows past the frame count must be zero'
        figures.append((b, e_dev, e_ref))
    for b, e_dev, e_ref in figures:
        assert e_dev <= MEL_FACTOR * e_ref, (b, e_dev, e_ref)


def test_gathered_partials_are_the_mel_rows(clean):
    """exact: slot p of the time-major input is rows first .. first + 159 of its item's mel"""
    mel, table = _np(clean['mel']), _np(clean['table'])
    assert len(clean['partials']) == 1
    x = _np(clean['partials'][0])
    assert x.shape == (160, 8, 40)
    for p, (item, first) in enumerate(table):
        assert x[:, p].tobytes() == mel[item, first:first + 160].tobytes(), p


def test_embeddings_against_float64(clean):
    ref = R.reference()
    want_h = np.concatenate([r['h_last'] for r in ref])
    want_p = np.concatenate([r['partial_embeds'] for r in ref])
    want_e = np.stack([r['embed'] for r in ref])
    e_h = np.abs(_np(clean['h_last']).astype(np.float64) - want_h).max()
    e_p = np.abs(_np(clean['partial_embeds']).astype(np.float64) - want_p).max()
    e_e = np.abs(_np(clean['embed']).astype(np.float64) - want_e).max()
    print(f'h_last error {e_h:.3e}, partial_embeds {e_p:.3e}, embed {e_e:.3e} (bound {EMB_TOL:.0e})')
    assert clean['embed'].shape == (5, 256) and clean['partial_embeds'].shape == (8, 256)
    assert clean['embed'].dtype == torch.float32 and clean['embed'].is_cuda
    assert e_h <= EMB_TOL and e_p <= EMB_TOL and e_e <= EMB_TOL


def test_batch_and_single(enc, clean, fx):
    batch = _np(clean['embed'])
    for b, w in enumerate(fx['wavs']):
        one = enc.embed_batch([w], return_partials=True)
        assert tuple(_np(one['n_partials'])) == (R.COUNTS[b],) and one['partial_embeds'].shape == (R.COUNTS[b], 256)
        err = np.abs(_np(one['embed'])[0].astype(np.float64) - batch[b]).max()
        print(f'item {b}: alone against inside the batch {err:.3e}')
        assert err <= 2 * EMB_TOL
        u = enc.embed_utterance(w)
        assert isinstance(u, np.ndarray) and u.dtype == np.float32 and u.tobytes() == _np(one['embed'])[0].tobytes()
    wd = torch.from_numpy(fx['wavs'][3].copy()).cuda()
    e, pe, slices = enc.embed_utterance(wd, return_partials=True)
    assert e.is_cuda and pe.shape == (2, 256) and [(s.start, s.stop) for s in slices] == [(0, 25600), (12320, 37920)]
    assert torch.equal(e, enc.embed_batch([wd])['embed'][0])


def test_nan_beyond_the_lengths_and_in_an_item_changes_no_other_bit(enc, fx, monkeypatch):
    from forwardtacotron_amd import speaker
    lens = torch.tensor([len(w) for w in fx['wavs']])
    base = enc.embed_batch(torch.from_numpy(_padded(fx['wavs'], 0.0, extra=37)).cuda(), wav_len=lens)
    monkeypatch.setattr(speaker, '_empty', _poison)             # every buffer of the module starts as NaN / junk
    pad = _padded(fx['wavs'], np.nan, extra=37)
    pad[2] = np.nan
    got = enc.embed_batch(torch.from_numpy(pad).cuda(), wav_len=lens)
    assert torch.equal(got['n_partials'], base['n_partials'])
    a, b = _np(got['embed']), _np(base['embed'])
    assert np.isfinite(b).all() and np.isnan(a[2]).all()
    for i in (0, 1, 3, 4):
        assert a[i].tobytes() == b[i].tobytes(), i


def test_device_side_lengths(enc, clean, fx):
    lens = [len(w) for w in fx['wavs']]
    pad = torch.from_numpy(_padded(fx['wavs'])).cuda()
    got = enc.embed_batch(pad, wav_len=torch.tensor(lens).cuda(), return_partials=True)
    assert tuple(_np(got['n_partials'])) == R.COUNTS
    assert got['partial_embeds'].shape == (5 * 3, 256)          # the slot count of L = 50000 for every item
    err = np.abs(_np(got['embed']).astype(np.float64) - _np(clean['embed'])).max()
    print(f'device-side against host-side lengths {err:.3e}')
    assert err <= 2 * EMB_TOL
    pe, item = _np(got['partial_embeds']), _np(got['partial_item'])
    assert list(item) == [b for b in range(5) for _ in range(3)]
    used = np.array([s < R.COUNTS[b] for b in range(5) for s in range(3)])
    assert not pe[~used].any() and np.abs(np.linalg.norm(pe[used], axis=1) - 1).max() < 1e-5
    from forwardtacotron_amd._lib import FtError
    for bad in ([1, 25600, 31519, 31520, 50001], [0, 25600, 31519, 31520, 50000], [1, -5, 31519, 31520, 50000]):
        with pytest.raises(FtError, match='wav_len'):
            enc.embed_batch(pad, wav_len=torch.tensor(bad).cuda())
    again = enc.embed_batch(pad, wav_len=torch.tensor(lens).cuda())          # and the object still works
    assert torch.equal(again['embed'], got['embed'])


def test_source_rate(enc, clean, fx):
    from forwardtacotron_amd.audio import DSP, resample_len
    dsp = DSP(num_mels=80, sample_rate=16000, hop_length=200, win_length=800, n_fft=800, fmin=0, fmax=8000)
    wavs = fx['wavs'][1:4]
    up = dsp.resample_batch(wavs, 16000, 22050)
    up_len = [resample_len(len(w), 16000, 22050) for w in wavs]
    wavs22 = [up['wav'][b, :n].clone() for b, n in enumerate(up_len)]
    a = enc.embed_batch(wavs22, source_sr=22050)
    rs = dsp.resample_batch(wavs22, 22050)
    b = enc.embed_batch(rs['wav'], wav_len=torch.tensor([resample_len(n, 22050, 16000) for n in up_len]))
    assert torch.equal(a['n_partials'], b['n_partials']) and torch.equal(a['embed'], b['embed'])
    assert torch.isfinite(a['embed']).all()
    same = enc.embed_batch(fx['wavs'], source_sr=16000)
    assert torch.equal(same['embed'], clean['embed'])


def test_chunking(enc, clean, fx, monkeypatch):
    from forwardtacotron_amd import speaker
    monkeypatch.setattr(speaker, 'PARTIAL_CHUNK', 3)
    st = enc.stages(fx['wavs'])
    assert [x.shape[1] for x in st['partials']] == [3, 3, 2]
    err = np.abs(_np(st['embed']).astype(np.float64) - _np(clean['embed'])).max()
    print(f'chunks of 3, 3, 2 against one chunk {err:.3e}')
    assert err <= 2 * EMB_TOL and torch.equal(st['n_partials'], clean['n_partials'])


def test_speaker_means_and_writers(enc, clean, tmp_path):
    from forwardtacotron_amd.speaker import write_mean_speaker_embs, write_speaker_embs
    embed = clean['embed']
    names, means = enc.mean_speaker_embs(embed, R.SPEAKERS)
    want_names, want = R.mean_speaker_embs(_np(embed), R.SPEAKERS)
    assert names == want_names == {'p225': 0, 'p226': 1, 'p227': 2} and means.shape == (3, 256) and means.is_cuda
    bound = (256 / 2 + 16) * U
    err = np.abs(_np(means).astype(np.float64) - want).max()
    print(f'speaker means error {err:.3e} bound {bound:.3e}')
    assert err <= bound
    ids = [f'utt_{b}' for b in range(5)]
    paths = write_speaker_embs({'embed': embed, 'n_partials': clean['n_partials']}, ids, tmp_path / 'speaker_emb')
    for b, p in enumerate(paths):
        a = np.load(p, allow_pickle=False)
        assert p.endswith(f'utt_{b}.npy') and a.dtype == np.float32 and a.tobytes() == _np(embed)[b].tobytes()
    mpaths = write_mean_speaker_embs(names, means, tmp_path / 'mean_speaker_emb')
    assert [p.rsplit('/', 1)[1] for p in mpaths] == ['p225.npy', 'p226.npy', 'p227.npy']
    for r, p in enumerate(mpaths):
        assert np.load(p, allow_pickle=False).tobytes() == _np(means)[r].tobytes()


@pytest.mark.parametrize('E', [256, 300])
def test_segment_mean_norm_beyond_one_row_chunk(E):
    """ft_spk_segment_mean_norm directly, at the sizes where it takes another path: segments of 1, 64, 65 and 70 rows
    (it normalises rows in chunks of 64), a count that cuts a segment, an index list, E above 256 (two columns per
    thread).  Rows are non-negative (as behind a ReLU), so nothing cancels: a component's relative error is at most n u
    for the n-term sum, (E / 2 + 2) u for each of the two norms and u for each of the three divisions, together below
    (n + E + 8) u of a value of at most 1."""
    from forwardtacotron_amd import hip as H
    rng = np.random.default_rng(E)
    sizes = [1, 64, 65, 70]
    N = sum(sizes)
    rows = np.abs(rng.standard_normal((N, E))).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    count = np.array([1, 64, 65, 66], dtype=np.int64)                       # the last segment is cut to 66 rows
    dev = torch.from_numpy(rows).cuda()
    rows_out = torch.zeros(N, E, device='cuda')
    got = H.spk_segment_mean_norm(dev, None, torch.from_numpy(off).cuda(), torch.from_numpy(count).cuda(), True,
                                  rows_out=rows_out)
    r64 = rows.astype(np.float64)
    unit = r64 / np.linalg.norm(r64, axis=1, keepdims=True)
    for s, (lo, n) in enumerate(zip(off[:-1], count)):
        m = unit[lo:lo + n].mean(axis=0)
        err = np.abs(_np(got)[s].astype(np.float64) - m / np.linalg.norm(m)).max()
        print(f'E {E} segment of {n} rows: error {err:.3e} bound {(n + E + 8) * U:.3e}')
        assert err <= (n + E + 8) * U
        assert np.abs(_np(rows_out)[lo:lo + n].astype(np.float64) - unit[lo:lo + n]).max() <= (E / 2 + 3) * U
    assert not _np(rows_out)[off[3] + 66:].any()                            # rows of no segment are not written
    perm = rng.permutation(N).astype(np.int64)                              # an index list, no row normalisation
    got = H.spk_segment_mean_norm(dev, torch.from_numpy(perm).cuda(), torch.from_numpy(off).cuda(), None, False)
    for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
        m = r64[perm[lo:hi]].mean(axis=0)
        err = np.abs(_np(got)[s].astype(np.float64) - m / np.linalg.norm(m)).max()
        assert err <= (hi - lo + E + 8) * U, (s, err)


def test_errors_are_raised_before_any_launch(enc, fx, monkeypatch):
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd._lib import FtError
    from forwardtacotron_amd.speaker import VoiceEncoder

    def no_launch(name, *a):
        raise AssertionError(f'{name} was launched')
    monkeypatch.setattr(_lib, 'call', no_launch)
    w = fx['wavs'][1]
    with pytest.raises(FtError, match='trim_long_silences'):
        enc.embed_batch([w], trim_long_silences=True)
    with pytest.raises(FtError, match='HIP device'):
        enc.embed_batch([torch.from_numpy(w.copy())])
    with pytest.raises(FtError, match='HIP device'):
        enc.embed_batch(torch.from_numpy(_padded([w])), wav_len=torch.tensor([len(w)]))
    with pytest.raises(FtError, match='empty'):
        enc.embed_batch([])
    with pytest.raises(FtError, match='at least one sample'):
        enc.embed_batch([w, np.zeros(0, np.float32)])
    with pytest.raises(FtError, match='at least one sample'):
        enc.embed_batch(torch.from_numpy(_padded([w, w])).cuda(), wav_len=torch.tensor([len(w), 0]))
    with pytest.raises(FtError, match='wav_len'):
        enc.embed_batch(torch.from_numpy(_padded([w])).cuda(), wav_len=torch.tensor([len(w) + 1]))
    with pytest.raises(FtError):
        VoiceEncoder().embed_batch([w])                        # CPU parameters
