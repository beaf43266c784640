"""GPU: per-token pitch and energy (forwardtacotron_amd/pitch_energy.py, ft_token_values / ft_pitch_norm) against the
files the reference wrote (tests/golden/pitch_energy.npz), the float64 restatement (tests/pitch_energy_cpu.py), and
create_align_features end to end into a ForwardTacotron train step.

Bound against the reference: a frame energy is the same fp32 sum except for the exp (the device's expf and numpy's
each round differently), and numpy averages a segment in fp32 pairwise sums where the kernel sums in fp64 and rounds
once: token energies and pitches agree to ULPS = 8 fp32 ulps."""
import os
import pickle

import numpy as np
import pytest
import torch

import pitch_energy_cpu as R
from helpers import TINY, TRAIN_CFG

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'pitch_energy.npz')
ULPS = 8


def _gold():
    g = np.load(GOLD)
    items = {}
    for k, item_id in enumerate(g['item_ids']):
        p = f'{item_id}/'
        it = {'speaker': str(g['speakers'][k]), 'split': int(g['split'][k]), 'case': str(g['case'][k]),
              'mel': g[p + 'mel'], 'mel_len': int(g[p + 'mel_len']), 'dur': g[p + 'dur'],
              'raw_pitch': g[p + 'raw_pitch']}
        if p + 'phon_pitch' in g.files:
            it['phon_pitch'], it['phon_energy'] = g[p + 'phon_pitch'], g[p + 'phon_energy']
        items[str(item_id)] = it
    stats = {str(s): (float(m), float(d)) for s, m, d in zip(g['stat_speakers'], g['stat_mean'], g['stat_std'])}
    return float(g['fmin']), float(g['fmax']), items, stats


def _within_ulps(got, ref, ulps, msg=''):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    np.testing.assert_array_equal(got == 0, ref == 0, err_msg=msg)
    bound = ulps * np.spacing(np.abs(ref))
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all(), (msg, np.max(np.abs(got - ref) / np.spacing(
        np.maximum(np.abs(ref), 1e-30))))


def _pack(items, pad_frames=3):
    """items (mel, mel_len, raw_pitch, dur) -> padded device batch with junk padding"""
    B = len(items)
    n_mels = items[0]['mel'].shape[0]
    Tm = max(it['mel'].shape[1] for it in items) + pad_frames
    Tp = max(len(it['raw_pitch']) for it in items) + 2
    Tx = max(len(it['dur']) for it in items) + 1
    mel = torch.full((B, n_mels, Tm), 7.0)
    pitch = torch.full((B, Tp), 200.0)
    dur = torch.full((B, Tx), 5, dtype=torch.int64)
    for b, it in enumerate(items):
        mel[b, :, :it['mel'].shape[1]] = torch.from_numpy(it['mel'])
        pitch[b, :len(it['raw_pitch'])] = torch.from_numpy(it['raw_pitch'])
        dur[b, :len(it['dur'])] = torch.from_numpy(it['dur'])
    mel_len = torch.tensor([it['mel_len'] for it in items])
    pitch_len = torch.tensor([len(it['raw_pitch']) for it in items])
    x_len = torch.tensor([len(it['dur']) for it in items])
    return mel.cuda(), mel_len, pitch.cuda(), pitch_len, dur.cuda(), x_len


def test_extract_batch_matches_reference_token_values():
    from forwardtacotron_amd.pitch_energy import SKIPPED, TokenValues
    fmin, fmax, items, stats = _gold()
    ids = sorted(items)
    res = TokenValues.extract_batch(*_pack([items[i] for i in ids]), fmin, fmax)
    st = res.status.cpu().numpy()
    P = res.pitch.cpu().numpy()
    E = res.energy.cpu().numpy()
    for b, i in enumerate(ids):
        it = items[i]
        xl = len(it['dur'])
        assert not P[b, xl:].any() and not E[b, xl:].any()
        if it['case'] == 'durations_do_not_sum':
            assert st[b] == SKIPPED and not P[b].any() and not E[b].any()
            continue
        assert st[b] == 0, i
        r = R.token_values(it['mel'], it['mel_len'], it['raw_pitch'], it['dur'], fmin, fmax)
        _within_ulps(P[b, :xl], r[0], 2, i)                 # fp64 segment sums of exact fp32 pitches: one rounding
        if 'phon_energy' in it:
            _within_ulps(E[b, :xl], it['phon_energy'], ULPS, i)
            if it['speaker'] in stats:                      # normalised with the reference's own fp32 mean / std
                mean, std = (np.float32(v) for v in stats[it['speaker']])
                p = P[b, :xl]
                expect = np.where(p != 0, (p - mean) / std, np.float32(0))
                np.testing.assert_allclose(expect, it['phon_pitch'], rtol=0, atol=1e-5, err_msg=i)


def _write_tree(root, items, order=None):
    for d in ('mel', 'alg', 'raw_pitch'):
        os.makedirs(root / d, exist_ok=True)
    for i, it in items.items():
        np.save(root / 'mel' / f'{i}.npy', it['mel'])
        np.save(root / 'alg' / f'{i}.npy', it['dur'])
        np.save(root / 'raw_pitch' / f'{i}.npy', it['raw_pitch'])
    ids = list(order or sorted(items))
    for name, obj in (('speaker_dict.pkl', {i: it['speaker'] for i, it in items.items()}),
                      ('train_dataset.pkl', [(i, items[i]['mel_len']) for i in ids if items[i]['split'] == 0]),
                      ('val_dataset.pkl', [(i, items[i]['mel_len']) for i in ids if items[i]['split'] == 1])):
        with open(root / name, 'wb') as f:
            pickle.dump(obj, f)


def _run(root, out, fmin, fmax, **kw):
    from forwardtacotron_amd.pitch_energy import extract_pitch_energy
    return extract_pitch_energy(root / 'speaker_dict.pkl', root / 'train_dataset.pkl', root / 'val_dataset.pkl',
                                root / 'alg', root / 'mel', root / 'raw_pitch', out / 'phon_pitch',
                                out / 'phon_energy', fmin, fmax, **kw)


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_extract_pitch_energy_matches_reference_files(tmp_path):
    fmin, fmax, items, stats = _gold()
    _write_tree(tmp_path, items)
    got = _run(tmp_path, tmp_path / 'out', fmin, fmax)
    pitch, energy = _files(tmp_path / 'out' / 'phon_pitch'), _files(tmp_path / 'out' / 'phon_energy')
    expect = {i for i, it in items.items() if 'phon_pitch' in it}
    assert set(pitch) == expect and set(energy) == expect
    for i in expect:
        for d, ref in ((pitch[i], items[i]['phon_pitch']), (energy[i], items[i]['phon_energy'])):
            assert d.dtype == np.float32 and d.shape == ref.shape
        np.testing.assert_allclose(pitch[i], items[i]['phon_pitch'], rtol=0, atol=1e-5, err_msg=i)
        np.testing.assert_array_equal(pitch[i] == 0, items[i]['phon_pitch'] == 0, err_msg=i)
        _within_ulps(energy[i], items[i]['phon_energy'], ULPS, i)
    assert set(got) == set(stats)
    for s, (mean, std) in stats.items():
        m, d = got[s]
        assert (np.isnan(mean) and np.isnan(m)) or m == pytest.approx(mean, rel=2e-6), s
        assert d == pytest.approx(std, rel=2e-6), s


def test_batching_and_order_give_identical_files(tmp_path):
    fmin, fmax, items, _ = _gold()
    _write_tree(tmp_path / 'a', items)
    _write_tree(tmp_path / 'b', items, order=sorted(items, reverse=True))
    runs = [_run(tmp_path / 'a', tmp_path / 'o1', fmin, fmax),
            _run(tmp_path / 'a', tmp_path / 'o2', fmin, fmax, batch_size=1),
            _run(tmp_path / 'b', tmp_path / 'o3', fmin, fmax, batch_size=3)]
    assert all(r.keys() == runs[0].keys() for r in runs)
    for r in runs[1:]:
        for s in r:
            np.testing.assert_array_equal(np.float32(r[s]), np.float32(runs[0][s]))
    for d in ('phon_pitch', 'phon_energy'):
        ref = _files(tmp_path / 'o1' / d)
        for o in ('o2', 'o3'):
            got = _files(tmp_path / o / d)
            assert got.keys() == ref.keys()
            for i in ref:
                assert got[i].tobytes() == ref[i].tobytes(), (d, o, i)


def test_ragged_batch_with_workspace_item_equals_single_calls():
    """one item longer than the LDS holds (8192 frames) takes the global workspace; every item alone gives the same
    bits, and the values match the float64 restatement"""
    from forwardtacotron_amd.pitch_energy import TokenValues
    rng = np.random.default_rng(3)
    items = []
    for Tm, Tx in ((9000, 700), (800, 150), (1, 1), (300, 400), (8192, 40)):
        w = rng.gamma(2., 1., Tx) * (rng.random(Tx) > 0.1) + 1e-3
        d = rng.multinomial(Tm, w / w.sum()).astype(np.int64)
        p = rng.uniform(20., 700., Tm).astype(np.float32)
        p[rng.random(Tm) < 0.3] = 0.
        items.append({'mel': rng.normal(-5., 2., (8, Tm)).astype(np.float32), 'mel_len': Tm, 'dur': d,
                      'raw_pitch': p[:max(1, Tm - 17)]})
    res = TokenValues.extract_batch(*_pack(items), 30., 600.)
    assert not res.status.cpu().numpy().any()
    for b, it in enumerate(items):
        one = TokenValues.extract_batch(*_pack([it], pad_frames=0), 30., 600.)
        xl = len(it['dur'])
        for a, c in ((res.pitch, one.pitch), (res.energy, one.energy)):
            assert a[b, :xl].cpu().numpy().tobytes() == c[0, :xl].cpu().numpy().tobytes()
        r = R.token_values(it['mel'], it['mel_len'], it['raw_pitch'], it['dur'], 30., 600.)
        _within_ulps(res.pitch[b, :xl].cpu().numpy(), r[0], 2, b)
        np.testing.assert_allclose(res.energy[b, :xl].cpu().numpy(), r[1], rtol=1e-5, atol=0)


def test_normalize_pitch_over_many_slabs():
    from forwardtacotron_amd.pitch_energy import normalize_pitch
    rng = np.random.default_rng(4)
    v = rng.normal(150., 40., 1_000_003).astype(np.float32)
    v[rng.random(v.size) < 0.25] = 0.
    t = torch.from_numpy(v).cuda()
    mean, std = normalize_pitch(t)
    m64, s64 = R.speaker_stats([v])
    assert mean == pytest.approx(m64, rel=1e-7) and std == pytest.approx(s64, rel=2e-6)
    expect = np.where(v != 0, (v - np.float32(mean)) / np.float32(std), np.float32(0))
    assert t.cpu().numpy().tobytes() == expect.astype(np.float32).tobytes()
    z = torch.zeros(17, device='cuda')
    mean, std = normalize_pitch(z)
    assert np.isnan(mean) and std == 1e10 and not z.any()


class _AttentionStub(torch.nn.Module):
    """stands in for a Tacotron at r = 1: align(batch) returns prepared attentions [B, steps, Tx] on the device"""

    def __init__(self, attn_by_id):
        super().__init__()
        self.attn_by_id = attn_by_id
        self.r = 1
        self.decoder = torch.nn.Module()
        self.decoder.prenet = torch.nn.Module()

    def align(self, batch):
        S, Tx = batch['mel'].shape[2], batch['x'].shape[1]
        out = torch.zeros(len(batch['item_id']), S, Tx)
        for b, i in enumerate(batch['item_id']):
            a = self.attn_by_id[i]
            out[b, :a.shape[0], :a.shape[1]] = torch.from_numpy(a)
        return out.cuda()


def test_create_align_features_equals_the_two_stages(tmp_path):
    from forwardtacotron_amd import model as M
    from forwardtacotron_amd.datapath import DevicePrefetcher, ForwardCollator, TacoCollator, batches
    from forwardtacotron_amd.durations import DurationExtractor, extract_durations
    from forwardtacotron_amd.pitch_energy import create_align_features
    from forwardtacotron_amd.trainer import TrainStep
    rng = np.random.default_rng(8)
    n_mels = TINY['n_mels']
    items, attn = [], {}
    for k, (Tm, Tx) in enumerate([(60, 12), (45, 9), (80, 15), (33, 7), (70, 14), (52, 11)]):
        centre = np.linspace(0, Tx - 1, Tm) + rng.normal(0, 1., Tm)
        logits = -0.3 * (np.arange(Tx)[None, :] - centre[:, None]) ** 2 + rng.normal(0, 0.5, (Tm, Tx))
        a = np.exp(logits - logits.max(1, keepdims=True))
        item_id = f'it{k}'
        attn[item_id] = (a / a.sum(1, keepdims=True)).astype(np.float32)
        mel = rng.normal(-6., 2., (n_mels, Tm)).astype(np.float32)
        items.append({'item_id': item_id, 'x': rng.integers(12, 60, Tx), 'x_len': Tx, 'mel': mel, 'mel_len': Tm,
                      'speaker_emb': np.zeros(1, np.float32), 'speaker_name': ('anna', 'ben', 'c')[k % 3],
                      'split': k % 2})
    (tmp_path / 'raw_pitch').mkdir()
    (tmp_path / 'mel').mkdir()
    for it in items:
        p = rng.uniform(60., 400., it['mel_len'] - 3).astype(np.float32)
        p[rng.random(p.size) < 0.3] = 0.
        np.save(tmp_path / 'raw_pitch' / f"{it['item_id']}.npy", p)
        np.save(tmp_path / 'mel' / f"{it['item_id']}.npy", it['mel'])

    def loader():
        return DevicePrefetcher(batches(items, [it['mel_len'] for it in items], 4, TacoCollator(r=1)), 'cuda')

    ext = DurationExtractor(-11., 0.25)
    dstats, pstats = create_align_features(_AttentionStub(attn), loader(), tmp_path / 'alg', tmp_path / 'raw_pitch',
                                           tmp_path / 'phon_pitch', tmp_path / 'phon_energy', 30., 600.,
                                           extractor=ext)
    ref_stats = extract_durations(_AttentionStub(attn), loader(), tmp_path / 'alg_ref', extractor=ext)
    assert dstats == ref_stats
    alg, alg_ref = _files(tmp_path / 'alg'), _files(tmp_path / 'alg_ref')
    assert alg.keys() == alg_ref.keys() == {it['item_id'] for it in items}
    for i in alg:
        assert alg[i].dtype == np.int64 and alg[i].tobytes() == alg_ref[i].tobytes()

    pickles = {'speaker_dict.pkl': {it['item_id']: it['speaker_name'] for it in items},
               'train_dataset.pkl': [(it['item_id'], it['mel_len']) for it in items if it['split'] == 0],
               'val_dataset.pkl': [(it['item_id'], it['mel_len']) for it in items if it['split'] == 1]}
    for name, obj in pickles.items():
        with open(tmp_path / name, 'wb') as f:
            pickle.dump(obj, f)
    from forwardtacotron_amd.pitch_energy import extract_pitch_energy
    ref_p = extract_pitch_energy(tmp_path / 'speaker_dict.pkl', tmp_path / 'train_dataset.pkl',
                                 tmp_path / 'val_dataset.pkl', tmp_path / 'alg_ref', tmp_path / 'mel',
                                 tmp_path / 'raw_pitch', tmp_path / 'ref' / 'phon_pitch', tmp_path / 'ref' / 'phon_energy',
                                 30., 600.)
    assert pstats == ref_p and set(pstats) == {'anna', 'ben'}
    for d in ('phon_pitch', 'phon_energy'):
        got, ref = _files(tmp_path / d), _files(tmp_path / 'ref' / d)
        assert got.keys() == ref.keys() == {it['item_id'] for it in items if it['speaker_name'] != 'c'}
        for i in got:
            assert got[i].dtype == np.float32 and got[i].shape == alg[i].shape
            assert got[i].tobytes() == ref[i].tobytes(), (d, i)

    # the ForwardDataset layout (utils/dataset.py:137-143) into a ForwardTacotron train step
    train = [it for it in items if it['speaker_name'] != 'c']
    pitch, energy = _files(tmp_path / 'phon_pitch'), _files(tmp_path / 'phon_energy')
    for it in train:
        p = pitch[it['item_id']]
        it.update(dur=alg[it['item_id']], pitch=p, energy=energy[it['item_id']],
                  pitch_cond=np.where(p != 0, 2, 1).astype(np.int64))
    batch = ForwardCollator(TacoCollator(r=1))(train)
    torch.manual_seed(0)
    model = M.ForwardTacotron(**TINY).cuda()
    out = TrainStep(model, lr=1e-3, train_cfg=TRAIN_CFG).step(
        {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})
    torch.cuda.synchronize()
    assert np.isfinite(float(out['loss']))


def test_bad_inputs_raise():
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd.pitch_energy import TokenValues, create_align_features
    rng = np.random.default_rng(9)
    items = [{'mel': rng.normal(-5., 1., (8, m)).astype(np.float32), 'mel_len': m,
              'dur': rng.multinomial(m, np.ones(x) / x).astype(np.int64), 'raw_pitch': np.full(m, 100., np.float32)}
             for m, x in ((20, 5), (30, 7))]
    mel, mel_len, pitch, pitch_len, dur, x_len = _pack(items)
    with pytest.raises(_lib.FtError, match='item 1: x_len'):
        TokenValues.extract_batch(mel, mel_len, pitch, pitch_len, dur, torch.tensor([5, 9]), 30., 600.)
    with pytest.raises(_lib.FtError, match='item 0: mel_len'):
        TokenValues.extract_batch(mel, torch.tensor([0, 30]), pitch, pitch_len, dur, x_len, 30., 600.)
    with pytest.raises(_lib.FtError, match='item 1: mel_len'):
        TokenValues.extract_batch(mel, torch.tensor([20, mel.shape[2] + 1]), pitch, pitch_len, dur, x_len, 30., 600.)
    with pytest.raises(_lib.FtError, match='item 0: pitch_len'):
        TokenValues.extract_batch(mel, mel_len, pitch, torch.tensor([pitch.shape[1] + 1, 30]), dur, x_len, 30., 600.)
    bad = dur.clone()
    bad[1, :2] = torch.tensor([-1, int(dur[1, 0]) + int(dur[1, 1]) + 1])      # the sum still equals mel_len
    with pytest.raises(_lib.FtError, match='item 1: a duration is negative'):
        TokenValues.extract_batch(mel, mel_len, pitch, pitch_len, bad, x_len, 30., 600.)
    with pytest.raises(_lib.FtError, match='batch sizes differ'):
        TokenValues.extract_batch(mel, mel_len, pitch[:1], pitch_len, dur, x_len, 30., 600.)
    with pytest.raises(_lib.FtError, match='must be'):
        TokenValues.extract_batch(mel, mel_len[:1], pitch, pitch_len, dur, x_len, 30., 600.)
    with pytest.raises(_lib.FtError, match='expected'):
        TokenValues.extract_batch(mel, mel_len, pitch, pitch_len, dur.float(), x_len, 30., 600.)
    model = _AttentionStub({})
    model.r = 2
    with pytest.raises(_lib.FtError, match='r = 1'):
        create_align_features(model, [], 'alg', 'raw_pitch', 'pp', 'pe', 30., 600.)
