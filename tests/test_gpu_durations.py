"""GPU: duration extraction (forwardtacotron_amd/durations.py, ft_dur_extract) against the reference fixtures
(tests/golden/durations.npz), the float64 DP restatement (tests/durations_cpu.py) on large ragged batches, and the
pipeline end to end into a ForwardTacotron training batch."""
import math
import os

import numpy as np
import pytest
import torch

import durations_cpu as R
from helpers import TINY

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'durations.npz')


def _gold_items():
    g = np.load(GOLD)
    items = []
    for k in range(int(g['n_items'])):
        p = f'{k}/'
        items.append({n: g[p + n] for n in ('x', 'mel', 'att', 'dur', 'att_score', 'align_score', 'cost', 'unique',
                                              'kind')})
    return g, items


def _pack(items, seed=0):
    """ragged items -> padded device batch; padding is junk (attention) / the collator's pad value (mel) / 0 (x)"""
    g = torch.Generator().manual_seed(seed)
    B = len(items)
    Tm = max(it['att'].shape[0] for it in items) + 1
    Tx = max(it['att'].shape[1] for it in items)
    n_mels = items[0]['mel'].shape[0]
    attn = torch.rand(B, Tm, Tx, generator=g)
    mel = torch.full((B, n_mels, Tm), -11.5129)
    x = torch.zeros(B, Tx, dtype=torch.int64)
    for b, it in enumerate(items):
        m, t = it['att'].shape
        attn[b, :m, :t] = torch.from_numpy(it['att'])
        mel[b, :, :m] = torch.from_numpy(it['mel'])
        x[b, :t] = torch.from_numpy(it['x'])
    x_len = torch.tensor([it['att'].shape[1] for it in items])
    mel_len = torch.tensor([it['att'].shape[0] for it in items])
    return attn.cuda(), x.cuda(), x_len, mel.cuda(), mel_len


def _same(a, b, rel=0.):
    """equal within rel, NaN matching NaN"""
    return (math.isnan(a) and math.isnan(b)) or a == pytest.approx(b, rel=rel, abs=0.)


def _check_item(res, b, ref, Tm, Tx, exact_dur):
    dur = res.durations[b].cpu().numpy()
    assert int(dur[:Tx].sum()) == Tm and not dur[Tx:].any()
    assert float(res.cost[b]) == pytest.approx(ref['cost'], rel=1e-9, abs=1e-12)
    if exact_dur:
        np.testing.assert_array_equal(dur[:Tx], ref['dur'])


def test_extract_batch_matches_reference_fixtures():
    from forwardtacotron_amd.durations import DurationExtractor
    g, items = _gold_items()
    ext = DurationExtractor(float(g['threshold']), float(g['shift']), g['silent_phonemes_indices'].tolist())
    res = ext.extract_batch(*_pack(items))
    for b, it in enumerate(items):
        kind = str(it['kind'])
        Tm, Tx = it['att'].shape
        dur = res.durations[b].cpu().numpy()
        assert int(dur.sum()) == Tm, kind
        assert not dur[Tx:].any(), kind
        assert float(res.cost[b]) == float(it['cost']), kind           # the DP's distances are Dijkstra's bit for bit
        r = R.extract(it['x'], it['mel'], it['att'], float(g['threshold']), float(g['shift']),
                      g['silent_phonemes_indices'])
        np.testing.assert_array_equal(dur[:Tx], r['dur'], err_msg=kind)   # same tie rule as the restatement
        if int(it['unique']):
            np.testing.assert_array_equal(dur[:Tx], it['dur'], err_msg=kind)
            ref_att = float(it['att_score'])
            if math.isnan(ref_att):
                assert math.isnan(float(res.att_score[b])), kind
            else:
                assert float(res.att_score[b]) == pytest.approx(ref_att, rel=1e-12), kind
        a_ref = float(it['align_score'])
        a = float(res.align_score[b])
        assert (math.isnan(a_ref) and math.isnan(a)) or a == a_ref, kind
        assert int(res.max_duration[b]) == r['max_duration'], kind
        assert int(res.max_consecutive_ones[b]) == r['max_consecutive_ones'], kind
    assert math.isnan(float(res.att_score[[str(it['kind']) for it in items].index('all_silent')]))


def _random_items(rng, shapes, n_mels=80):
    items = []
    for Tm, Tx in shapes:
        centre = np.linspace(0, Tx - 1, Tm) + rng.normal(0, 2., Tm)
        logits = -0.2 * (np.arange(Tx)[None, :] - centre[:, None]) ** 2 + rng.normal(0, 1., (Tm, Tx))
        att = np.exp(logits - logits.max(1, keepdims=True))
        att = (att / att.sum(1, keepdims=True)).astype(np.float32)
        mel = rng.normal(-6., 3., (n_mels, Tm)).astype(np.float32)
        n_sil = min(40, Tm // 3)
        s = int(rng.integers(0, Tm - n_sil + 1))
        mel[:, s:s + n_sil] = -11.5
        x = rng.integers(0, 60, Tx).astype(np.int64)
        items.append({'att': att, 'mel': mel, 'x': x})
    return items


@pytest.mark.parametrize('shapes', [
    [(1250, 200), (1100, 170), (900, 200), (1250, 31), (640, 120), (1249, 199)],      # back-pointers in LDS
    [(2000, 300), (1250, 200), (300, 80)],                                             # global back-pointers too
])
def test_extract_batch_matches_float64_dp_on_ragged_batches(shapes):
    from forwardtacotron_amd.durations import DurationExtractor
    rng = np.random.default_rng(len(shapes))
    items = _random_items(rng, shapes)
    ext = DurationExtractor(-11., 0.25)
    res = ext.extract_batch(*_pack(items, seed=1))
    for b, it in enumerate(items):
        Tm, Tx = it['att'].shape
        r = R.extract(it['x'], it['mel'], it['att'], -11., 0.25, ext.silent_phonemes_indices)
        _check_item(res, b, r, Tm, Tx, exact_dur=True)
        assert _same(float(res.att_score[b]), r['att_score'], rel=1e-12)
        assert _same(float(res.align_score[b]), r['align_score'])


def test_ragged_batch_equals_per_item_calls():
    from forwardtacotron_amd.durations import DurationExtractor
    rng = np.random.default_rng(5)
    items = _random_items(rng, [(300, 50), (120, 17), (301, 64), (7, 3)], n_mels=20)
    ext = DurationExtractor(-11., 0.25)
    res = ext.extract_batch(*_pack(items, seed=2))
    for b, it in enumerate(items):
        Tx = it['att'].shape[1]
        dur, att_score = ext(torch.from_numpy(it['x']), torch.from_numpy(it['mel']), torch.from_numpy(it['att']))
        assert dur.dtype == torch.float32 and dur.device.type == 'cpu'
        np.testing.assert_array_equal(dur.numpy().astype(np.int64), res.durations[b, :Tx].cpu().numpy())
        assert _same(att_score, float(res.att_score[b]))


def test_bad_lengths_raise():
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd.durations import DurationExtractor
    rng = np.random.default_rng(6)
    attn, x, x_len, mel, mel_len = _pack(_random_items(rng, [(40, 10), (30, 8)], n_mels=20))
    ext = DurationExtractor(-11., 0.25)
    with pytest.raises(_lib.FtError, match='item 1: x_len'):
        ext.extract_batch(attn, x, torch.tensor([10, 11]), mel, mel_len)
    with pytest.raises(_lib.FtError, match='item 0: mel_len'):
        ext.extract_batch(attn, x, x_len, mel, torch.tensor([0, 30]))


class _AttentionStub(torch.nn.Module):
    """stands in for a Tacotron at r = 1: align(batch) returns prepared attentions [B, steps, Tx] on the device"""

    def __init__(self, attn_by_id):
        super().__init__()
        self.attn_by_id = attn_by_id
        self.r = 1
        self.decoder = torch.nn.Module()
        self.decoder.prenet = torch.nn.Module()

    def align(self, batch):
        assert not self.training and self.decoder.prenet.training
        S, Tx = batch['mel'].shape[2], batch['x'].shape[1]
        out = torch.zeros(len(batch['item_id']), S, Tx)
        for b, i in enumerate(batch['item_id']):
            a = self.attn_by_id[i]
            out[b, :a.shape[0], :a.shape[1]] = torch.from_numpy(a)
        return out.cuda()


def test_extract_durations_feeds_forward_tacotron(tmp_path):
    from forwardtacotron_amd import model as M
    from forwardtacotron_amd.datapath import DevicePrefetcher, ForwardCollator, TacoCollator, batches
    from forwardtacotron_amd.durations import DurationExtractor, extract_durations
    rng = np.random.default_rng(7)
    shapes = [(60, 12), (45, 9), (80, 15), (33, 7), (70, 14)]
    raw = _random_items(rng, shapes, n_mels=TINY['n_mels'])
    items = []
    for k, it in enumerate(raw):
        Tm, Tx = it['att'].shape
        items.append({'item_id': f'it{k}', 'x': np.where(it['x'] == 0, 1, it['x']), 'x_len': Tx, 'mel': it['mel'],
                      'mel_len': Tm, 'speaker_emb': np.zeros(1, np.float32), 'speaker_name': 's'})
    model = _AttentionStub({f'it{k}': it['att'] for k, it in enumerate(raw)})
    loader = DevicePrefetcher(batches(items, [it['mel_len'] for it in items], 2, TacoCollator(r=1)), 'cuda')
    ext = DurationExtractor(-11., 0.25)
    stats = extract_durations(model, loader, tmp_path / 'alg', extractor=ext, save_attention=tmp_path / 'att')
    assert set(stats) == {it['item_id'] for it in items}
    for k, it in enumerate(items):
        d = np.load(tmp_path / 'alg' / f"{it['item_id']}.npy")
        assert d.dtype == np.int64 and d.shape == (it['x_len'],) and int(d.sum()) == it['mel_len']
        np.testing.assert_array_equal(np.load(tmp_path / 'att' / f"{it['item_id']}.npy"), raw[k]['att'])
        r = R.extract(it['x'], it['mel'], raw[k]['att'], -11., 0.25, ext.silent_phonemes_indices)
        np.testing.assert_array_equal(d, r['dur'])
        st = stats[it['item_id']]
        assert st.max_duration == r['max_duration'] and st.max_consecutive_ones == r['max_consecutive_ones']
        assert _same(st.att_sharpness_score, r['att_score'], rel=1e-12)
        assert _same(st.att_align_score, r['align_score'])
        it.update(dur=d, pitch=np.zeros(it['x_len'], np.float32), energy=np.zeros(it['x_len'], np.float32),
                  pitch_cond=np.zeros(it['x_len'], np.int64))

    batch = ForwardCollator(TacoCollator(r=1))(items)
    torch.manual_seed(0)
    m = M.ForwardTacotron(**TINY).cuda().eval()
    with torch.no_grad():
        out = m({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})
    torch.cuda.synchronize()
    assert out['mel'].shape[0] == len(items)
    assert out['mel'].shape[-1] >= max(it['mel_len'] for it in items)
    assert torch.isfinite(out['mel']).all()


def test_extract_durations_requires_r1(tmp_path):
    from forwardtacotron_amd import _lib
    from forwardtacotron_amd.durations import extract_durations
    model = _AttentionStub({})
    model.r = 2
    with pytest.raises(_lib.FtError, match='r = 1'):
        extract_durations(model, [], tmp_path)
