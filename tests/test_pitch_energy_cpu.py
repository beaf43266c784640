"""CPU: the float64 restatement of the per-token pitch / energy targets (tests/pitch_energy_cpu.py) reproduces the files
the reference's extract_pitch_energy wrote (tests/golden/pitch_energy.npz, made by
tests/golden/make_golden_pitch_energy.py), and the C ABI of the kernels is declared."""
import math
import os
import re

import numpy as np
import pytest

import pitch_energy_cpu as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'pitch_energy.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _items(g):
    for k, item_id in enumerate(g['item_ids']):
        p = f'{item_id}/'
        it = {'id': str(item_id), 'speaker': str(g['speakers'][k]), 'case': str(g['case'][k]),
              'mel': g[p + 'mel'], 'mel_len': int(g[p + 'mel_len']), 'dur': g[p + 'dur'],
              'raw_pitch': g[p + 'raw_pitch']}
        if p + 'phon_pitch' in g.files:
            it['phon_pitch'], it['phon_energy'] = g[p + 'phon_pitch'], g[p + 'phon_energy']
        yield it


def test_fixture_covers_the_cases(gold):
    items = list(_items(gold))
    cases = {it['case'] for it in items}
    assert {'plain', 'zero_durations', 'short_raw_pitch', 'pitch_out_of_range', 'x_len_gt_mel_len',
            'durations_do_not_sum', 'one_char_speaker', 'all_zero_pitch'} <= cases
    for it in items:
        written = 'phon_pitch' in it
        assert written == (it['case'] not in ('durations_do_not_sum', 'one_char_speaker')), it['id']
        if written:
            assert it['phon_pitch'].dtype == np.float32 and it['phon_pitch'].shape == it['dur'].shape
            assert it['phon_energy'].dtype == np.float32 and it['phon_energy'].shape == it['dur'].shape
    assert len({it['speaker'] for it in items}) >= 4
    assert sorted(str(s) for s in gold['stat_speakers']) == ['alice', 'bob', 'dora']


def test_restatement_matches_reference(gold):
    fmin, fmax = float(gold['fmin']), float(gold['fmax'])
    pitches = {}
    for it in _items(gold):
        r = R.token_values(it['mel'], it['mel_len'], it['raw_pitch'], it['dur'], fmin, fmax)
        if it['case'] == 'durations_do_not_sum':
            assert r is None
            continue
        assert r is not None
        if len(it['speaker']) > 1:
            pitches.setdefault(it['speaker'], []).append((it, r[0]))
            np.testing.assert_allclose(it['phon_energy'], r[1], rtol=2e-6, atol=0, err_msg=it['id'])
            np.testing.assert_array_equal(it['phon_energy'] == 0, r[1] == 0, err_msg=it['id'])
    for s, mean_ref, std_ref in zip(gold['stat_speakers'], gold['stat_mean'], gold['stat_std']):
        entries = pitches[str(s)]
        mean, std = R.speaker_stats([p for _, p in entries])
        if math.isnan(float(mean_ref)):
            assert math.isnan(mean) and std == 1e10 and float(std_ref) == 1e10
        else:
            assert mean == pytest.approx(float(mean_ref), rel=2e-6)
            assert std == pytest.approx(float(std_ref), rel=2e-6)
        for it, p in entries:
            np.testing.assert_allclose(it['phon_pitch'], R.normalize(p, mean, std), rtol=0, atol=1e-5,
                                       err_msg=it['id'])
            np.testing.assert_array_equal(it['phon_pitch'] == 0, p == 0, err_msg=it['id'])


def test_quirks_of_the_reference_are_in_the_fixture(gold):
    items = {it['id']: it for it in _items(gold)}
    x = items['bob_001']                                # mel_len 6 < x_len 9: tokens 6.. stay 0 despite durations
    assert x['mel_len'] < len(x['dur']) and x['dur'][6:].any()
    assert not x['phon_energy'][x['mel_len']:].any() and x['phon_energy'][:x['mel_len']].any()
    z = items['alice_001']                              # zero-duration tokens give 0
    assert (z['phon_energy'][z['dur'] == 0] == 0).all() and (z['phon_energy'][z['dur'] > 0] > 0).all()
    d = items['dora_000']
    assert not d['phon_pitch'].any() and (d['phon_energy'][d['dur'] > 0] > 0).all()


def test_token_value_abi_declared():
    from forwardtacotron_amd import _lib
    protos = _lib.parse_header()
    assert protos['ft_token_values_workspace'][0] == 'size_t' and protos['ft_pitch_norm_workspace'][0] == 'size_t'
    ret, args = protos['ft_token_values']
    assert ret == 'int' and [n for _, n in args][-2:] == ['ws', 'stream'] and len(args) == 18
    ret, args = protos['ft_pitch_norm']
    assert ret == 'int' and [n for _, n in args] == ['values', 'n', 'stats', 'ws', 'stream']
    assert re.search(r'#define FWDTACO_ABI_VERSION (\d+)', open(_lib.HEADER_PATH).read()).group(1) == '8'
