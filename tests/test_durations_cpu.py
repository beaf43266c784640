"""CPU: the float64 DP restatement (tests/durations_cpu.py) reproduces the reference DurationExtractor on every item of
tests/golden/durations.npz (made by tests/golden/make_golden_durations.py from the reference), and the C ABI of the
duration kernel is declared."""
import math
import os

import numpy as np
import pytest

import durations_cpu as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden', 'durations.npz')


@pytest.fixture(scope='module')
def gold():
    return np.load(GOLD)


def _items(g):
    for k in range(int(g['n_items'])):
        p = f'{k}/'
        yield k, {n: g[p + n] for n in ('x', 'mel', 'att', 'dur', 'att_score', 'align_score', 'cost', 'unique',
                                          'kind')}


def test_fixture_covers_the_edge_cases(gold):
    kinds = {str(it['kind']) for _, it in _items(gold)}
    assert {'tiny_tacotron', 'diagonal_silences', 'tx1', 'tm1', 'all_silent', 'one_silent_frame',
            'flat_ties'} <= kinds
    shapes = {str(it['kind']): it['att'].shape for _, it in _items(gold)}
    assert shapes['tx1'][1] == 1 and shapes['tm1'][0] == 1
    assert any(int(it['unique']) == 0 for _, it in _items(gold))


def test_silent_phoneme_table_matches_reference(gold):
    from forwardtacotron_amd.durations import SILENT_PHONEME_INDICES
    assert tuple(int(i) for i in gold['silent_phonemes_indices']) == SILENT_PHONEME_INDICES


def test_restatement_matches_reference(gold):
    thr, shift, sil = float(gold['threshold']), float(gold['shift']), gold['silent_phonemes_indices']
    for k, it in _items(gold):
        r = R.extract(it['x'], it['mel'], it['att'], thr, shift, sil)
        kind = str(it['kind'])
        Tm, Tx = it['att'].shape
        assert r['cost'] == float(it['cost']), (k, kind)                      # bit-equal to scipy's Dijkstra
        assert R.is_monotone(r['path'], Tm, Tx)
        assert R.path_cost(r['path'], r['cost_matrix']) == r['cost']
        assert int(r['dur'].sum()) == Tm
        if int(it['unique']):
            np.testing.assert_array_equal(r['dur'], it['dur'], err_msg=f'{k} {kind}')
        if math.isnan(float(it['att_score'])):
            assert kind == 'all_silent' and math.isnan(r['att_score'])
        elif int(it['unique']):
            assert r['att_score'] == pytest.approx(float(it['att_score']), rel=1e-12, abs=1e-12), (k, kind)
        a_ref = float(it['align_score'])
        assert (math.isnan(a_ref) and math.isnan(r['align_score'])) or r['align_score'] == a_ref, (k, kind)


def test_duration_abi_declared():
    from forwardtacotron_amd import _lib
    protos = _lib.parse_header()
    assert protos['ft_dur_workspace'][0] == 'size_t'
    ret, args = protos['ft_dur_extract']
    assert ret == 'int' and [n for _, n in args][-2:] == ['ws', 'stream'] and len(args) == 21
