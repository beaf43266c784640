"""No device: the error paths of the ragged-batch intake (forwardtacotron_amd/ragged.py).  Every refusal is an FtError
raised before the first device operation: the device named here is never touched (without one, touching it would raise
something else than FtError), and the allocator handed to gather_wavs -- its first device operation -- raises Reached,
which only the accepted all-empty batch gets to."""
import numpy as np
import pytest
import torch

from forwardtacotron_amd import ragged
from forwardtacotron_amd._lib import FtError


class Reached(Exception):
    pass


def _no_alloc(*shape, **kw):
    raise Reached


def _lens(lens, B=3, lo=0, hi=13, flag=True):
    return ragged.device_lens(lens, B, lo, hi, 'caller', 'wav_len', 'L', 'cuda', flag=flag)


@pytest.mark.parametrize('flag', [True, False])
def test_device_lens_refuses_wrong_dtype_rank_and_count(flag):
    for bad in (torch.tensor([0, 5, 13], dtype=torch.int32), torch.tensor([0.0, 5.0, 13.0]), np.array([0, 5, 13], np.int32),
                torch.tensor([[0, 5, 13]]), torch.tensor(5), torch.tensor([0, 5]), torch.tensor([0, 5, 13, 1]), [0, 5]):
        with pytest.raises(FtError, match=r'caller: wav_len must be int64 \[B = 3\]'):
            _lens(bad, flag=flag)


@pytest.mark.parametrize('bad', [[0, 5, 14], [-1, 5, 13], [0, 14, 2]])
def test_device_lens_refuses_a_host_length_out_of_range_and_names_the_list(bad):
    for lens in (torch.tensor(bad), np.array(bad, np.int64), bad):
        with pytest.raises(FtError) as e:
            _lens(lens)
        assert str(e.value) == f'caller: every wav_len must be in [0, L = 13] (got {bad})'
    with pytest.raises(FtError, match=r'every mel_len must be in \[1, Tmax = 13\] \(got \[0, 5, 13\]\)'):
        ragged.device_lens(torch.tensor([0, 5, 13]), 3, 1, 13, 'caller', 'mel_len', 'Tmax', 'cuda')
    assert ragged.range_message('caller', 'mel_len', 1, 13, 'Tmax') == 'caller: every mel_len must be in [1, Tmax = 13]'


@pytest.mark.parametrize('allow', [True, False])
def test_gather_wavs_refuses_an_empty_list_and_an_item_that_is_not_1d(allow):
    kw = dict(row_multiple=4, allow_all_empty=allow, alloc=_no_alloc)
    with pytest.raises(FtError, match='caller: an empty batch'):
        ragged.gather_wavs([], 'cuda', 'caller', **kw)
    y = np.zeros(5, np.float32)
    for bad in (np.zeros((2, 5), np.float32), torch.zeros(1, 5), torch.tensor(1.0), 3.0, [1.0, 2.0]):
        with pytest.raises(FtError, match='caller: every wav must be a 1-D array or tensor'):
            ragged.gather_wavs([y, bad], 'cuda', 'caller', **kw)


def test_gather_wavs_all_empty_batch_refused_or_allowed():
    empty = [np.zeros(0, np.float32), torch.zeros(0)]
    with pytest.raises(FtError, match='caller: every wav of the batch is empty'):
        ragged.gather_wavs(empty, 'cuda', 'caller', allow_all_empty=False, alloc=_no_alloc)
    with pytest.raises(Reached):                                # accepted: it goes on to allocate [2, 1]
        ragged.gather_wavs(empty, 'cuda', 'caller', allow_all_empty=True, alloc=_no_alloc)
    with pytest.raises(Reached):                                # one sample somewhere is no all-empty batch
        ragged.gather_wavs(empty + [np.zeros(1, np.float32)], 'cuda', 'caller', allow_all_empty=False, alloc=_no_alloc)


def test_intake_refuses_a_padded_batch_without_lengths_of_another_type_or_empty():
    pad = np.zeros((3, 13), np.float32)
    kw = dict(alloc=_no_alloc)
    for wavs in (pad, torch.from_numpy(pad)):
        with pytest.raises(FtError, match='caller: a padded .* batch needs wav_len'):
            ragged.intake(wavs, None, 'cuda', 'caller', **kw)
    for bad in (torch.zeros(3, 13, dtype=torch.float64), torch.zeros(13), torch.zeros(1, 3, 13), [pad[0], pad[1], pad[2]]):
        with pytest.raises(FtError, match='caller: with wav_len, the batch must be a float32'):
            ragged.intake(bad, torch.tensor([0, 5, 13]), 'cuda', 'caller', **kw)
    with pytest.raises(FtError, match='caller: an empty batch'):
        ragged.intake(torch.zeros(0, 13), torch.zeros(0, dtype=torch.int64), 'cuda', 'caller', **kw)
    with pytest.raises(FtError, match='caller: an empty batch'):                 # L == 0 where an all-empty batch is refused
        ragged.intake(torch.zeros(3, 0), torch.zeros(3, dtype=torch.int64), 'cuda', 'caller', allow_all_empty=False, **kw)
    for flag in (True, False):                                                  # the lengths are checked as device_lens does
        with pytest.raises(FtError, match=r'caller: every wav_len must be in \[0, L = 13\] \(got \[0, 5, 14\]\)'):
            ragged.intake(pad, [0, 5, 14], 'cuda', 'caller', flag=flag, **kw)
        with pytest.raises(FtError, match=r'caller: wav_len must be int64 \[B = 3\]'):
            ragged.intake(pad, torch.tensor([0, 5]), 'cuda', 'caller', flag=flag, **kw)
    with pytest.raises(Reached):                                                # a list goes on to gather_wavs' allocation
        ragged.intake([pad[0], pad[1, :5]], None, 'cuda', 'caller', **kw)


def test_the_flag_read_back_ignores_host_side_lengths():
    ragged.LenFlag().check(None, 'never raised')               # no flag: no pinned word, no synchronisation
