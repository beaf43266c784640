"""GPU: Griffin-Lim on a ragged batch (vocoder.GriffinLim.griffinlim_batch, the *_ragged kernels of csrc/ft_dsp.hip) against
the numpy oracle (oracle/gl_oracle.py) applied item by item, against the per-item path, and against itself: an item's
samples are bit-identical alone and inside any batch, and a NaN item or NaN padding changes no other item's bits.

Two DSP settings: the project's (n_fft 1024, hop 256, win 1024, 80 mels) and a small one with win < n_fft and another
overlap ratio (n_fft 512, hop 128, win 400, 40 mels).  Frame counts [1, 2, 3, 5, 37, 64], shuffled: the empty wav (one
frame), items shorter than n_fft / hop frames (head and tail of the window sum overlap), an item that straddles a
128-row GEMM tile (rows 67 .. 130), and the longest item not last.

Tolerances are those of tests/test_gpu_vocoder.py (2e-4 relative for the mel inversion; 1e-4 / 2e-4 / 1e-3 for 0 / 1 / 3
iterations): the same algorithm at the same K.  Every comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

from poison import poison as _poison

pytestmark = pytest.mark.gpu

LENS = [5, 64, 1, 37, 2, 3]
SETTINGS = {
    'project': dict(num_mels=80, sample_rate=22050, hop_length=256, win_length=1024, n_fft=1024, fmin=0, fmax=8000),
    'small': dict(num_mels=40, sample_rate=22050, hop_length=128, win_length=400, n_fft=512, fmin=0, fmax=8000),
}


def _signal(n, seed):
    t = np.arange(n) / 22050.0
    rng = np.random.default_rng(seed)
    return (0.5 * np.sin(2 * np.pi * 440 * t) + 0.2 * np.sin(2 * np.pi * 1200 * t) * np.exp(-3 * t)
            + 0.05 * rng.standard_normal(n)).astype(np.float32)


class Case:
    """one DSP setting: the items, their oracle spectra, and everything packed in the batch layout (built once)"""

    def __init__(self, name):
        from oracle import gl_oracle as G
        from forwardtacotron_amd.vocoder import GriffinLim, gl_batch_geometry
        d = SETTINGS[name]
        self.name, self.d = name, d
        self.n_fft, self.hop, self.win, self.C = d['n_fft'], d['hop_length'], d['win_length'], d['num_mels']
        self.gl = GriffinLim(**d)
        self.F, self.Fp = self.gl.F, self.gl.Fp
        self.Tmax = max(LENS)
        self.Tcap = gl_batch_geometry(len(LENS), self.Tmax, self.n_fft, self.hop)['Tcap']
        basis = G.mel_filterbank(d['sample_rate'], self.n_fft, self.C, d['fmin'], d['fmax'])
        self.S, self.u, self.mel = [], [], []
        for i, N in enumerate(LENS):
            S = np.abs(G.stft(_signal(self.hop * (N - 1) + self.hop // 2, 10 + i), self.n_fft, self.hop, self.win))
            assert S.shape == (self.F, N)
            self.S.append(S)
            self.u.append(np.random.default_rng(100 + i).random(S.shape))
            self.mel.append(np.log(np.clip(basis @ S, 1e-5, None)).astype(np.float32))
        self.mel_len = torch.tensor(LENS, dtype=torch.int64)

    def rows(self, items, Tcap=None):
        """list of [F, N_b] arrays -> packed [B * Tcap, Fp] device tensor, zero elsewhere"""
        Tcap = Tcap or self.Tcap
        out = np.zeros((len(items) * Tcap, self.Fp), dtype=np.float32)
        for b, a in enumerate(items):
            out[b * Tcap:b * Tcap + a.shape[1], :self.F] = a.T
        return torch.from_numpy(out).cuda()

    def mel_batch(self, order=None, pad=-11.5129):
        order = list(range(len(LENS))) if order is None else order
        Tm = max(LENS[i] for i in order)
        m = np.full((len(order), self.C, Tm), pad, dtype=np.float32)
        for b, i in enumerate(order):
            m[b, :, :LENS[i]] = self.mel[i]
        return torch.from_numpy(m).cuda(), torch.tensor([LENS[i] for i in order], dtype=torch.int64)

    def alone_geometry(self, i):
        from forwardtacotron_amd.vocoder import gl_batch_geometry
        return gl_batch_geometry(1, LENS[i], self.n_fft, self.hop)['Tcap']


_cases = {}


@pytest.fixture(scope='module', params=list(SETTINGS))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


@pytest.fixture(scope='module')
def project():
    if 'project' not in _cases:
        _cases['project'] = Case('project')
    return _cases['project']


def _item(out, b):
    return out['wav'][b, :int(out['wav_len'][b])]


# ---- 1. oracle -------------------------------------------------------------------------------------------------------
def test_mel_inversion_matches_the_oracle_item_by_item(case):
    from oracle import gl_oracle as G
    d, gl = case.d, case.gl
    mel, ml = case.mel_batch()
    X = gl.mel_to_stft_batch(mel, ml).cpu().numpy()
    assert X.shape == (len(LENS) * case.Tcap, case.Fp) and float(X.min()) >= 0.0
    assert float(np.abs(X[:, case.F:]).max()) == 0.0
    for b, N in enumerate(LENS):
        want = G.mel_to_stft(np.exp(case.mel[b].astype(np.float64)), d['sample_rate'], case.n_fft, d['fmin'], d['fmax'],
                             nnls_iter=gl.nnls_iter)
        got = X[b * case.Tcap:b * case.Tcap + N, :case.F].T
        err = float(np.abs(got - want).max() / np.abs(want).max())
        print(f'{case.name} mel inversion item {b} (N {N}): rel err {err:.3e}')
        assert err < 2e-4, (b, N, err)
        assert not X[b * case.Tcap + N:(b + 1) * case.Tcap].any()           # NNLS is row-local: zero rows stay zero


def test_griffinlim_from_stft_batch_matches_the_oracle_for_a_few_iterations(case):
    from oracle import gl_oracle as G
    gl = case.gl
    Sd, ud = case.rows(case.S), case.rows(case.u)
    for n_iter, tol in ((0, 1e-4), (1, 2e-4), (3, 1e-3)):
        out = gl.griffinlim_from_stft_batch(Sd, case.mel_len, case.Tmax, n_iter, init_u=ud)
        assert out['wav'].shape == (len(LENS), case.hop * (case.Tmax - 1)) and out['wav'].dtype == torch.float32
        assert out['wav_len'].dtype == torch.int64 and out['wav_len'].tolist() == [case.hop * (N - 1) for N in LENS]
        for b, N in enumerate(LENS):
            want = G.griffinlim(case.S[b], n_iter, case.hop, case.win, case.u[b])
            got = _item(out, b).cpu().numpy()
            assert got.shape == want.shape == (case.hop * (N - 1),)
            if N > 1:
                err = float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))
                print(f'{case.name} n_iter {n_iter} item {b} (N {N}): err {err:.3e} (bound {tol:.0e})')
                assert err < tol, (n_iter, b, N, err)


# ---- 2. the per-item path --------------------------------------------------------------------------------------------
def test_batched_item_matches_the_per_item_path(case):
    gl = case.gl
    out = gl.griffinlim_from_stft_batch(case.rows(case.S), case.mel_len, case.Tmax, 3, init_u=case.rows(case.u))
    for b, N in enumerate(LENS):
        one = gl.griffinlim_from_stft(case.rows([case.S[b]], Tcap=N), 3, init_u=case.rows([case.u[b]], Tcap=N))
        got = _item(out, b)
        assert got.shape == one.shape == (case.hop * (N - 1),)
        if N > 1:
            err = float((got - one).abs().max() / max(1.0, float(one.abs().max())))
            print(f'{case.name} item {b} (N {N}) against griffinlim_from_stft: err {err:.3e}')
            assert err < 1e-3, (b, N, err)


# ---- 3. composition invariance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('phases', ['init_u', 'seed'])
def test_an_item_gives_the_same_bits_alone_in_a_batch_and_in_the_reversed_batch(case, phases):
    gl, B = case.gl, len(LENS)

    def run(order):
        mel, ml = case.mel_batch(order)
        if phases == 'seed':
            return gl.griffinlim_batch(mel, ml, n_iter=4, seed=1234)
        Tm = max(LENS[i] for i in order)
        Tcap = case.Tcap if len(order) > 1 else case.alone_geometry(order[0])
        assert Tcap == Tm - 1 + case.n_fft // case.hop
        return gl.griffinlim_batch(mel, ml, n_iter=4, init_u=case.rows([case.u[i] for i in order], Tcap=Tcap))

    full, rev = run(list(range(B))), run(list(range(B))[::-1])
    for i, N in enumerate(LENS):
        alone = run([i])
        assert alone['wav'].shape == (1, case.hop * (N - 1)) and int(alone['wav_len'][0]) == case.hop * (N - 1)
        assert torch.equal(_item(alone, 0), _item(full, i)), (phases, i, N)
        assert torch.equal(_item(full, i), _item(rev, B - 1 - i)), (phases, i, N)
        assert N == 1 or bool(torch.isfinite(_item(full, i)).all())


# ---- 4. leakage and poison ---------------------------------------------------------------------------------------------
def test_nan_and_inf_items_nan_padding_and_poisoned_buffers_change_no_other_item(case, monkeypatch):
    from forwardtacotron_amd import vocoder
    gl, B = case.gl, len(LENS)
    mel, ml = case.mel_batch()
    clean = gl.griffinlim_batch(mel, ml, n_iter=2, seed=7)
    clean_S = gl.mel_to_stft_batch(mel, ml)
    bad, _ = case.mel_batch(pad=float('nan'))                  # NaN in the padding of every item
    bad[1] = float('nan')                                      # the longest item, whole
    bad[3] = float('inf')
    monkeypatch.setattr(vocoder, '_empty', _poison)            # every buffer of the batched path starts as NaN
    out = gl.griffinlim_batch(bad, ml, n_iter=2, seed=7)
    S = gl.mel_to_stft_batch(bad, ml)
    for b, N in enumerate(LENS):
        L = case.hop * (N - 1)
        assert not out['wav'][b, L:].any() and not clean['wav'][b, L:].any()              # exactly zero beyond wav_len
        rows = slice(b * case.Tcap, b * case.Tcap + N)
        assert not S[b * case.Tcap + N:(b + 1) * case.Tcap].any()                        # zero rows at n >= N_b
        if b not in (1, 3):
            assert torch.equal(out['wav'][b], clean['wav'][b]), b
            assert torch.equal(S[rows], clean_S[rows]), b
    # (what the NaN item itself becomes is not pinned: max(NaN, 0) of the NNLS clip is 0, as in the per-item path)


# ---- 5. 32 iterations ----------------------------------------------------------------------------------------------------
def test_32_iterations_converge_per_item_like_the_oracle(case):
    """as in tests/test_gpu_vocoder.py: after 32 iterations rounding differences have been amplified by c / |c| at
    near-silent bins, so the check is the algorithm's own figure of merit per item.  The one-frame item has an empty wav
    and with it no figure."""
    from oracle import gl_oracle as G
    from forwardtacotron_amd.vocoder import spectral_convergence
    gl = case.gl
    Sd, ud = case.rows(case.S), case.rows(case.u)
    w32 = gl.griffinlim_from_stft_batch(Sd, case.mel_len, case.Tmax, 32, init_u=ud)
    w0 = gl.griffinlim_from_stft_batch(Sd, case.mel_len, case.Tmax, 0, init_u=ud)
    for b, N in enumerate(LENS):
        if N == 1:
            assert _item(w32, b).numel() == 0
            continue
        Sb = Sd[b * case.Tcap:b * case.Tcap + N].contiguous()
        sc_got, sc0 = spectral_convergence(gl, _item(w32, b).contiguous(), Sb), spectral_convergence(gl, _item(w0, b).contiguous(), Sb)
        sc_want = G.spectral_convergence(G.griffinlim(case.S[b], 32, case.hop, case.win, case.u[b]), case.S[b], case.n_fft,
                                         case.hop, case.win)
        print(f'{case.name} item {b} (N {N}): spectral convergence {sc0:.4f} -> {sc_got:.4f} (oracle {sc_want:.4f})')
        assert sc_got < 0.5 * sc0 and abs(sc_got - sc_want) < 0.02, (b, N, sc0, sc_got, sc_want)


# ---- 6. device-drawn phases ----------------------------------------------------------------------------------------------
def test_device_drawn_phases_are_reproducible_seeded_and_uniform(case):
    from forwardtacotron_amd import hip as H
    gl, B = case.gl, len(LENS)
    mel, ml = case.mel_batch()
    a, b, c = (gl.griffinlim_batch(mel, ml, n_iter=1, seed=s)['wav'] for s in (5, 5, 6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    from forwardtacotron_amd.vocoder import gl_batch_geometry
    lens, Tm = [100, 128], 128                                                  # 228 frames: >= 30,000 draws in both settings
    Tcap = gl_batch_geometry(2, Tm, case.n_fft, case.hop)['Tcap']
    ones = torch.ones(2 * Tcap, case.Fp, device='cuda')
    mld = torch.tensor(lens, dtype=torch.int64).cuda()
    _, u = H.gl_init_ragged(ones, mld, 2, Tcap, Tm, seed=5, want_u=True)
    _, u2 = H.gl_init_ragged(ones, mld, 2, Tcap, Tm, seed=6, want_u=True)
    u = u.reshape(2, Tcap, case.Fp)
    valid = torch.cat([u[i, :N].reshape(-1) for i, N in enumerate(lens)])
    assert valid.numel() >= 30000
    mean = float(valid.double().mean())
    print(f'{case.name}: {valid.numel()} draws, min {float(valid.min()):.3e}, max {float(valid.max()):.8f}, mean {mean:.5f}')
    assert float(valid.min()) >= 0.0 and float(valid.max()) < 1.0 and abs(mean - 0.5) < 0.01
    assert not torch.equal(u.reshape(-1, case.Fp), u2)
    assert not u[0, 100:].any() and not u[1, 128:].any()                        # nothing drawn past an item
    assert torch.equal(u[0, :100], u[1, :100])                                  # keyed on (seed, n, m), not on the item


# ---- 7. argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors(project):
    from forwardtacotron_amd import hip as H
    from forwardtacotron_amd._lib import FtError
    case, gl = project, project.gl
    mel, ml = case.mel_batch()
    clean = gl.griffinlim_batch(mel, ml, n_iter=1, seed=3)
    torch.cuda.synchronize()
    for pos, v in ((2, 0), (0, case.Tmax + 1)):
        bad = ml.clone()
        bad[pos] = v
        before = H.gemm_variant_counts()
        with pytest.raises(FtError, match='mel_len'):
            gl.griffinlim_batch(mel, bad, n_iter=1, seed=3)
        assert H.gemm_variant_counts() == before                                # host lengths: refused before any launch
        with pytest.raises(FtError, match='mel_len'):                           # device lengths: clamped, raised at the end
            gl.griffinlim_batch(mel, bad.cuda(), n_iter=1, seed=3)
        torch.cuda.synchronize()
    again = gl.griffinlim_batch(mel, ml.cuda(), n_iter=1, seed=3)               # device lengths in range: the same bits
    assert torch.equal(again['wav'], clean['wav']) and torch.equal(again['wav_len'].cpu(), clean['wav_len'].cpu())
    with pytest.raises(FtError, match='mel channels'):
        gl.griffinlim_batch(mel[:, :40].contiguous(), ml)
    with pytest.raises(FtError, match='float32'):
        gl.griffinlim_batch(mel.double(), ml)
    with pytest.raises(FtError, match='int64'):
        gl.griffinlim_batch(mel, ml.int())
    with pytest.raises(FtError):
        gl.griffinlim_batch(mel, ml[:3])


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------
def test_text_to_wav_for_a_batch():
    from forwardtacotron_amd.audio import DSP, split_wavs
    from forwardtacotron_amd.model import ForwardTacotron
    from helpers import TINY
    dsp = DSP(**SETTINGS['project'])
    torch.manual_seed(0)
    m = ForwardTacotron(**dict(TINY, n_mels=80)).cuda()
    x_len = torch.tensor([12, 5, 9], dtype=torch.int64)
    gen = m.generate_batch(torch.randint(1, 100, (3, 12)).cuda(), x_len, alpha=1.0)
    mel = gen['mel_post'].clamp(-11.5, 2.0)                                 # an untrained model's "log-mel"
    out = dsp.griffinlim_batch(mel, gen['mel_len'], n_iter=4, seed=0)
    assert isinstance(out['wav'], torch.Tensor) and out['wav'].is_cuda
    wavs = split_wavs(out)
    mel_len = gen['mel_len'].tolist()
    assert [len(w) for w in wavs] == [256 * (n - 1) for n in mel_len]
    assert all(isinstance(w, np.ndarray) and np.isfinite(w).all() for w in wavs)
    out_np = dsp.griffinlim_batch(mel.cpu().numpy(), np.asarray(mel_len), n_iter=4, seed=0)     # numpy in -> numpy out
    assert isinstance(out_np['wav'], np.ndarray) and isinstance(out_np['wav_len'], np.ndarray)
    for w, v in zip(wavs, split_wavs(out_np)):
        assert np.array_equal(w, v)
