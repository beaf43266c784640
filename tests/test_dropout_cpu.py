"""Statistics and exact rules of the dropout mask, on the numpy restatement alone (dropout_cpu; test_gpu_dropout.py ties it
bit for bit to ft_dropout and to every kernel that fuses the mask).  Seeds and sizes are fixed, so every figure below is a
fact about the mixer, not a probability, and nothing here can flake.  No GPU needed.

All z values are in binomial sigmas: a rate against the exact drop probability ceil(float32(p) * 2^24) / 2^24, a pair
statistic as sum (a_i - q)(b_i - q) / (sqrt(N) q (1 - q)) with q the exact keep probability (its terms are uncorrelated
under independence, so the denominator is exact).  The bars are |z| <= 5.

Observed (recomputed by these tests; run with -s to print them):
  keep rate, 12 seeds x 3 p, n = 2^22                                   max |z| 2.11
  lags {1, 2, 64, 70, 128, 256, 841}                                    max |z| 2.91
  residue classes (841: 0, 1, 7; 4096: 0, 5; all of 64 and of 256)      max |z| 3.82
  64 consecutive stream seeds, 2016 pairs, n = 2^18, p = 0.1 / 0.5      max pair |z| 3.29 / 3.24, max rate |z| 3.14 / 3.13
  index bit flips 0..39, 6 seeds x 3 p, n = 2^20                        max |z| 3.09
  index offset 2^32 against offset 0                                    rate max |z| 2.48, pair max |z| 2.05

The seed limits (documented facts, see test_equal_high_words_give_an_xor_permuted_mask): two seeds with the same high word
give one mask permuted by an XOR of the index, and the top bits of the high word meet only the last mixing round, so
flipping one of seed bits 54..63 leaves the masks correlated: at p = 0.5, n = 2^20, first stream seed of torch seed 0,
  bit 50..53: |z| <= 4;  54: -13, 55: +11, 56: +8, 57: -13, 58: +86, 59: +6, 60: +35, 61: +84, 62: 0, 63: +309
  (z = 309 at n = 2^20 is a correlation coefficient of 0.30).
Callers must not rely on such seeds; base._seed() and tacotron.dropout_seed() do not produce them (the last test).
"""
import numpy as np
import pytest
import torch

import dropout_cpu as D

PS = (0.1, 0.5, 0.9)
N = 1 << 22
SEEDS = D.seed_stream(0, 8) + [0, 1, 1 << 32, (1 << 62) - 1]
LAGS = (1, 2, 64, 70, 128, 256, 841)
# the residue classes round 3 printed (stride 841, T of the benchmark: 0, 1, 7; stride 4096: 0, 5) plus every class of strides 64 and 256
CLASSES = [(841, r) for r in (0, 1, 7)] + [(4096, r) for r in (0, 5)] + [(64, r) for r in range(64)] + \
          [(256, r) for r in range(256)]


def _q(p):
    return 1.0 - D.drop_probability(p)


def _rate_z(k, p):
    q = _q(p)
    return (float(k.sum()) - k.size * q) / np.sqrt(k.size * q * (1 - q))


def _pair_z(a, b, p):
    q = _q(p)
    if a.size == 0:
        return 0.0
    return float(np.dot(a.astype(np.float64) - q, b.astype(np.float64) - q)) / (np.sqrt(a.size) * q * (1 - q))


@pytest.fixture(scope='module')
def u_of_seed():
    """u24 over [0, 2^22) of every seed, computed once (every p thresholds the same u)"""
    return {s: D.u24(s, np.arange(N, dtype=np.uint64)) for s in SEEDS}


def test_restatement_known_values():
    """hand-checked anchors: the all-zero input, and the formula written out once in Python ints"""
    def scalar(seed, i):
        m = 0xFFFFFFFF
        h = (i & m) ^ (((i >> 32) * 0x9E3779B1) & m)
        h = ((h ^ (seed & m)) * 0x85EBCA6B) & m
        h ^= h >> 15
        h = ((h + (seed >> 32)) * 0xC2B2AE35) & m
        h ^= h >> 13
        h = (h * 0x27D4EB2F) & m
        return h ^ (h >> 16)
    assert int(D.hash32(0, 0)) == 0
    for seed in (0, 1, 0x123456789ABCDEF, (1 << 64) - 1):
        idx = [0, 1, 255, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345]
        got = D.hash32(seed, np.array(idx, dtype=np.uint64))
        assert [int(g) for g in got] == [scalar(seed, i) for i in idx]
    assert D.hash32(-1, 5) == D.hash32((1 << 64) - 1, 5)                  # the wrapper's masking of a Python int
    assert D.drop_probability(0.5) == 0.5 and D.drop_probability(0.0) == 0.0
    assert D.drop_probability(0.1) == 1677722 / 2 ** 24                   # float32(0.1) * 2^24 = 1677721.625


def test_keep_rate(u_of_seed):
    worst = 0.0
    for s, u in u_of_seed.items():
        for p in PS:
            z = _rate_z(u >= np.float32(p), p)
            worst = max(worst, abs(z))
            assert abs(z) <= 5, (hex(s), p, z)
    print(f'keep rate: max |z| {worst:.2f}')


def test_lags_and_residue_classes(u_of_seed):
    worst_lag = worst_cls = 0.0
    for s, u in u_of_seed.items():
        for p in PS:
            k = u >= np.float32(p)
            for lag in LAGS:
                z = _pair_z(k[:-lag], k[lag:], p)
                worst_lag = max(worst_lag, abs(z))
                assert abs(z) <= 5, (hex(s), p, 'lag', lag, z)
            q = _q(p)
            for stride, r in CLASSES:
                if r == 0 and stride in (64, 256):                       # N is a multiple: all classes of the stride at once
                    cnt = k.reshape(-1, stride).sum(axis=0)
                    zs = (cnt - (N // stride) * q) / np.sqrt((N // stride) * q * (1 - q))
                z = float(zs[r]) if stride in (64, 256) else _rate_z(k[r::stride], p)
                worst_cls = max(worst_cls, abs(z))
                assert abs(z) <= 5, (hex(s), p, 'class', stride, r, z)
    print(f'lags: max |z| {worst_lag:.2f}; residue classes: max |z| {worst_cls:.2f}')


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_the_sites_of_a_step_are_independent(p):
    """a training step draws ~170 consecutive stream seeds: 64 of them, all 2016 pairs at the same index, n = 2^18"""
    n = 1 << 18
    q = _q(p)
    seeds = D.seed_stream(0, 64)
    C = np.stack([D.keep(s, n, p).astype(np.float64) - q for s in seeds])
    rate_z = C.sum(axis=1) / np.sqrt(n * q * (1 - q))
    G = (C @ C.T) / (np.sqrt(n) * q * (1 - q))
    pair_z = np.abs(G[np.triu_indices(64, 1)])
    assert pair_z.size == 2016
    print(f'p {p}: 64 stream seeds: max pair |z| {pair_z.max():.2f}, max rate |z| {np.abs(rate_z).max():.2f}')
    assert np.abs(rate_z).max() <= 5
    assert pair_z.max() <= 5


@pytest.mark.parametrize('seed', D.seed_stream(0, 2) + [0, 1, 1 << 32, (1 << 62) - 1])
def test_index_avalanche(seed):
    """flipping one index bit, 0..39, gives an uncorrelated decision (each unordered pair counted once)"""
    n = 1 << 20
    i = np.arange(n, dtype=np.uint64)
    u0 = D.u24(seed, i)
    worst = 0.0
    for bit in range(40):
        if bit < 20:
            j = i[(i >> np.uint64(bit)) & np.uint64(1) == 0]
            a, b = u0[j.astype(np.int64)], u0[(j | np.uint64(1 << bit)).astype(np.int64)]
        else:
            a, b = u0, D.u24(seed, i | np.uint64(1 << bit))
        for p in PS:
            z = _pair_z(a >= np.float32(p), b >= np.float32(p), p)
            worst = max(worst, abs(z))
            assert abs(z) <= 5, (hex(seed), bit, p, z)
    print(f'seed {seed:#x}: index avalanche max |z| {worst:.2f}')


def test_high_word_of_the_index(u_of_seed):
    worst_r = worst_c = 0.0
    for s, u in u_of_seed.items():
        uh = D.u24(s, np.arange(N, dtype=np.uint64) + np.uint64(1 << 32))
        for p in PS:
            a, b = u >= np.float32(p), uh >= np.float32(p)
            zr, zc = _rate_z(b, p), _pair_z(a, b, p)
            worst_r, worst_c = max(worst_r, abs(zr)), max(worst_c, abs(zc))
            assert abs(zr) <= 5 and abs(zc) <= 5, (hex(s), p, zr, zc)
    print(f'index offset 2^32: max rate |z| {worst_r:.2f}, max |z| against the low range {worst_c:.2f}')


def test_the_exact_rule(u_of_seed):
    """u >= float32(p) on a 24-bit u.  p = 0 drops nothing; p = 2^-24 drops exactly h >> 8 == 0.  The largest float32
    below 1 is 1 - 2^-24, which IS the largest u: at that p exactly the elements with h >> 8 == 0xFFFFFF survive (kept
    value x * 2^24), one in 2^24 -- the drop probability ceil(p * 2^24) / 2^24 = 1 - 2^-24 says the same.  Over the 2^22
    indices of these twelve seeds none does."""
    top = np.float32(np.nextafter(np.float32(1), np.float32(0)))
    assert float(top) == 1 - 2.0 ** -24 and D.drop_probability(top) == 1 - 2.0 ** -24
    survivors = 0
    for s, u in u_of_seed.items():
        h24 = D.hash32(s, np.arange(N, dtype=np.uint64)) >> np.uint32(8)
        assert (u >= np.float32(0.0)).all()
        assert np.array_equal(~(u >= np.float32(2.0 ** -24)), h24 == 0)
        assert np.array_equal(u >= top, h24 == 0xFFFFFF)
        survivors += int((u >= top).sum())
    assert survivors == 0
    # the rule is the same through keep() and site_mask()
    s = SEEDS[0]
    assert np.array_equal(D.keep(s, 1000, 0.5), u_of_seed[s][:1000] >= np.float32(0.5))
    m = D.site_mask(s, (10, 100), 0.5, np.float32)
    assert np.array_equal(m, np.where(D.keep(s, 1000, 0.5), np.float32(2), np.float32(0)).reshape(10, 100))
    assert np.array_equal(D.site_mask(s, (3, 4), 0.0), np.ones((3, 4)))


def test_equal_high_words_give_an_xor_permuted_mask():
    """A LIMIT of the mixer, stated so that it is known, not a requirement: the low seed word is XORed onto the index
    before the first multiply, so mask(s_b, i) == mask(s_a, i ^ lo(s_a) ^ lo(s_b)) whenever the high words agree --
    seeds 1, 2, 3, ... are shuffles of one mask.  Callers must not rely on such seeds for independent sites; seeds of
    different sites must differ in the high word, and not only in its top ten bits (module docstring)."""
    i = np.arange(1 << 16, dtype=np.uint64) + np.uint64((1 << 32) - 1000)        # straddles the index's high word too
    for sa, sb in ((1, 2), (0, 0xFFFFFFFF), ((0x1234567 << 32) | 77, (0x1234567 << 32) | 0xDEADBEEF)):
        x = np.uint64((sa ^ sb) & 0xFFFFFFFF)
        assert np.array_equal(D.hash32(sb, i), D.hash32(sa, i ^ x))
        for p in PS:
            assert np.array_equal(D.keep_at(sb, i, p), D.keep_at(sa, i ^ x, p))


def test_high_seed_bits_record():
    """prints the correlations quoted in the module docstring (python -m pytest -s); asserts nothing about them"""
    n, p = 1 << 20, 0.5
    s = D.seed_stream(0, 1)[0]
    a = D.keep(s, n, p)
    print('seed bit: z  ' + ', '.join(f'{b}: {_pair_z(a, D.keep(s ^ (1 << b), n, p), p):+.0f}' for b in range(50, 64)))


def test_the_product_seeds_are_spread_over_both_words():
    """what training relies on: base._seed() and tacotron.dropout_seed() stay below 2^62 and no two of 64 draws share a
    high word"""
    from forwardtacotron_amd import base, tacotron
    state = torch.get_rng_state()
    try:
        torch.manual_seed(4242)
        base._seed_state['torch_seed'] = None
        a = [base._seed() for _ in range(64)]
        assert a == D.seed_stream(4242, 64)                              # and the restated stream is the product's
        torch.manual_seed(4242)
        b = [tacotron.dropout_seed() for _ in range(64)]
    finally:
        torch.set_rng_state(state)
        base._seed_state['torch_seed'] = None                            # re-base on the next draw, whoever makes it
    for seeds in (a, b):
        assert all(0 <= s < 1 << 62 for s in seeds)
        assert len({s >> 32 for s in seeds}) == 64
