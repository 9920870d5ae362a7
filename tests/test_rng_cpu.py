"""The dropout generator as a generator: statistics and structure of tests/rng_ref.py, the numpy restatement of the
counter RNG in csrc/common.h that tests/test_rng_gpu.py holds every kernel against.  No GPU, fixed seeds: deterministic.

Every statistic is a z-score (normal approximation, n = 2^22 elements unless stated) and must stay within |z| <= 5.
The restatement's own figures, from this file's run (worst |z| per check):

    keep rate, overall and per sub-position 0..3, six (seed, site) pairs
        p = 0.05: 2.71   0.1: 3.17   0.2: 2.18   0.3: 2.15   0.5: 2.91   0.8: 2.87      (30 z-scores each)
    correlation inside a group of four (fields, keep decisions at p = 0.2 and 0.5)     2.57      (108)
    lag correlation, lags 1..8, 64, 128, 256 (fields and keep decisions at p = 0.3)    2.88      (132)
    correlation across site +-1, seed +-1, seed + 2^32, sites 64 / 65                  1.93      (66)
    correlation across consecutive seeds of the seed stream                            2.45      (24)
    per-column keep rate, width 128, 32768 rows                                        3.97      (768)

(the largest of 768 independent standard normal values exceeds 3.97 about once in 18 draws; each test prints its figure.)
Not asserted: the top byte of sub-position 1 is slightly uneven (chi-square 269-365 against 255 +- 23).
"""
import numpy as np
import pytest

import rng_ref as R

N = 1 << 22
Z_MAX = 5.0
# (seed, site) pairs every statistic runs over: small and large seeds, the sites the model draws
PAIRS = [(0, 0), (1, 1), (12345, 17), (2 ** 32 + 7, R.SITE_H1), (2 ** 63 + 5, R.SITE_H2), (2 ** 64 - 1, R.SITE_SUP)]
FIRSTS = [0, 0, 2 ** 32 - N // 2, 2 ** 34 - N // 2, 2 ** 50, 2 ** 62]       # first element of the window, per pair


def _note(name, z):
    z = float(np.max(np.abs(z)))
    print(f"{name}: worst |z| = {z:.2f}")
    return z


def _z_rate(kept, n, q):
    return (kept - n * q) / np.sqrt(n * q * (1.0 - q))


def _z_corr(a, b):
    """z-score of the Pearson correlation of two equally long samples under independence: r * sqrt(n)."""
    n = a.size
    if a.dtype == np.bool_:
        sa, sb, sab = int(np.count_nonzero(a)), int(np.count_nonzero(b)), int(np.count_nonzero(a & b))
        saa, sbb = sa, sb
    else:                                   # 16-bit values: every sum is exact in int64
        a, b = a.astype(np.int64), b.astype(np.int64)
        sa, sb, sab, saa, sbb = int(a.sum()), int(b.sum()), int(np.dot(a, b)), int(np.dot(a, a)), int(np.dot(b, b))
    cov, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    return cov / (float(va) ** 0.5 * float(vb) ** 0.5) * n ** 0.5


@pytest.fixture(scope="module")
def streams():
    """The 16-bit fields of N consecutive elements per (seed, site) pair, computed once."""
    return [R.fields(s, site, first, N) for (s, site), first in zip(PAIRS, FIRSTS)]


@pytest.mark.parametrize("p", [0.05, 0.1, 0.2, 0.3, 0.5, 0.8])
def test_keep_rate_is_the_quantised_probability(streams, p):
    """Overall and per sub-position 0..3 of a group of four, against 1 - thr / 65536 (not 1 - p)."""
    thr = R.threshold(p)
    q = 1.0 - thr / 65536.0
    assert abs(q - (1.0 - p)) <= 1.0 / 65536.0
    zs = []
    for (s, site), first, f in zip(PAIRS, FIRSTS, streams):
        k = f >= thr
        assert np.array_equal(k[:4099], R.keep(s, site, first, 4099, p))
        zs.append(_z_rate(int(k.sum()), N, q))
        assert first % 4 == 0
        for sub in range(4):
            zs.append(_z_rate(int(k[sub::4].sum()), N // 4, q))
    assert _note(f"keep rate, overall and per sub-position, p={p}", zs) <= Z_MAX


def test_the_four_fields_of_a_group_are_uncorrelated(streams):
    zs = []
    for f in streams:
        g = f.reshape(-1, 4)
        for i in range(4):
            for j in range(i + 1, 4):
                zs.append(_z_corr(g[:, i], g[:, j]))                                          # the 16-bit values
                for p in (0.2, 0.5):
                    zs.append(_z_corr(g[:, i] >= R.threshold(p), g[:, j] >= R.threshold(p)))   # the keep decisions
    assert _note("correlation inside a group of four", zs) <= Z_MAX


def test_lagged_elements_are_uncorrelated(streams):
    zs = []
    for f in streams:
        k = f >= R.threshold(0.3)
        for lag in (1, 2, 3, 4, 5, 6, 7, 8, 64, 128, 256):
            zs.append(_z_corr(k[:-lag], k[lag:]))
            zs.append(_z_corr(f[:-lag], f[lag:]))
    assert _note("lag correlation, lags 1..8, 64, 128, 256", zs) <= Z_MAX


def test_neighbouring_sites_and_seeds_are_uncorrelated(streams):
    """site +-1, seed +-1, seed + 2^32 (the high word of the seed), and the two head sites of one seed."""
    zs = []
    for (s, site), first, f in zip(PAIRS, FIRSTS, streams):
        for s2, site2 in ((s, site + 1), (s, site - 1), (s + 1, site), (s - 1, site), (s + 2 ** 32, site)):
            f2 = R.fields(s2 % 2 ** 64, site2 % 2 ** 32, first, N)
            zs.append(_z_corr(f, f2))
            zs.append(_z_corr(f >= R.threshold(0.3), f2 >= R.threshold(0.3)))
    for s in (0, 77, 2 ** 63 + 5):
        a, b = R.fields(s, R.SITE_H1, 0, N), R.fields(s, R.SITE_H2, 0, N)
        zs.append(_z_corr(a, b))
        zs.append(_z_corr(a >= R.threshold(0.2), b >= R.threshold(0.2)))
    assert _note("correlation across site +-1, seed +-1, seed + 2^32, sites 64 / 65", zs) <= Z_MAX


def test_consecutive_seeds_of_the_seed_stream_are_uncorrelated():
    zs = []
    for state in ((0, 0), (0, 2 ** 64 - 0x9E3779B97F4A7C15 + 3), (0, 123456789)):
        prev = None
        for _ in range(5):
            state = R.splitmix(state)
            assert 0 <= state[0] < 2 ** 62
            f = R.fields(state[0], 3, 0, N)
            if prev is not None:
                zs.append(_z_corr(prev, f))
                zs.append(_z_corr(prev >= R.threshold(0.2), f >= R.threshold(0.2)))
            prev = f
    assert _note("correlation across consecutive seeds of the seed stream", zs) <= Z_MAX


def test_keep_rate_per_column(streams):
    """Width 128, 32768 rows: no column of an activation is dropped more often than another."""
    q = 1.0 - R.threshold(0.3) / 65536.0
    zs = []
    for f in streams:
        k = (f >= R.threshold(0.3)).reshape(-1, 128)
        zs.extend(_z_rate(k.sum(0), k.shape[0], q))
    assert _note("per-column keep rate, width 128, 32768 rows", zs) <= Z_MAX


# ---------------------------------------------------------------------------------------------- structure
def test_every_site_of_a_step_has_its_own_key():
    sites = [2 * call + j for call in (0, 1) for j in (0, 1)]
    sites += [R.SITE_CONV + 8 * l + ti for l in range(6) for ti in range(8)]
    sites += [R.SITE_H1, R.SITE_H2, R.SITE_SUP]
    assert len(set(sites)) == len(sites)
    for seed in (0, 1, 99, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1):
        keys = [R.key(seed, s) for s in sites]
        assert len(set(keys)) == len(keys), seed


def test_p_zero_keeps_everything_and_p_one_nothing():
    for (s, site), first in zip(PAIRS, FIRSTS):
        assert R.keep(s, site, first, 1 << 16, 0.0).all()
        assert not R.keep(s, site, first, 1 << 16, 1.0).any()
    assert R.threshold(0.0) == 0 and R.threshold(1.0) == 65536 and R.threshold(1e-6) == 0 and R.threshold(0.99999) == 65535
    assert R.threshold(0.3) == 19660 and R.threshold(0.5) == 32768


def test_a_field_depends_only_on_key_group_and_sub_position():
    n = 4099
    for (s, site), first in zip(PAIRS, FIRSTS):
        base = R.fields(s, site, first, n)
        # the window does not matter: a start that is no multiple of 4, one element at a time, a permuted order
        assert np.array_equal(R.fields(s, site, first + 3, n - 3), base[3:])
        for e in (0, 1, 2, 3, 4, 4098):
            assert int(R.fields(s, site, first + e, 1)[0]) == int(base[e])
        perm = np.random.default_rng(5).permutation(n)
        assert np.array_equal(R.fields_at(R.key(s, site), np.uint64(first) + perm.astype(np.uint64)), base[perm])
        # (key, group) -> two words, sub-position -> one half of one word
        w0, w1 = R.group_words(R.key(s, site), (np.uint64(first) + np.arange(n, dtype=np.uint64)) >> np.uint64(2))
        halves = np.stack([w0 & 0xFFFF, w0 >> 16, w1 & 0xFFFF, w1 >> 16], 1)
        assert np.array_equal(halves[np.arange(n), (first + np.arange(n)) % 4], base)
        # another (seed, site) with the SAME key draws the same fields: the high word of the seed and the site enter
        # the key through one XOR, so a change of one is undone by a change of the other
        d = 0x5A5A1234
        site2 = (((site * 0x632BE5AB) & R.M32) ^ d) * pow(0x632BE5AB, -1, 2 ** 32) & R.M32
        seed2 = s ^ (d << 32)
        assert (seed2, site2) != (s, site) and R.key(seed2, site2) == R.key(s, site)
        assert np.array_equal(R.fields(seed2, site2, first, n), base)
    # two sites of one seed: the same sequence of groups under an XOR of the group index's low word with key ^ key'
    ka, kb = R.key(7, 16), R.key(7, 17)
    g = np.arange(1 << 12, dtype=np.uint64)
    wa = R.group_words(ka, g)
    wb = R.group_words(kb, g ^ np.uint64(ka ^ kb))
    assert np.array_equal(wa[0], wb[0]) and np.array_equal(wa[1], wb[1])


def test_mask2d_is_the_row_major_stream():
    m = R.mask2d(9, 3, 7, 64, 0.3, row_offset=2 ** 27 - 5)
    assert m.shape == (7, 64) and m.dtype == np.bool_
    assert np.array_equal(m.ravel(), R.keep(9, 3, (2 ** 27 - 5) * 64, 7 * 64, 0.3))
    assert np.array_equal(m[3], R.keep(9, 3, (2 ** 27 - 2) * 64, 64, 0.3))


def test_splitmix_restates_splitmix64():
    # the first outputs of SplitMix64 from state 0 (Vigna's reference implementation), >> 2 as the kernels publish them
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    state = (0, 0)
    for w in want:
        state = R.splitmix(state)
        assert state[0] == w >> 2
    assert state[1] == (3 * 0x9E3779B97F4A7C15) % 2 ** 64
    wrap = R.splitmix((5, 2 ** 64 - 1))
    assert wrap[1] == 0x9E3779B97F4A7C14 and 0 <= wrap[0] < 2 ** 62


# ---------------------------------------------------------------------------------------------- site allocation
CFG = {"model": {"architecture": "RGCN", "hidden_dim": 64, "num_layers": 2, "dropout": 0.2, "use_batch_norm": True,
                 "activation": "relu"}}


def test_conv_sites_cannot_reach_the_head_sites():
    """SITE_CONV + 8 * l + ti reaches 64 (the heads' first site) at layer index 6, and a ninth node type would draw the
    next layer's site: the model refuses both."""
    import mmgnn  # noqa: F401
    from mmgnn import model as mm
    from oracle import fixtures as fx
    assert mm.SITE_CONV == R.SITE_CONV and mm.SITE_H1 == R.SITE_H1
    meta = (fx.NODE_TYPES, fx.EDGE_TYPES)
    m = mm.build_model({"model": dict(CFG["model"], num_layers=6)}, meta, None)
    top = mm.SITE_CONV + 8 * (m.num_layers - 1) + len(fx.NODE_TYPES) - 1
    assert top < R.SITE_H1
    with pytest.raises(ValueError, match="dropout sites"):
        mm.build_model({"model": dict(CFG["model"], num_layers=7)}, meta, None)
    many = list(fx.NODE_TYPES) + [f"extra{i}" for i in range(9 - len(fx.NODE_TYPES))]
    with pytest.raises(ValueError, match="dropout sites"):
        mm.build_model(CFG, (many, fx.EDGE_TYPES), None)
    with pytest.raises(ValueError, match="dropout sites"):
        mm.check_dropout_sites(2, 9)
    mm.check_dropout_sites(6, 8)
