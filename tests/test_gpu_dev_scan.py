"""dev_scan.hip's carry in two levels, alone (dhts_debug_carry: the launcher the count functions call), against numpy at the sizes where it
takes another path: inside one thread's elements, around a chunk, a partial last chunk, and the last size of one turn / the first of two
turns of the single-workgroup pass, which no count function reaches.  Every comparison is exact."""
import numpy as np
import pytest

import duckhts_amd

pytestmark = pytest.mark.gpu

CHUNK = 4096                      # 256 threads x 16 elements
SIZES = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, CHUNK * 255 + 5, CHUNK * CHUNK, CHUNK * CHUNK + 1]
COV_CHUNK = 1024                  # 256 threads x 4 elements of four words
COV_SIZES = [1, 3, 4, 5, COV_CHUNK - 1, COV_CHUNK, COV_CHUNK + 1, COV_CHUNK * COV_CHUNK, COV_CHUNK * COV_CHUNK + 1]
FULL = np.uint64(0xffffffffffffffff)


@pytest.fixture(scope="module")
def ctx():
    c = duckhts_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool():
    """random words the cases cut their inputs from (made once, never written to)"""
    rng = np.random.default_rng(20261020)
    w = rng.integers(0, 1 << 64, size=CHUNK * CHUNK + 1, dtype=np.uint64)
    w.setflags(write=False)
    return w


def exclusive(v):
    """[0, v0, v0 + v1, ...] in v's own width (numpy's cumsum wraps as the device does), the total last"""
    out = np.zeros((v.shape[0] + 1,) + v.shape[1:], v.dtype)
    np.cumsum(v, axis=0, dtype=v.dtype, out=out[1:])
    return out


def suffix_min(v, seed):
    """out[i] = min(v[i + 1:]), seed where nothing lies behind i"""
    out = np.empty_like(v)
    out[-1] = seed
    if v.shape[0] > 1:
        out[:-1] = np.minimum(np.minimum.accumulate(v[:0:-1])[::-1], np.uint64(seed))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sum_u32(ctx, pool, n):
    """32-bit sums wrap (bam_coverage.hip's contract): runs of values near 2^32 among random ones, so the running sum wraps many times"""
    v = (pool[:n] >> np.uint64(32)).astype(np.uint32)
    v[n // 3: n // 3 + max(1, n // 5)] |= np.uint32(0xfffffff0)
    got = ctx.debug_carry(0, v)
    assert got.dtype == np.uint32 and got.shape == (n + 1,) and np.array_equal(got, exclusive(v))


@pytest.mark.parametrize("n", SIZES)
def test_sum_u64(ctx, pool, n):
    v = pool[:n] >> np.uint64(24)                 # below 2^40
    got = ctx.debug_carry(1, v)
    assert got.shape == (n + 1,) and np.array_equal(got, exclusive(v))


@pytest.mark.parametrize("n", SIZES)
def test_suffix_min_u64(ctx, pool, n):
    """the reverse form with min: random words, all ~0, strictly increasing (every answer is the next element) and strictly decreasing (every
    answer is the last element); seeded with ~0 and with a word below every element"""
    idx = np.arange(n, dtype=np.uint64)
    inputs = {"random": (pool[:n] >> np.uint64(1)) + np.uint64(1000), "full": np.full(n, FULL), "increasing": idx * np.uint64(3) + np.uint64(1000),
              "decreasing": np.uint64(3 * n + 1000) - idx * np.uint64(3)}
    for name, v in inputs.items():
        for seed in (int(FULL), 7):
            got = ctx.debug_carry(2, v, seed)
            assert got.shape == (n,) and np.array_equal(got, suffix_min(v, seed)), (name, seed)
            if seed == int(FULL) and name == "increasing":
                assert np.array_equal(got[:-1], v[1:]) and got[-1] == FULL
            if seed == int(FULL) and name == "decreasing":
                assert (got[:-1] == v[-1]).all() and got[-1] == FULL


@pytest.mark.parametrize("n", COV_SIZES)
def test_sum_four_words(ctx, pool, n):
    """four independent random columns, added word by word: none leaks into another"""
    v = pool[:4 * n].reshape(n, 4)
    got = ctx.debug_carry(3, v)
    assert got.shape == (n + 1, 4) and np.array_equal(got, exclusive(v))
    one = np.zeros((n, 4), np.uint64)
    one[:, 2] = v[:, 2]
    got = ctx.debug_carry(3, one)
    assert not got[:, [0, 1, 3]].any() and np.array_equal(got[:, 2], exclusive(v[:, 2].copy()))
