"""The interval functions' radix sort on the device (csrc/interval_sort.hip through dhts_debug_ivl_sort) against numpy's stable lexsort, exactly:
every size around the tile and the carry's chunk, random 64-bit keys, keys whose passes are all or mostly skipped, a pass with every digit value,
many equal keys (stability) and enough ranks for two rank passes."""
import numpy as np
import pytest

import duckhts_amd
import interval_ref as R

pytestmark = pytest.mark.gpu
T = duckhts_amd.IVL_SORT_TILE
SIZES = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 17 * T + 1)     # 17 T + 1: 18 tiles x 256 digits of counts are more than one 4,096-element chunk of the carry


@pytest.fixture(scope="module")
def ctx():
    c = duckhts_amd.Context(0)
    yield c
    c.close()


def check(ctx, keys, rank):
    got, passes = ctx.debug_ivl_sort(keys, rank)
    exp = R.sort_rows(keys, rank)
    assert got.dtype == np.uint32 and len(got) == len(exp)
    bad = np.flatnonzero(got != exp)
    assert not len(bad), (len(keys), bad[:5].tolist(), got[bad[:5]].tolist(), exp[bad[:5]].tolist())
    return passes


def test_the_tile_is_what_the_mirror_says():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "duckhts_amd", "csrc", "interval_sort.hip")).read()
    assert "#define IVL_SORT_NT 256u" in src and "#define IVL_SORT_PER 16u" in src and "#define IVL_SORT_TILE (IVL_SORT_NT * IVL_SORT_PER)" in src and T == 256 * 16


@pytest.mark.parametrize("n", SIZES)
def test_random_keys_and_ranks(ctx, n):
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    passes = check(ctx, keys, np.zeros(n, np.uint32))
    assert passes <= 8 and (passes == 8 or n < T - 1) and (passes == 0) == (n < 2)
    passes = check(ctx, keys, rng.integers(0, 5, n, dtype=np.uint32))
    assert passes <= 9 and (passes == 9 or n < T - 1)


@pytest.mark.parametrize("n", SIZES)
def test_equal_keys_skip_every_pass(ctx, n):
    assert check(ctx, np.full(n, 0x0123456789abcdef, np.uint64), np.full(n, 7, np.uint32)) == 0


@pytest.mark.parametrize("n", SIZES)
def test_keys_that_differ_in_the_top_byte_only(ctx, n):
    rng = np.random.default_rng(1000 + n)
    top = rng.integers(0, 256, n, dtype=np.uint64)
    if n >= 2:
        top[0], top[1] = 0x7f, 0x80                                              # both sides of the sign
    passes = check(ctx, (top << np.uint64(56)) | np.uint64(0x00aabbccddeeff11), np.zeros(n, np.uint32))
    assert passes == (1 if n >= 2 else 0)


@pytest.mark.parametrize("n", SIZES)
def test_positions_below_2_32_on_one_chrom(ctx, n):
    rng = np.random.default_rng(2000 + n)
    keys = R.sort_key(rng.integers(0, 1 << 32, n, dtype=np.int64))
    assert check(ctx, keys, np.zeros(n, np.uint32)) <= 4


@pytest.mark.parametrize("n", (T - 1, T + 1, 3 * T + 5, 17 * T + 1))
def test_a_pass_with_all_256_digit_values(ctx, n):
    rng = np.random.default_rng(3000 + n)
    d = rng.permutation(np.arange(n, dtype=np.uint64) % np.uint64(256))
    assert len(np.unique(d)) == 256
    assert check(ctx, d << np.uint64(16), np.zeros(n, np.uint32)) == 1
    assert check(ctx, np.zeros(n, np.uint64), d.astype(np.uint32)) == 1                 # the same through the rank


@pytest.mark.parametrize("n", SIZES)
def test_many_equal_keys_stay_in_input_order(ctx, n):
    rng = np.random.default_rng(4000 + n)
    keys = rng.integers(0, 3, n, dtype=np.uint64) * np.uint64(0x0101010101010101)
    got, _ = ctx.debug_ivl_sort(keys, np.zeros(n, np.uint32))
    assert (got == R.sort_rows(keys, np.zeros(n, np.uint32))).all()
    for v in np.unique(keys):
        rows = got[keys[got] == v].astype(np.int64)
        assert (np.diff(rows) > 0).all()


def test_300_ranks_need_two_rank_passes(ctx):
    rank = np.random.default_rng(5).permutation(300).astype(np.uint32)
    assert check(ctx, np.full(300, 1 << 63, np.uint64), rank) == 2
    rng = np.random.default_rng(6)
    n = 3 * T + 5
    passes = check(ctx, R.sort_key(rng.integers(-1000, 1000, n, dtype=np.int64)), rng.integers(0, 300, n, dtype=np.uint32))
    assert passes == 10                                                          # a negative start turns every byte of the key: 8 passes, and 2 of the rank
