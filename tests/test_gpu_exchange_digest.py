"""GPU: the digest kernel of the verified exchange (digest_kernels.hip, mmt_exchange_digest) against a numpy restatement of
its definition, computed in uint64 with wrap-around.

Per piece of `piece_elements` elements, for element i (0-based inside the piece) with value v zero-extended to 64 bits:
    x = v + (i + 1) * 0x9E3779B97F4A7C15;  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;
    x ^= x >> 31;  sum += x;  xor ^= x
The words are integers: the comparison is exact.  Shapes: counts around the 16-byte vector (15, 16, 17), around a wave's 64 lanes
and its step of 256 vectors, 4097, and 2^22 + 3 (more steps than the grid has workgroups: the grid stride); bases 0, 1 and 3
elements into the allocation (not 16-byte aligned: scalar head and tail); pieces of 997 elements (boundaries inside a vector load,
more pieces than a small grid has workgroups) and one piece for everything."""
import numpy as np
import pytest

import mumemto_amd

pytestmark = pytest.mark.gpu

GOLD, MUL1, MUL2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
DTYPES = {1: np.uint8, 4: np.uint32, 8: np.int64}
COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 4097, 2 ** 22 + 3]


def ref_digest(values, piece):
    v = np.ascontiguousarray(values)
    v = v.view(np.uint64) if v.dtype.itemsize == 8 else v.astype(np.uint64)     # int64: its bit pattern
    n = len(v)
    out = np.zeros((max(1, -(-n // piece)), 2), np.uint64)
    with np.errstate(over="ignore"):
        for p in range(out.shape[0] if n else 0):
            seg = v[p * piece:(p + 1) * piece]
            x = seg + np.arange(1, len(seg) + 1, dtype=np.uint64) * GOLD
            x ^= x >> np.uint64(30); x *= MUL1
            x ^= x >> np.uint64(27); x *= MUL2
            x ^= x >> np.uint64(31)
            out[p, 0] = np.add.reduce(x, dtype=np.uint64)
            out[p, 1] = np.bitwise_xor.reduce(x)
    return out


def random_values(width, n, seed):
    rng = np.random.default_rng(seed)
    if width == 1:
        return rng.integers(0, 256, n, dtype=np.uint8)
    if width == 4:
        return rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    return rng.integers(-2 ** 63, 2 ** 63, n, dtype=np.int64)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("width", [1, 4, 8])
def test_digest_equals_the_definition(width, count):
    for skip in (0, 1, 3):
        a = random_values(width, count + skip, 1000 * width + skip)
        for piece in (997, count + 5):
            got = mumemto_amd.exchange_digest(a, piece, skip_elements=skip)
            want = ref_digest(a[skip:], piece)
            assert got.shape == want.shape, (width, count, skip, piece)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, "width %d, %d elements, skip %d, pieces of %d: piece %d of %d: got %s, want %s" % (
                width, count, skip, piece, bad[0], len(want), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("width", [1, 4])
def test_grid_stride_of_the_narrow_elements(width):
    """The grid is capped at 4096 workgroups of 4 KiB a step: 2^22 + 3 elements are more than one pass for 8-byte elements only;
    2^25 + 5 are for 1- and 4-byte ones (2 and 8 passes), with piece boundaries that are no multiple of anything."""
    a = random_values(width, 2 ** 25 + 5 + 3, 5 + width)
    for skip, piece in ((3, 2 ** 20 + 7), (0, 2 ** 25 + 10)):
        got = mumemto_amd.exchange_digest(a, piece, skip_elements=skip)
        assert np.array_equal(got, ref_digest(a[skip:], piece)), (width, skip, piece)


@pytest.mark.parametrize("width", [1, 4, 8])
def test_zeros_have_digests_that_tell_lengths_apart(width):
    seen = set()
    for n in (1, 2, 16, 17, 4097):
        got = mumemto_amd.exchange_digest(np.zeros(n, DTYPES[width]), n)
        assert np.array_equal(got, ref_digest(np.zeros(n, DTYPES[width]), n))
        assert got[0, 0] != 0 and got[0, 1] != 0
        seen.add((int(got[0, 0]), int(got[0, 1])))
    assert len(seen) == 5


@pytest.mark.parametrize("width", [1, 4, 8])
def test_swapping_two_elements_changes_the_digest(width):
    a = random_values(width, 5000, 7)
    b = a.copy()
    i, j = 1234, 1240                       # inside one piece of 997 (piece 1: elements 997 .. 1993)
    assert a[i] != a[j]
    b[i], b[j] = a[j], a[i]
    da, db = mumemto_amd.exchange_digest(a, 997), mumemto_amd.exchange_digest(b, 997)
    assert np.array_equal(db, ref_digest(b, 997))
    differ = np.flatnonzero((da != db).any(axis=1))
    assert list(differ) == [1] and da[1, 0] != db[1, 0] and da[1, 1] != db[1, 1]
    # halves of a piece exchanged, and the second half lost: the damage a transport has been measured to do
    c = np.concatenate([a[2500:], a[:2500]])
    z = a.copy(); z[2500:] = 0
    whole = mumemto_amd.exchange_digest(a, 5000)
    assert (mumemto_amd.exchange_digest(c, 5000) != whole).all() and (mumemto_amd.exchange_digest(z, 5000) != whole).all()


@pytest.mark.parametrize("width", [1, 4, 8])
def test_another_cut_gives_other_words_for_the_pieces_and_the_same_for_the_same_elements(width):
    a = random_values(width, 2000, 11)
    coarse, fine = mumemto_amd.exchange_digest(a, 500), mumemto_amd.exchange_digest(a, 250)
    assert coarse.shape == (4, 2) and fine.shape == (8, 2)
    assert (coarse[0] != fine[0]).all() and (coarse[1] != fine[1]).all()
    # a range of elements that is a piece of its own has the same words however it was reached
    assert np.array_equal(fine[1], mumemto_amd.exchange_digest(a[250:500], 250)[0])
    assert np.array_equal(fine[1], mumemto_amd.exchange_digest(a, 250, skip_elements=250)[0])
    assert np.array_equal(coarse[1], mumemto_amd.exchange_digest(a[500:1000], 500)[0])
    assert np.array_equal(coarse[1], mumemto_amd.exchange_digest(a, 500, skip_elements=500)[0])
