"""The counter hash (deeptreeattention_amd/_hash.py) against its formula in Python integers, where the 64-bit counter
base + i crosses 2^32 and wraps 2^64."""
import numpy as np
import pytest

M = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def draws_int(seed, stream, base, n, shift):
    key = mix_int(((seed & M) * GOLDEN + stream + 1) & M)
    return [mix_int((((base + i) & M) * GOLDEN + key) & M) >> shift for i in range(n)]


BASES = (0, 2 ** 32 - 3, 2 ** 63 - 2, 2 ** 64 - 4, 2 ** 64 - 1)      # base + i crosses 2^32, 2^63 and wraps 2^64 within n = 9
N = 9


@pytest.mark.parametrize("seed, stream", [(0, 0), (5, 1), (2 ** 64 - 1, 79), (2 ** 40, 2)])
def test_draw32_and_order_of_are_the_integer_formula(seed, stream):
    from deeptreeattention_amd import _hash as H
    assert H.GOLDEN == GOLDEN and H.stream_key(seed, stream) == mix_int(((seed & M) * GOLDEN + stream + 1) & M)
    assert H.stream_key(seed + 2 ** 64, stream) == H.stream_key(seed, stream)
    want = [draws_int(seed, stream, b, N, 32) for b in BASES]
    for b, w in zip(BASES, want):
        d = H.draw32(seed, stream, b, N)
        assert d.dtype == np.uint64 and d.shape == (N,) and d.tolist() == w and max(w) < 2 ** 32
        assert H.order_of(d).dtype == np.int32 and H.order_of(d).tolist() == [i for _, i in sorted(zip(w, range(N)))]
        counters = np.array([(b + i) & M for i in range(N)], np.uint64)
        assert H.draw24(seed, stream, counters).tolist() == draws_int(seed, stream, b, N, 40)
    many = H.draw32(seed, stream, list(BASES), N)                    # a sequence of bases: one row each
    assert many.shape == (len(BASES), N) and many.tolist() == want
    assert H.order_of(many).tolist() == [H.order_of(np.array(w, np.uint64)).tolist() for w in want]
    assert H.draw32(seed, stream, np.array(BASES, np.uint64), N).tolist() == want
    assert [H.shuffle_base(t, N) for t in (0, 3, 2 ** 63 + 1, 2 ** 64 + 3)] == [0, 27, ((2 ** 63 + 1) * N) & M, 27]


def test_order_of_breaks_equal_draws_by_index():
    from deeptreeattention_amd import _hash as H
    assert H.order_of(np.array([7, 3, 7, 3, 0], np.uint64)).tolist() == [4, 1, 3, 0, 2]
    assert H.order_of(np.array([2 ** 32 - 1, 0], np.uint64)).tolist() == [1, 0]      # the top draw stays below the padding
