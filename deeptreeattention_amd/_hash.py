"""The counter hash of the sampling features (abundance, split, treedata, levels): THE definition, in NumPy and Python
integers; csrc/hash_dev.h is the same hash on the device, bit for bit.  Unsigned 64-bit arithmetic, modulo 2^64:
    mix(z)                = z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^ (z >> 31)
    stream_key(seed, s)   = mix(seed * GOLDEN + s + 1)                      GOLDEN = 0x9E3779B97F4A7C15
    the draw at counter c = mix(c * GOLDEN + stream_key(seed, s))           draw24: its top 24 bits, draw32: its top 32
    a shuffle of n        entry i draws draw32 at the counter (base + i) mod 2^64, base = shuffle_base(epoch or iteration, n);
                          the order: the entries ascending by (draw32 << 32) | i -- distinct keys, so stable and exact
The streams in use are listed in csrc/hash_dev.h and DESIGN.md section 4; a new feature takes a number that is not there.
This is oracle/prng.py's construction, restated because the product never imports the oracle."""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
STREAM_ABUNDANCE_KEEP, STREAM_ABUNDANCE_DRAW, STREAM_SPLIT = 0, 1, 0      # (_lib.LEVEL_STREAM, _lib.EPOCH_ORDER_STREAM + level)
STREAM_DEAD_FLIP = 3           # dead.flips_np (_lib.DEAD_FLIP_STREAM); the image pool's order is level id DEAD_ORDER_LEVEL
DEAD_ORDER_LEVEL = 63          # _lib.DEAD_ORDER_LEVEL: stream EPOCH_ORDER_STREAM + 63


def mix_int(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix(z):
    """mix on a uint64 array, under np.errstate(over="ignore"): wrapping is the point."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def stream_key(seed, stream):
    return mix_int(((int(seed) & M64) * GOLDEN + int(stream) + 1) & M64)


def _draw(seed, stream, counter):
    with np.errstate(over="ignore"):
        return mix(np.asarray(counter, np.uint64) * np.uint64(GOLDEN) + np.uint64(stream_key(seed, stream)))


def draw24(seed, stream, counter):
    """24-bit integers (int64) for the uint64 counters `counter` under (seed, stream)."""
    return (_draw(seed, stream, counter) >> np.uint64(40)).astype(np.int64)


def shuffle_base(turn, n):
    """(turn * n) mod 2^64, a Python integer: the first counter of shuffle number `turn` (an epoch, an iteration) of n."""
    return ((int(turn) & M64) * int(n)) & M64


def draw32(seed, stream, base, n):
    """The 32-bit draws (uint64 [n]) at the counters (base + i) mod 2^64, i < n.  base: a Python integer, or a sequence of
    m of them (Python integers: NumPy would turn a list that holds 2^63 and more into float64), which gives [m][n]."""
    many = isinstance(base, (list, tuple, np.ndarray))
    b = np.array([int(x) & M64 for x in base], np.uint64)[:, None] if many else np.uint64(int(base) & M64)
    with np.errstate(over="ignore"):
        return _draw(seed, stream, b + np.arange(int(n), dtype=np.uint64)) >> np.uint64(32)


def order_of(draw):
    """The shuffle that the draws of draw32 give: int32, the stable argsort of (draw << 32) | i along the last axis."""
    d = np.asarray(draw, np.uint64)
    return np.argsort((d << np.uint64(32)) | np.arange(d.shape[-1], dtype=np.uint64), axis=-1, kind="stable").astype(np.int32)


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
