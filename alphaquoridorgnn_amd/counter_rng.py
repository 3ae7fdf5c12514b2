"""The counter-based generator of csrc/counter_rng.hpp in Python (the recipe is in include/aqgnn.h): stream b of a seed is keyed by
K(seed, b) = mix(seed + GOLDEN (b + 1)), and draw i of a stream is u_i = (mix(key + GOLDEN (i + 1)) >> 11) 2^-53.  Every Python
restatement of a device draw -- the agents' uniforms, the root noise, the resignation draw, the derived seeds -- is built from these."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def _u64(x):
    """x mod 2^64 as numpy uint64: a Python int of any size and sign, or an integer array."""
    return np.uint64(x & MASK64) if isinstance(x, int) else np.asarray(x).astype(np.uint64)


def mix64(z):
    """The splitmix64 finaliser.  A Python int (taken mod 2^64) gives a Python int, a numpy uint64 value or array gives its like."""
    with np.errstate(over="ignore"):
        m = _u64(z)
        m = (m ^ (m >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        m = (m ^ (m >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        m = m ^ (m >> np.uint64(31))
    return int(m) if isinstance(z, int) else m


def stream_key(seed, b):
    """K(seed, b): the uint64 key of stream b under `seed`; either may be an int or an integer array (they broadcast)."""
    with np.errstate(over="ignore"):
        return mix64(_u64(seed) + np.uint64(GOLDEN) * (_u64(b) + np.uint64(1)))


def counter_uniform(key, i):
    """Draw i of the stream `key`: float64 in [0, 1); either may be an int or an integer array (they broadcast)."""
    return (stream_key(key, i) >> np.uint64(11)).astype(np.float64) * (2.0 ** -53)
