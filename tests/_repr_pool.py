"""The stratified pool of float32 bit patterns that the shortest-repr formatter is checked on, on
the host (tests/test_repr32_host.py, tools/asan/repr32_main.cpp uses the same strata) and on the
GPU (tests/test_xyz_text_gpu.py).  numpy's ``np.float32(v).astype(str)`` is the yardstick."""
from __future__ import annotations

import numpy as np

FIXED_MANTISSAS = (0, 1, 2, 0x400000, 0x7ffffe, 0x7fffff)

# even mantissas whose shortest decimal is an end point of the rounding interval, i.e. one digit
# shorter than anything strictly inside: 0x4c215b00 prints 42298370.0; the others were found by a
# seeded search (np.random.default_rng(20251019), normal even bit patterns, repr == an exact
# half-way point to a neighbour)
BOUNDARY_EVEN = (0x4c215b00, 0x4dc912da, 0x4cf8ca6c, 0x4dda688c, 0x4c470e82, 0x4c86ce98,
                 0x4cff28e4, 0x4c35a48a, 0x4c60d646)

NAMED = (
    0x38d1b717, 0x38d1b718, 0x5a0e1bc9, 0x5a0e1bca, 0x5a0e1bcb,  # the notation thresholds
    *BOUNDARY_EVEN,
    0x00000000, 0x80000000,                                       # +-0
    0x00000001, 0x007fffff, 0x00800000, 0x7f7fffff,               # subnormal ends, min normal, max
    0x3f800000, 0x4b800000, 0x3dcccccd, 0x477fe080,               # 1.0, 2^24, 0.1, 65504.5
)

# what numpy prints for some of them (a wrong yardstick would show here first)
KNOWN = {0x38d1b717: "1e-04", 0x38d1b718: "0.000100000005", 0x5a0e1bc9: "9999999000000000.0",
         0x5a0e1bca: "1e+16", 0x4c215b00: "42298370.0", 0x80000000: "-0.0", 0x00000001: "1e-45",
         0x00800000: "1.1754944e-38", 0x7f7fffff: "3.4028235e+38", 0x3f800000: "1.0",
         0x4b800000: "16777216.0", 0x3dcccccd: "0.1", 0x477fe080: "65504.5",
         0xb3bbbd2e: "-8.742278e-08"}


def pool_bits(random_per_exponent: int, seed: int = 1310) -> np.ndarray:
    """uint32 bit patterns of finite float32 values: the named ones, then for every biased
    exponent 0..254 and both signs the fixed mantissas and ``random_per_exponent`` seeded random
    ones."""
    rng = np.random.default_rng(seed)
    e = np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)
    fixed = np.array(FIXED_MANTISSAS, dtype=np.uint32)[None, :]
    rand = rng.integers(0, 1 << 23, (255, random_per_exponent), dtype=np.uint32)
    mag = np.concatenate([e | fixed, e | rand], axis=1).reshape(-1)
    named = np.array(NAMED + (0xb3bbbd2e,), dtype=np.uint32)
    return np.concatenate([named, mag, mag | np.uint32(0x80000000)])


def pool(random_per_exponent: int, seed: int = 1310) -> np.ndarray:
    return pool_bits(random_per_exponent, seed).view(np.float32)


def numpy_repr(values: np.ndarray) -> np.ndarray:
    """np.float32(v).astype(str) per value (the text to_csv writes for a float32 column)."""
    return np.asarray(values, dtype=np.float32).astype(str)
