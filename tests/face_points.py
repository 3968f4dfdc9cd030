"""Operands for the tests of the face form (interp.h: face2_k / face3_k): the special-value grid and random bit patterns."""
import itertools

import numpy as np

F = np.float32


def _bits(*words):
    return np.array(words, np.uint32).view(F)


# every sign of: zero, a subnormal, FLT_MIN, 1, FLT_MAX, infinity, a quiet NaN
SPECIAL = np.concatenate([_bits(0x00000000, 0x00000001, 0x00800000, 0x3f800000, 0x7f7fffff, 0x7f800000, 0x7fc00000),
                          _bits(0x80000000, 0x80000001, 0x80800000, 0xbf800000, 0xff7fffff, 0xff800000, 0xffc00000)])


def grid(terms):
    """Every combination of the special values, one array per term."""
    g = np.array(list(itertools.product(SPECIAL.view(np.uint32), repeat=terms)), np.uint32)
    return [np.ascontiguousarray(g[:, t]).view(F) for t in range(terms)]


def random_bits(rng, n, terms):
    return [rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(F) for _ in range(terms)]


def same(a, b):
    """Equal bit for bit, or NaN on both sides (payloads are not part of any contract here)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
