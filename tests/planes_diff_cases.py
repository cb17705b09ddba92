"""What the diff byte-plane tests share (test_planes_diff_abi.py on the host, test_gpu_planes_diff.py on the device): the rule in numpy, and
the element pairs at which an arithmetic difference, unlike an XOR, can go wrong — carries and borrows through every byte, across the dword
boundary of an 8-byte element and between the two 2-byte elements of a dword — planted into random tensors."""
import numpy as np

NP_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}


def zigzag(a, b):
    """z of `a` against `b` (arrays of one unsigned dtype): d = a - b modulo 2^(8 W), z = (d << 1) ^ (0 - (d >> (8 W - 1)))"""
    t = a.dtype.type
    d = a - b  # (unsigned arrays wrap)
    return (d << t(1)) ^ (np.zeros_like(d) - (d >> t(8 * a.itemsize - 1)))


def unzigzag(z, b):
    """the inverse: d = (z >> 1) ^ (0 - (z & 1)), a = b + d"""
    t = z.dtype.type
    return b + ((z >> t(1)) ^ (np.zeros_like(z) - (z & t(1))))


def planes_of(z):
    """plane p = byte p of every element"""
    rows = np.ascontiguousarray(z).view(np.uint8).reshape(-1, z.itemsize)
    return [np.ascontiguousarray(rows[:, p]) for p in range(z.itemsize)]


def carry_cases(W):
    """(in, base): consecutive elements, an even number of them, to be planted at an even index so that for W = 2 elements 4 and 5 share a dword"""
    bits = 8 * W
    ones, top = (1 << bits) - 1, 1 << (bits - 1)
    pairs = [
        (0, ones),                                         # d = +1 by a wrap: in = 0, base = all ones
        (top, 0),                                          # d = 2^(8 W - 1): z is all ones
        (1 << (bits - 8), (1 << (bits - 8)) - 1),          # a borrow through every byte: 0x01 00..00 - 0x00 FF..FF
    ]
    if W != 8:
        pairs.append((ones, 0))                            # d = -1
    if W == 2:
        # elements 4 and 5, one dword: a borrow (split) and a carry (merge) in its low half, none in its high half — nothing may leak
        # between the packed halves (elements 0 and 1 are such a dword too: base 0xFFFF and d = +1 below d = 0x8000)
        pairs += [(0x0000, 0x0001), (0x0005, 0x0005)]
    if W == 8:
        low = 0x00000001_FFFFFFFF  # the base's low dword all ones, d = +1 and d = -1: the carry crosses the dword boundary
        pairs += [(low + 1, low), (low - 1, low), (0x00000001_00000000 - 1, 0x00000001_00000000)]  # ... and a borrow that does
    assert len(pairs) in (4, 6)
    t = NP_UINT[W]
    return np.array([p[0] for p in pairs], t), np.array([p[1] for p in pairs], t)


CARRY_N = 94  # five full 16-element blocks and a tail of 14


def planted(W, seed):
    """(in, base, starts): CARRY_N random elements with the carry cases planted as the first elements, inside a full block, in the tail and
    as the last elements"""
    rng = np.random.default_rng(seed * 100 + W)
    a = rng.integers(0, 256, CARRY_N * W, dtype=np.uint8).view(NP_UINT[W]).copy()
    b = rng.integers(0, 256, CARRY_N * W, dtype=np.uint8).view(NP_UINT[W]).copy()
    ca, cb = carry_cases(W)
    L = ca.size
    whole = CARRY_N // 16 * 16
    starts = [0, 32, whole, CARRY_N - L]
    assert L % 2 == 0 and 32 + L <= 48 and whole + L <= CARRY_N - L and all(s % 2 == 0 for s in starts)
    for s in starts:
        a[s: s + L], b[s: s + L] = ca, cb
    return a, b, starts
