"""hsrans_decode_device_gather's host side, without a GPU: the exported symbols, the ctypes mirrors of its two structs, and the pure
function that cuts byte ranges into one-wave tasks (hsrans_gather_tasks) — tiling, cuts at absolute multiples of the segment length,
destination deltas, the task bound, the capacity protocol and the refusals."""
import ctypes

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

FLOOR = 4096  # kGatherMinSegment (csrc/hsrans_capi_gather.cpp)
U64 = 1 << 64


def test_symbols_and_struct_sizes():
    L = H.load_library()
    assert hasattr(L, "hsrans_decode_device_gather") and hasattr(L, "hsrans_gather_tasks") and hasattr(L, "hsrans_gather_segment")
    assert ctypes.sizeof(api.Range) == 24 and ctypes.sizeof(api.GatherTask) == 24


def test_null_context_is_an_argument_error():
    L = H.load_library()
    r = (api.Range * 1)(api.Range(0, 1, 0))
    assert L.hsrans_decode_device_gather(None, None, None, 0, r, 1, None, 0, None) == 2


def _expected_segment(decoded_len, n_chains, states, interval):
    base = interval * states
    if base == 0:
        mean = -(-decoded_len // n_chains)
        base = max(-(-mean // states) * states, states)
    return base if base >= FLOOR else base * -(-FLOOR // base)


@pytest.mark.parametrize("decoded_len,n_chains,states,interval", [
    (100_000_000, 48_829, 64, 32), (100_000_000, 763, 64, 2048), (3_000_001, 46, 64, 0), (3_000_001, 1465, 32, 64), (1000, 1, 32, 0), (1 << 33, 1 << 20, 64, 128),
    (5_000_000, 2441, 64, 32)])
def test_segment_length(decoded_len, n_chains, states, interval):
    L = H.gather_segment(decoded_len, n_chains, states, interval)
    assert L == _expected_segment(decoded_len, n_chains, states, interval)
    assert L >= FLOOR and L % states == 0
    if interval * states >= FLOOR:
        assert L == interval * states
    elif interval:
        assert L % (interval * states) == 0  # tasks still start on checkpoints


def _check(decoded_len, n_chains, states, interval, ranges):
    ranges = np.asarray(ranges, dtype=np.uint64).reshape(-1, 3)
    L = H.gather_segment(decoded_len, n_chains, states, interval)
    tasks = H.gather_tasks(decoded_len, n_chains, states, interval, ranges)
    t = 0
    bound = 0
    for off, length, dst in ((int(a), int(b), int(c)) for a, b, c in ranges):
        if length == 0:
            continue  # no task
        bound += -(-length // L) + 1
        pos = off
        while pos < off + length:
            b, e, delta = (int(v) for v in tasks[t])
            assert b == pos and b < e <= off + length, (off, length, t)  # tiles the range exactly, in order
            assert b // L == (e - 1) // L, (b, e, L)                       # no task crosses an absolute multiple of L
            assert delta == (dst - off) % U64                             # the same for all tasks of the range
            pos = e
            t += 1
        assert pos == off + length
    assert t == tasks.shape[0]
    assert t <= bound
    return tasks


def test_edge_cases():
    n, chains, S, iv = 3_000_001, 1465, 64, 32
    L = H.gather_segment(n, chains, S, iv)
    tasks = _check(n, chains, S, iv, [(n - 10, 10, 0)])  # ends at decoded_len
    assert tasks.shape[0] == 1
    assert _check(n, chains, S, iv, [(12345, 1, 7)]).shape[0] == 1  # one byte
    assert _check(n, chains, S, iv, [(L - 1, 2, 0)]).shape[0] == 2  # one byte either side of a cut
    assert _check(n, chains, S, iv, [(L, L, 0)]).shape[0] == 1      # exactly one segment
    many = _check(n, chains, S, iv, [(100, 100 * L, 5)])             # spans many segments
    assert many.shape[0] == 101
    assert _check(n, chains, S, iv, [(500, 0, 0)]).shape[0] == 0    # empty: no task
    assert _check(n, chains, S, iv, [(0, 0, 0), (0, n, 0), (n, 0, 3)]).shape[0] == -(-n // L)
    assert _check(n, chains, S, iv, [(4000, 200, 0), (4000, 200, 200)]).shape[0] == 4  # the same source twice
    assert _check(n, chains, S, iv, [(1000, 10, 3)])[0, 2] == (3 - 1000) % U64         # a destination in front of its source: modulo 2^64


@pytest.mark.parametrize("seed", range(6))
def test_random_range_lists(seed):
    rng = np.random.default_rng(seed)
    states = (32, 64)[seed % 2]
    interval = (0, 32, 64, 1024)[seed % 4]
    n = int(rng.integers(1, 50_000_000))
    chains = max(1, n // (states * (interval or 700)))
    count = int(rng.integers(1, 400))
    lens = np.minimum((2.0 ** rng.uniform(0, 20, count)).astype(np.uint64), np.uint64(n))
    lens[rng.random(count) < 0.05] = 0
    offs = (rng.random(count) * (n - lens.astype(np.float64))).astype(np.uint64)
    dsts = rng.integers(0, 1 << 40, count).astype(np.uint64)
    _check(n, chains, states, interval, np.stack([offs, lens, dsts], axis=1))


def test_capacity_protocol():
    L = H.load_library()
    n, chains, S, iv = 3_000_001, 1465, 64, 32
    ranges = np.array([[10, 50_000, 0], [70_000, 9_000, 50_000]], np.uint64)
    need = L.hsrans_gather_tasks(n, chains, S, iv, ranges.ctypes.data, 2, None, 0)
    full = H.gather_tasks(n, chains, S, iv, ranges)
    assert need == full.shape[0] > 4
    short = np.full((need, 3), 0xCCCCCCCCCCCCCCCC, np.uint64)
    assert L.hsrans_gather_tasks(n, chains, S, iv, ranges.ctypes.data, 2, short.ctypes.data, 3) == need  # still the need
    assert np.array_equal(short[:3], full[:3]) and np.all(short[3:] == 0xCCCCCCCCCCCCCCCC)              # and not overrun
    assert np.array_equal(H.gather_tasks(n, chains, S, iv, ranges, capacity=2), full[:2])


def test_invalid_input_gives_zero():
    L = H.load_library()
    one = np.array([[0, 10, 0]], np.uint64)
    out = np.zeros((4, 3), np.uint64)
    assert L.hsrans_gather_tasks(1000, 4, 64, 0, None, 1, out.ctypes.data, 4) == 0                    # null ranges, count > 0
    assert L.hsrans_gather_tasks(1000, 0, 64, 0, one.ctypes.data, 1, out.ctypes.data, 4) == 0          # no chains
    past = np.array([[0, 10, 0], [995, 6, 0]], np.uint64)
    assert L.hsrans_gather_tasks(1000, 4, 64, 0, past.ctypes.data, 2, out.ctypes.data, 4) == 0         # a range beyond decoded_len
    beyond = np.array([[1001, 0, 0]], np.uint64)
    assert L.hsrans_gather_tasks(1000, 4, 64, 0, beyond.ctypes.data, 1, out.ctypes.data, 4) == 0
    wrap = np.array([[8, (1 << 64) - 4, 0]], np.uint64)
    assert L.hsrans_gather_tasks(1000, 4, 64, 0, wrap.ctypes.data, 1, out.ctypes.data, 4) == 0         # offset + length wraps
    assert not out.any()
    assert L.hsrans_gather_tasks(1000, 4, 64, 0, None, 0, None, 0) == 0                                 # nothing asked: nothing needed
    assert H.gather_segment(1000, 0, 64, 0) == 0
