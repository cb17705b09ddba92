"""hsrans_decode_host without a plan on a block_ stream (the reference's decodeFunc shape): the first call's walk records an index, the
context keeps it, and later calls on the same bytes launch it — the block_ counterpart of
tests/test_gpu_parity.py::test_plain_host_decode_keeps_the_index_of_its_first_call."""
import ctypes

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from oracle_lib import BLOCK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zipf():
    return synth.enwik8_shaped(1 << 20, seed=11)


@pytest.fixture(scope="module")
def nonstat():
    return synth.nonstationary(3_000_000)


def _cpu_decode(states, bits, stream, n):
    """the library's host decoder (hsrans_decode_cpu, scalar route): a second implementation for streams no encoder wrote"""
    out = np.full(n, 0xCC, np.uint8)
    r = H.load_library().hsrans_decode_cpu(0, 1, H.BLOCK, states, bits, stream.ctypes.data, stream.size, out.ctypes.data, n, None, 0)
    return r, out


def test_plain_host_decode_keeps_a_block_streams_index(ref, zipf, nonstat):
    n = 3_000_000
    d = nonstat[:n]
    s = np.ascontiguousarray(ref.encode(BLOCK, 64, 11, d))
    ctx = H.Context(0)  # (its own context: the cache belongs to it)
    assert ctx.host_index_chains() == 0
    r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
    assert r == n and np.array_equal(got, d)
    chains = ctx.host_index_chains()
    assert chains > 100
    for _ in range(3):
        r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
        assert r == n and np.array_equal(got, d) and ctx.host_index_chains() == chains
    # one bit of one word flipped IN PLACE: a decoder that trusted the address would emit the old states' bytes
    s[s.size // 2] ^= 0x10
    want_r, want = _cpu_decode(64, 11, s, n)
    r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
    assert r == want_r and np.array_equal(got[:r], want[:r]) and not np.array_equal(got, d)
    s[s.size // 2] ^= 0x10
    r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
    assert r == n and np.array_equal(got, d)
    # another codec is not served from the cache; a stream below 1 MiB leaves the cache as it is
    s2 = np.ascontiguousarray(ref.encode(BLOCK, 32, 13, d))
    r, got = ctx.decode_host(H.BLOCK, 32, 13, s2, n)
    assert r == n and np.array_equal(got, d)
    kept = ctx.host_index_chains()
    small = np.ascontiguousarray(ref.encode(BLOCK, 64, 11, zipf[:524_300]))
    want_r, want = _cpu_decode(64, 11, small, 524_300)  # (a length whose last bytes the reference itself mis-decodes)
    r, got = ctx.decode_host(H.BLOCK, 64, 11, small, 524_300)
    assert r == want_r and np.array_equal(got[:r], want[:r]) and ctx.host_index_chains() == kept
    r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
    assert r == n and np.array_equal(got, d)


def test_cache_switched_off(ref, nonstat, monkeypatch):
    n = 3_000_000
    d = nonstat[:n]
    s = np.ascontiguousarray(ref.encode(BLOCK, 64, 11, d))
    monkeypatch.setenv("HSRANS_HOST_INDEX_CACHE_OFF", "1")
    ctx = H.Context(0)
    for _ in range(2):
        r, got = ctx.decode_host(H.BLOCK, 64, 11, s, n)
        assert r == n and np.array_equal(got, d) and ctx.host_index_chains() == 0


@pytest.mark.parametrize("name", ("hsrans_block_rANS32x64_16w_decode_11", "hsrans_block_rANS32x64_16w_decode_hip_11"))
def test_drop_in_names_twice_on_one_buffer(gpu_ctx, ref, nonstat, name):
    """the reference's decoder name (runtime dispatch) and its GPU-only twin (hsrans_decode_host on the library's own context: the second
    call launches the index the first one left), resolved as tests/test_dropin_link.py resolves the C aliases"""
    n = 3_000_000
    d = nonstat[:n]
    s = np.ascontiguousarray(ref.encode(BLOCK, 64, 11, d))
    f = getattr(ctypes.CDLL(H.lib_path()), name)
    f.restype = ctypes.c_size_t
    f.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    for _ in range(2):
        got = np.full(n + 64, 0xCC, np.uint8)
        assert f(s.ctypes.data, s.size, got.ctypes.data, n) == n
        assert np.array_equal(got[:n], d) and bool((got[n:] == 0xCC).all())
