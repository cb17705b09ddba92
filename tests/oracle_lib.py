"""ctypes loaders for the TEST ORACLES (never imported by the product):

* ``Oracle``  - oracle/libhsrans_oracle.so, the plain-C restatement of the reference algorithms;
* ``Ref``     - oracle/_ref/libhsrans_ref.so, the real reference compiled by oracle/Makefile where its sources lie (may be absent);
* ``RecordedRef`` - what the real reference returned for the tests' seeded inputs, replayed from tests/golden/reference_calls.json.gz
                (written by tests/golden/make_golden.py with ``Ref``): the tests' ``ref`` fixture, present in every checkout.
"""
from __future__ import annotations

import ctypes
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "libhsrans_oracle.so")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libhsrans_ref.so")
REFSPLIT_SO = os.path.join(ROOT, "oracle", "libhsrans_refsplit.so")
REF_RECORD = os.path.join(ROOT, "tests", "golden", "reference_calls.json.gz")

RAW, BLOCK, MT = 0, 1, 2
CONTAINER_NAMES = {RAW: "raw", BLOCK: "block", MT: "mt"}

_sz = ctypes.c_size_t
_vp = ctypes.c_void_p
_i = ctypes.c_int
_u = ctypes.c_uint


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_vp)


def digest(a: np.ndarray) -> str:
    """SHA-256 of an array's bytes, first 128 bits"""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


class OrcHist(ctypes.Structure):
    _fields_ = [("symbolCount", ctypes.c_uint16 * 256), ("cumul", ctypes.c_uint16 * 256)]


class Oracle:
    def __init__(self):
        if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(os.path.join(ROOT, "oracle", "hsrans_oracle.c")):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"])
        L = ctypes.CDLL(ORACLE_SO)
        L.orc_idx2idx.restype = ctypes.c_uint8
        L.orc_idx2idx.argtypes = [_u]
        L.orc_make_hist.restype = None
        L.orc_make_hist.argtypes = [ctypes.POINTER(OrcHist), _vp, _sz, _u]
        L.orc_make_dec_table.restype = _i
        L.orc_make_dec_table.argtypes = [_u, _vp, _vp, _vp, _i]
        L.orc_capacity.restype = _sz
        L.orc_capacity.argtypes = [_i, _i, _sz]
        L.orc_raw_encode.restype = _sz
        L.orc_raw_encode.argtypes = [_i, _u, _vp, _sz, _vp, _sz, ctypes.POINTER(OrcHist)]
        L.orc_decode.restype = _sz
        L.orc_decode.argtypes = [_i, _i, _u, _vp, _sz, _vp, _sz]
        L.orc_exec_plan.restype = _sz
        L.orc_exec_plan.argtypes = [_vp, _sz, _vp, _sz, _vp, _sz]
        self.L = L

    def exec_plan(self, plan: np.ndarray, stream: np.ndarray, out_cap: int):
        plan = np.ascontiguousarray(plan, dtype=np.uint8)
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        out = np.full(max(out_cap, 1), 0xCC, np.uint8)
        r = self.L.orc_exec_plan(_ptr(plan), plan.size, _ptr(stream), stream.size, _ptr(out), out_cap)
        return r, out[:out_cap]

    def idx2idx(self, j):
        return self.L.orc_idx2idx(j)

    def capacity(self, container, states, n):
        return self.L.orc_capacity(container, states, n)

    def make_hist(self, data: np.ndarray, bits: int) -> OrcHist:
        h = OrcHist()
        self.L.orc_make_hist(ctypes.byref(h), _ptr(data), data.size, bits)
        return h

    def hist_from_counts(self, counts) -> OrcHist:
        h = OrcHist()
        c = 0
        for k in range(256):
            h.symbolCount[k] = int(counts[k])
            h.cumul[k] = c & 0xFFFF
            c += int(counts[k])
        return h

    def make_dec_table(self, bits, counts: np.ndarray, wide_sum=0):
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        cumul = np.zeros(256, np.uint16)
        inv = np.zeros(1 << bits, np.uint8)
        ok = self.L.orc_make_dec_table(bits, _ptr(counts), _ptr(cumul), _ptr(inv), wide_sum)
        return ok, cumul, inv

    def raw_encode(self, states, bits, data: np.ndarray, hist: OrcHist | None = None) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if hist is None:
            hist = self.make_hist(data, bits)
        cap = self.capacity(RAW, states, data.size)
        out = np.zeros(cap, np.uint8)
        m = self.L.orc_raw_encode(states, bits, _ptr(data), data.size, _ptr(out), cap, ctypes.byref(hist))
        return out[:m].copy()

    def decode(self, container, states, bits, stream: np.ndarray, out_cap: int, in_len: int | None = None):
        """Returns (returned_length, output buffer of out_cap bytes pre-filled with 0xCC)."""
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        out = np.full(max(out_cap, 1), 0xCC, np.uint8)
        r = self.L.orc_decode(container, states, bits, _ptr(stream), stream.size if in_len is None else in_len, _ptr(out), out_cap)
        return r, out[:out_cap]


class Ref:
    """The real reference (only where oracle/_ref/libhsrans_ref.so has been built)."""

    def timed_decode(self, container, states, bits, stream: np.ndarray, out_cap: int, variant: int = 0, threads: int = 0, runs: int = 3, budget_s: float = 4.0,
                     max_runs: int = 40):
        """Best wall time of the C call alone (buffers allocated and touched beforehand), the output of the last run, and the run count."""
        import time

        buf = np.zeros(stream.size + 64, np.uint8)
        buf[:stream.size] = stream
        out = np.full(max(out_cap, 1) + 64, 0xCC, np.uint8)
        best, n, total = None, 0, 0.0
        while n < runs or (total < budget_s and n < max_runs):
            t0 = time.perf_counter()
            r = self.L.hsref_decode(container, states, bits, variant, _ptr(buf), stream.size, _ptr(out), out_cap, threads)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            total += dt
            n += 1
        return best, r, out[:out_cap], n

    @staticmethod
    def available() -> bool:
        return os.path.exists(REF_SO)

    def __init__(self):
        L = ctypes.CDLL(REF_SO)
        L.hsref_capacity.restype = _sz
        L.hsref_capacity.argtypes = [_i, _i, _sz]
        L.hsref_make_hist.restype = None
        L.hsref_make_hist.argtypes = [_vp, _sz, _i, _vp, _vp]
        L.hsref_encode.restype = _sz
        L.hsref_encode.argtypes = [_i, _i, _i, _vp, _sz, _vp, _sz, _vp]
        L.hsref_decode.restype = _sz
        L.hsref_decode.argtypes = [_i, _i, _i, _i, _vp, _sz, _vp, _sz, _i]
        L.hsref_pool_threads.restype = _sz
        L.hsref_has_avx2.restype = _i
        L.hsref_has_avx512.restype = _i
        self.L = L

    def has_avx512(self) -> bool:
        return bool(self.L.hsref_has_avx512())

    def capacity(self, container, states, n):
        return self.L.hsref_capacity(container, states, n)

    def make_hist(self, data: np.ndarray, bits: int):
        counts = np.zeros(256, np.uint16)
        cumul = np.zeros(256, np.uint16)
        self.L.hsref_make_hist(_ptr(data), data.size, bits, _ptr(counts), _ptr(cumul))
        return counts, cumul

    def encode(self, container, states, bits, data: np.ndarray, counts=None) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        cap = self.capacity(container, states, data.size)
        out = np.zeros(cap + 64, np.uint8)
        cp = None
        if counts is not None:
            counts = np.ascontiguousarray(counts, dtype=np.uint16)
            cp = _ptr(counts)
        m = self.L.hsref_encode(container, states, bits, _ptr(data), data.size, _ptr(out), cap, cp)
        return out[:m].copy()

    def decode(self, container, states, bits, stream: np.ndarray, out_cap: int, variant: int = 0, threads: int = 0, pad: int = 64):
        """variant 0: scalar (raw) / runtime dispatch (block_, mt_); 1: fastest AVX2 raw; 2: mt_ thread pool; 3: fastest AVX-512 raw."""
        buf = np.zeros(stream.size + pad, np.uint8)  # SIMD variants over-read up to 32 B
        buf[:stream.size] = stream
        out = np.full(max(out_cap, 1) + 64, 0xCC, np.uint8)
        r = self.L.hsref_decode(container, states, bits, variant, _ptr(buf), stream.size, _ptr(out), out_cap, threads)
        return r, out[:out_cap]

    def decode_digest(self, container, states, bits, stream: np.ndarray, out_cap: int, variant: int = 0):
        """(returned_length, SHA-256 of the out_cap-byte output buffer, pre-filled with 0xCC)"""
        r, out = self.decode(container, states, bits, stream, out_cap, variant=variant)
        return int(r), digest(out)


class RecordedRef:
    """The real reference's results for the seeded inputs of the tests, replayed from tests/golden/reference_calls.json.gz.

    Same calls as ``Ref``, so the tests are the same with either:
      make_hist     the reference's histogram counts (cumul is their prefix sum);
      encode        the reference's stream, rebuilt and accepted only when its length and SHA-256 are the recorded stream's:
                    the product encoder's bytes, or, where the product merges a last block shorter than S symbols into the one
                    before it and the reference does not, those of oracle/libhsrans_refsplit.so (the same encoder without that merge);
      decode_digest (returned length, SHA-256 of the output buffer) of the reference's decoder.
    Hashes are SHA-256 cut to 128 bits.  A call that is not in the record fails: regenerate the record with
    tests/golden/make_golden.py.  With ``live`` (a ``Ref``) every call is answered by the real reference and recorded;
    ``save()`` writes the record."""

    def __init__(self, live: Ref | None = None, path: str = REF_RECORD):
        self.live, self.path = live, path
        self.calls = {}
        if live is None:
            with gzip.open(path, "rt") as f:
                self.calls = json.load(f)["calls"]
        self._split = None

    def save(self, path: str | None = None):
        text = json.dumps({"source": "tests/golden/make_golden.py: the real reference (oracle/_ref/libhsrans_ref.so)",
                           "calls": dict(sorted(self.calls.items()))}, separators=(",", ":"))
        with open(path or self.path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
            z.write(text.encode())

    def _get(self, key: str):
        if key not in self.calls:
            raise KeyError(f"no recorded reference result for {key}: regenerate {os.path.basename(self.path)} with tests/golden/make_golden.py")
        return self.calls[key]

    def _split_encode(self, container, states, bits, data: np.ndarray) -> np.ndarray:
        if self._split is None:
            if not os.path.exists(REFSPLIT_SO) or os.path.getmtime(REFSPLIT_SO) < os.path.getmtime(os.path.join(ROOT, "oracle", "refsplit_shim.cpp")):
                subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "oracle"])
            self._split = ctypes.CDLL(REFSPLIT_SO)
            self._split.orc_refsplit_encode.restype = _sz
            self._split.orc_refsplit_encode.argtypes = [_i, _i, _u, _vp, _sz, _vp, _sz]
        import hypersonic_rans_amd as H

        cap = H.capacity(container, states, data.size)
        out = np.zeros(cap, np.uint8)
        m = self._split.orc_refsplit_encode(container, states, bits, _ptr(data), data.size, _ptr(out), cap)
        return out[:m].copy()

    def make_hist(self, data: np.ndarray, bits: int):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        key = f"hist b{bits} n{data.size} {digest(data)}"
        if self.live is not None:
            self.calls[key] = [int(c) for c in self.live.make_hist(data, bits)[0]]
        counts = np.asarray(self._get(key), dtype=np.uint16)
        cumul = (np.cumsum(counts, dtype=np.uint32) - counts).astype(np.uint16)
        return counts, cumul

    def encode(self, container, states, bits, data: np.ndarray) -> np.ndarray:
        data = np.ascontiguousarray(data, dtype=np.uint8)
        key = f"encode {CONTAINER_NAMES[container]} s{states} b{bits} n{data.size} {digest(data)}"
        if self.live is not None:
            s = self.live.encode(container, states, bits, data)
            self.calls[key] = [int(s.size), digest(s)]
            return s
        size, sha = self._get(key)
        import hypersonic_rans_amd as H

        s = H.encode(container, states, bits, data)
        if (s.size, digest(s)) != (size, sha) and container != RAW:
            s = self._split_encode(container, states, bits, data)
        assert s.size == size and digest(s) == sha, f"no encoder here reproduces the reference's stream ({key}: {s.size} bytes, reference {size})"
        return s

    def decode_digest(self, container, states, bits, stream: np.ndarray, out_cap: int, variant: int = 0):
        stream = np.ascontiguousarray(stream, dtype=np.uint8)
        key = f"decode {CONTAINER_NAMES[container]} s{states} b{bits} v{variant} cap{out_cap} n{stream.size} {digest(stream)}"
        if self.live is not None:
            self.calls[key] = list(self.live.decode_digest(container, states, bits, stream, out_cap, variant=variant))
        r, sha = self._get(key)
        return int(r), sha
