#!/usr/bin/env python3
"""Generates the golden vectors in this directory from the REAL reference (oracle/_ref/libhsrans_ref.so, built from
/root/reference/src by oracle/Makefile).  Run in the build container only; the vectors (data, not code) are committed.

  small_vectors.npz   for every container x states x bits: the reference-ENCODED stream of a small seeded input and what
                      the reference DECODER returns for it (+ a few "quirk" lengths where the reference's own round trip
                      is wrong, SURVEY.md §8 quirks: the bytes held here are what the reference produces)
  manifest.json       SHA-256 of stream / decoded output for 1 MiB inputs (too big to commit), raw histogram counts,
                      and the reference's capacity() values
  reference_calls.json.gz  what the reference returned for every call the tests make of the ``ref`` fixture (oracle_lib.RecordedRef):
                      tests/test_oracle_vs_ref.py run against the compiled reference, plus the reference-encoded streams of the
                      GPU tests (tests/test_gpu_parity.py) and the reference's histograms of the designed blocks of
                      tests/test_normalise_host.py, enumerated below.  `make_golden.py --calls` writes this file only.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from hypersonic_rans_amd import synth  # noqa: E402  (pure numpy data generator)
from oracle_lib import BLOCK, MT, RAW, RecordedRef, Ref  # noqa: E402

NAMES = {RAW: "raw", BLOCK: "block", MT: "mt"}


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ref = Ref()
    small = {}
    manifest = {"source": "rainerzufalldererste/hypersonic-rANS @ 2024_10_08, clang++ -O3 -std=c++20 -mxsave (oracle/Makefile)", "large": [], "capacity": [],
                "hist": []}
    zipf_small = synth.enwik8_shaped(3000, seed=101)
    two = synth.two_symbol(3000, seed=5)
    big = synth.enwik8_shaped(1 << 20, seed=1)
    uni = synth.uniform_bytes(1 << 20, seed=1)
    nonstat = synth.nonstationary(1 << 20, seed=99)
    for cont in (RAW, BLOCK, MT):
        for S in (32, 64):
            for n in (0, 1, 63, 64, 65, 1000, 65536, 100_000_000):
                manifest["capacity"].append({"container": NAMES[cont], "states": S, "n": n, "capacity": int(ref.capacity(cont, S, n))})
            for bits in range(10, 16):
                for tag, data in (("zipf3000", zipf_small), ("two3000", two), ("zipf127", zipf_small[:127]), ("zipf64", zipf_small[:64])):
                    if cont != RAW and tag in ("zipf127", "zipf64") and bits != 11:
                        continue
                    s = ref.encode(cont, S, bits, data)
                    r, dec = ref.decode(cont, S, bits, s, data.size)
                    assert r == data.size and np.array_equal(dec, data), (cont, S, bits, tag)
                    key = f"{NAMES[cont]}_s{S}_b{bits}_{tag}"
                    small[key + "_in"] = data.copy()
                    small[key + "_stream"] = s
                # 1 MiB inputs: hashes only
                for tag, data in (("zipf1M_seed1", big), ("uniform1M_seed1", uni), ("nonstat1M_seed99", nonstat)):
                    if cont != RAW and bits not in (11, 14) and tag != "nonstat1M_seed99":
                        continue
                    s = ref.encode(cont, S, bits, data)
                    r, dec = ref.decode(cont, S, bits, s, data.size)
                    assert r == data.size and np.array_equal(dec, data)
                    manifest["large"].append({"container": NAMES[cont], "states": S, "bits": bits, "input": tag, "n": int(data.size),
                                              "stream_len": int(s.size), "stream_sha256": sha(s), "decoded_sha256": sha(dec)})
    # quirk lengths: reference round trip is wrong for MinBlockSize < n < MinBlockSize + S; keep what its decoder returns
    zq = synth.enwik8_shaped(65600, seed=7)
    for cont, S, bits, n in ((MT, 64, 11, 65560), (MT, 32, 11, 65550), (MT, 64, 11, 65599), (BLOCK, 64, 12, 65560)):
        d = zq[:n]
        s = ref.encode(cont, S, bits, d)
        r, dec = ref.decode(cont, S, bits, s, n)
        key = f"quirk_{NAMES[cont]}_s{S}_b{bits}_n{n}"
        small[key + "_stream"] = s
        small[key + "_decoded"] = dec.copy()
        small[key + "_in_sha"] = np.frombuffer(bytes.fromhex(sha(d)), dtype=np.uint8)
        manifest.setdefault("quirks", []).append({"key": key, "returned": int(r), "round_trip_ok": bool(np.array_equal(dec, d)),
                                                   "mismatching_bytes": int((dec != d).sum())})
    for bits in range(10, 16):
        for tag, data in (("zipf1M_seed1", big), ("uniform1M_seed1", uni), ("two3000", two)):
            counts, cumul = ref.make_hist(data, bits)
            manifest["hist"].append({"input": tag, "bits": bits, "counts": [int(c) for c in counts]})
    np.savez_compressed(os.path.join(HERE, "small_vectors.npz"), **small)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=0)
    print("wrote", len(small), "arrays;", os.path.getsize(os.path.join(HERE, "small_vectors.npz")), "bytes npz")


def _gpu_test_encodes(rec: RecordedRef):
    """The ref.encode calls of tests/test_gpu_parity.py (its zipf / nonstat fixtures and case lists)."""
    zipf, nonstat = synth.enwik8_shaped(1 << 20, seed=11), synth.nonstationary(3_000_000)
    for cont in (RAW, BLOCK, MT):  # test_reference_encoded_streams
        for S in (32, 64):
            for bits in range(10, 16):
                for src, n in ((zipf, 65537), (zipf, 65560), (zipf, 65599), (zipf, 65600), (zipf, 131073), (zipf, 524300), (nonstat, 3_000_000)):
                    rec.encode(cont, S, bits, src[:n])
    for S in (32, 64):
        for bits, src, n in ((11, zipf, 65560), (14, zipf, 1 << 20), (11, nonstat, 3_000_000)):  # test_device_side_mt_walk_matches_host_planner,
            rec.encode(MT, S, bits, src[:n])                                                      # test_index_build_for_reference_mt_streams,
        rec.encode(RAW, S, 11, zipf[:400_037])                                                    # test_first_decode_of_an_unindexed_stream_...
        for bits in (11, 13):  # test_index_build_for_block_streams
            for src, n in ((nonstat, 3_000_000), (zipf, 1 << 20), (zipf, 524_300)):
                rec.encode(BLOCK, S, bits, src[:n])
    n = 3_000_000  # test_plain_host_decode_keeps_the_index_of_its_first_call
    for cont in (MT, RAW):
        rec.encode(cont, 64, 11, nonstat[:n])
        rec.encode(cont, 32, 12, nonstat[:n][::-1])
        rec.encode(cont, 64, 11, nonstat[:300_000])
    runs = np.concatenate([np.full(70_000, 7, np.uint8), zipf[:100_000], np.full(200_000, 200, np.uint8), zipf[:33]])
    one = np.full(50_000, 65, np.uint8)
    for S in (32, 64):  # test_gpu_raw_encoder_matches_host_encoder_and_reference
        for bits in range(10, 16):
            for src, n in ((zipf, 1), (zipf, 31), (zipf, 63), (zipf, 64), (zipf, 65), (zipf, 255), (zipf, 256), (zipf, 4096 + 17), (zipf, 8192), (zipf, 12288 + 64 + 3),
                           (zipf, 100_000), (zipf, 300_001), (nonstat, 1_000_003), (runs, runs.size), (one, one.size)):
                rec.encode(RAW, S, bits, src[:n])


def _normalise_hists(rec: RecordedRef):
    """The ref.make_hist calls of tests/test_normalise_host.py: the boundary and extreme blocks of tests/normalise_inputs.py."""
    import normalise_inputs

    for bits, block in normalise_inputs.reference_subset():
        rec.make_hist(block, bits)


def record_calls():
    """reference_calls.json.gz: the CPU differential tests run against the compiled reference, then the GPU tests' encodes; every
    entry is then replayed once (the product encoder must reproduce each recorded stream)."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "calls.json.gz")
        subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_ref.py")],
                              cwd=ROOT, env=dict(os.environ, HSRANS_REF_RECORD=path))
        rec = RecordedRef(live=Ref())
        rec.calls = RecordedRef(path=path).calls
    _gpu_test_encodes(rec)
    _normalise_hists(rec)
    rec.save()
    _gpu_test_encodes(RecordedRef())
    _normalise_hists(RecordedRef())
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_oracle_vs_ref.py")], cwd=ROOT)
    print("wrote", len(rec.calls), "reference calls;", os.path.getsize(rec.path), "bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["--calls"]:
        record_calls()
    else:
        main()
        record_calls()
