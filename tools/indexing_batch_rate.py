"""The first decode of many streams: one hsrans_decode_device_indexing_batch call against K hsrans_decode_device_indexing calls.
K = 8 / 32 / 128 block_ streams of 1 MB and 4 MB (enwik8-shaped, 64 states, 11 bits, the host encoder's default blocks — byte-identical to the
reference's streams — interval 32), every member a different slice of the data; then the same with mt_ streams in 64 KiB blocks.  Legs per
shape, rotated, the host clock around the synchronous calls, fresh base plans (hsrans_dplan_create_from_device_stream, not timed) for every
leg of every repetition, every member's bytes compared after every leg:
  batch    one batch call for the K members
  singles  K single calls, one after the other
  largest  the single call of the largest member alone (for information: what the batch cannot be faster than, plus assembly)
One JSON line per leg and shape (median and quartiles over the repetitions after one dropped round), one line of ratios per shape.
Run on the GPU box:
  python tools/indexing_batch_rate.py [--reps R] [--members 8,32,128] [--sizes 1000000,4000000] [--out profiles/r15_indexing_batch_rate.jsonl]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--members", default="8,32,128")
ap.add_argument("--sizes", default="1000000,4000000")
ap.add_argument("--containers", default="block,mt")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r15_indexing_batch_rate.jsonl"))
args = ap.parse_args()
assert args.reps >= 16, "medians and quartiles of at least 16 repetitions"
KS = [int(v) for v in args.members.split(",")]
SIZES = [int(v) for v in args.sizes.split(",")]
S, BITS, INTERVAL, MT_BLOCK = 64, 11, 32, 1 << 16

ctx = H.Context(0)
pool = synth.enwik8_shaped(2 * max(SIZES), seed=15)
lines = []


def emit(line):
    lines.append(line)
    print(json.dumps(line), flush=True)


for cname in args.containers.split(","):
    container = H.BLOCK if cname == "block" else H.MT
    for size in SIZES:
        # member k: its own slice of the pool (k = 0 is the largest stream among equals: the slices have one length)
        members = []
        for k in range(max(KS)):
            off = (k * 64 * 31_337) % (pool.size - size)
            d = pool[off:off + size]
            s = H.encode(container, S, BITS, d, block_size=MT_BLOCK) if container == H.MT else H.encode(container, S, BITS, d)
            members.append({"m": s.size, "d_in": torch.from_numpy(np.concatenate([s, np.zeros((-s.size) % 16, np.uint8)])).cuda(), "d_ref": torch.from_numpy(d).cuda(),
                            "d_out": torch.zeros(size, dtype=torch.uint8, device="cuda")})
        largest = max(range(len(members)), key=lambda k: members[k]["m"])
        for K in KS:
            ms = members[:K]
            big = members[largest] if largest < K else max(ms, key=lambda e: e["m"])

            def bases(which):
                return [ctx.make_device_plan_from_stream(container, S, BITS, e["d_in"], e["m"], size) for e in which]

            def leg_batch(b):
                return ctx.decode_device_indexing_batch([(p, e["d_in"], e["d_out"], INTERVAL, e["m"]) for p, e in zip(b, ms)], stats=stats)

            def leg_singles(b):
                return [ctx.decode_device_indexing(p, e["d_in"], e["d_out"], INTERVAL, stream_length=e["m"]) for p, e in zip(b, ms)]

            def leg_largest(b):
                return [ctx.decode_device_indexing(b[0], big["d_in"], big["d_out"], INTERVAL, stream_length=big["m"])]

            stats = {}
            LEGS = [("batch", leg_batch, ms), ("singles", leg_singles, ms), ("largest", leg_largest, [big])]
            times = {name: [] for name, _, _ in LEGS}
            chains = 0
            for rep in range(args.reps + 1):  # (the first round warms buffers and code objects up and is dropped)
                order = LEGS[rep % len(LEGS):] + LEGS[:rep % len(LEGS)]
                for name, call, which in order:
                    b = bases(which)
                    for e in which:
                        e["d_out"].zero_()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    plans = call(b)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    for e in which:
                        assert torch.equal(e["d_out"], e["d_ref"]), (cname, size, K, name)
                    if name == "batch":
                        chains = sum(H.plan_chain_count(ctx.read_device_plan(p, capacity=1 << 24)) for p in plans[:1]) if rep == 0 else chains
                    for p in plans + b:
                        p.close()
                    if rep:
                        times[name].append(dt * 1e3)
            med = {}
            for name, _, which in LEGS:
                q1, q2, q3 = (float(v) for v in np.percentile(times[name], (25, 50, 75)))
                med[name] = q2
                line = {"container": cname, "members": K, "size": size, "leg": name, "median_ms": round(q2, 4), "q1_ms": round(q1, 4), "q3_ms": round(q3, 4),
                        "iqr_ms": round(q3 - q1, 4), "reps": len(times[name]), "states": S, "bits": BITS, "interval": INTERVAL,
                        "stream_bytes": int(sum(e["m"] for e in which))}
                if name == "batch":
                    line.update({"launches": stats["launches"], "tasks": stats["tasks"], "chains_of_member_0": chains})
                emit(line)
            emit({"container": cname, "members": K, "size": size,
                  "ratios": {"singles_over_batch": round(med["singles"] / med["batch"], 4), "batch_over_largest": round(med["batch"] / med["largest"], 4),
                             "batch_ms_per_member": round(med["batch"] / K, 4), "singles_ms_per_member": round(med["singles"] / K, 4)}})
        del members
        torch.cuda.empty_cache()

emit({"device": ctx.device_name,
      "note": "wall clock around each synchronous call; legs rotated; fresh base plans per leg and repetition (not timed); medians over the repetitions after one dropped round"})
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
