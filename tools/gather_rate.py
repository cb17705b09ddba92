"""hsrans_decode_device_gather against what the library offered for the same request before it, in ONE process on one MI355X:
a 100 MB 64-state 11-bit stream — raw with a checkpoint every 32 groups, and the same data as mt_ in 64 KiB blocks with the same
checkpoints — and random byte ranges of 4 KiB, 64 KiB and 1 MiB that total 1 %, 10 % and 100 % of the decoded bytes, into destinations
that keep the source's alignment modulo 4 ("aligned": the word-store path) or are packed back to back behind an odd base ("packed").
Per case one JSON line with
  gather_us     one gather launch (the task list's copy included), HIP events around --iters calls that rotate over --sets
                (stream, destination) sets — beyond the 256 MB Infinity Cache, as DESIGN.md §8's "rotated"
  full_us       (a) one decode_device of the whole stream, measured the same way
  full_copy_us  (a) ... followed by a device-side copy of the ranges (torch.cat of the ranges' views of the full output)
  slice_us      (b) 1 % cases only: per range plan_slice + make_device_plan + decode_device_ranges of the chains that cover it (the range
                rounded outward to chain boundaries), host clock around all ranges including the final synchronisation
--segments 1024,2048,...: the same gather with other floors of the task length (HSRANS_GATHER_MIN_SEGMENT, read when a device plan is
made) on the 1 % / 4 KiB and 10 % / 64 KiB cases — the table kGatherMinSegment was chosen from.
--indirect: instead of all that, the 1 % / 4 KiB and 10 % / 64 KiB cases through hsrans_decode_device_gather_indirect, beside the host-ranges
entry in the same process.  Per case one JSON line with
  host_us            decode_device_gather as above (ranges in host memory; the parent's path)
  indirect_us        decode_device_gather_indirect with the ranges already on the device (k_gather_cut + k_gather_ranges), measured the same way
  graph_us           the same call captured once per set into a graph, the graphs replayed in rotation
  host_clock_*_us    wall clock per gather for ranges that START on the device, everything waited for: the device-to-host copy of the
                     ranges + synchronisation + decode_device_gather (roundtrip), against the one indirect call (indirect)
Run on the GPU box: python tools/gather_rate.py --out profiles/r10_gather_rate.jsonl --segments 1024,2048,4096,8192,16384
                    python tools/gather_rate.py --indirect --out profiles/r11_gather_indirect_rate.jsonl"""
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
ap.add_argument("--size", type=int, default=100_000_000)
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--iters", type=int, default=24)
ap.add_argument("--segments", default="")
ap.add_argument("--indirect", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
CHAIN = INTERVAL * S
N = args.size
data = synth.enwik8_shaped(N, seed=5)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def event_us(fn, iters):
    """fn(k) queued iters times between two HIP events, after a warm-up round over the sets"""
    for k in range(args.sets):
        fn(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def make_stream(container):
    if container == "raw":
        s, plan = H.encode(H.RAW, S, BITS, data, index_interval=INTERVAL)
    else:
        s, plan = H.encode(H.MT, S, BITS, data, block_size=BLOCK, index_interval=INTERVAL)
    pad = np.concatenate([s, np.zeros((-s.size) % 16, np.uint8)])
    return s.size, plan, [torch.from_numpy(pad).cuda() for _ in range(args.sets)]


def make_ranges(rng, length, fraction, packing):
    count = max(1, int(N * fraction) // length)
    offs = np.sort(rng.integers(0, N - length, count).astype(np.int64))
    if packing == "aligned":
        dst = np.cumsum(np.full(count, length + 4, np.int64)) - (length + 4)
        dst += (offs - dst) % 4
        base = 0
    else:
        dst = np.arange(count, dtype=np.int64) * length
        base = 1  # an odd destination base: no range's destination is word-aligned against its source unless by chance
    ranges = np.stack([offs, np.full(count, length, np.int64), dst], axis=1).astype(np.uint64)
    return ranges, int(dst[-1] + length), base


def check(ranges, d_dst):
    got = d_dst.cpu().numpy()
    for off, length, dst in ranges[:: max(1, len(ranges) // 64)]:
        assert np.array_equal(got[int(dst):int(dst + length)], data[int(off):int(off + length)])


def run_case(container, m, plan, d_streams, dplan, length, fraction, packing, rng, floor=None):
    ranges, size, base = make_ranges(rng, length, fraction, packing)
    backs = [torch.zeros(size + 16, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
    dsts = [b[base:base + size] for b in backs]
    gather = lambda k: ctx.decode_device_gather(dplan, d_streams[k % args.sets], ranges, dsts[k % args.sets], stream_length=m)
    gather_us = event_us(gather, args.iters)
    check(ranges, dsts[0])
    assert ctx.status(dplan) == 0
    rec = {"container": container, "range_bytes": length, "fraction": fraction, "ranges": int(len(ranges)), "dst": packing,
           "tasks": int(H.gather_tasks(N, H.plan_chain_count(plan), S, INTERVAL, ranges).shape[0]) if floor is None else None,
           "gather_us": round(gather_us, 2)}
    if floor is not None:
        rec["min_segment"] = floor
        return rec
    # (a) the whole stream, then a device-side copy of the ranges
    fulls = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
    views = [[f[int(o):int(o + l)] for o, l, _ in ranges] for f in fulls]
    packed = [torch.zeros(int(len(ranges)) * length, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
    full = lambda k: ctx.decode_device(dplan, d_streams[k % args.sets], fulls[k % args.sets], stream_length=m)

    def full_copy(k):
        full(k)
        torch.cat(views[k % args.sets], out=packed[k % args.sets])

    rec["full_us"] = round(event_us(full, args.iters), 2)
    rec["full_copy_us"] = round(event_us(full_copy, max(4, args.iters // 4)), 2)
    rec["gather_over_full_copy"] = round(gather_us / rec["full_copy_us"], 3)
    if fraction <= 0.011:
        # (b) a sliced plan, a device plan and a window launch per range, rounded outward to chain boundaries
        n_chains = H.plan_chain_count(plan)
        todo = ranges[: min(len(ranges), 64)]
        out = fulls[0]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for off, ln, _ in todo:
            c0, c1 = int(off) // CHAIN, min(n_chains, -(-int(off + ln) // CHAIN))
            dp = ctx.make_device_plan(H.plan_slice(plan, c0, c1 - c0))
            o0, o1 = c0 * CHAIN, min(N, c1 * CHAIN)
            ctx.decode_device_ranges(dp, d_streams[0], 0, m, out[o0:o1], o0, o1 - o0)
        torch.cuda.synchronize()
        rec["slice_us"] = round((time.perf_counter() - t0) * 1e6 / len(todo) * len(ranges), 1)
        rec["slice_ranges_timed"] = int(len(todo))
    return rec


def run_indirect_case(container, m, plan, d_streams, dplan, length, fraction, packing, rng):
    ranges, size, base = make_ranges(rng, length, fraction, packing)
    count = int(len(ranges))
    backs = [torch.zeros(size + 16, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
    dsts = [b[base:base + size] for b in backs]
    d_ranges = torch.from_numpy(ranges.view(np.int64)).cuda()
    d_count = torch.tensor(count, dtype=torch.int32, device="cuda")
    spaces = [torch.empty(H.gather_workspace_bytes(count), dtype=torch.uint8, device="cuda") for _ in range(args.sets)]
    host = lambda k: ctx.decode_device_gather(dplan, d_streams[k % args.sets], ranges, dsts[k % args.sets], stream_length=m)
    indirect = lambda k: ctx.decode_device_gather_indirect(dplan, d_streams[k % args.sets], d_ranges, dsts[k % args.sets], count=d_count, workspace=spaces[k % args.sets],
                                                           stream_length=m)
    rec = {"container": container, "range_bytes": length, "fraction": fraction, "ranges": count, "dst": packing,
           "tasks": int(H.gather_tasks(N, H.plan_chain_count(plan), S, INTERVAL, ranges).shape[0])}
    rec["host_us"] = round(event_us(host, args.iters), 2)
    check(ranges, dsts[0])
    for d in dsts:
        d.zero_()
    rec["indirect_us"] = round(event_us(indirect, args.iters), 2)
    check(ranges, dsts[0])
    # one graph per set (its stream, destination and workspace are baked in; the ranges and the count are read at every replay)
    graphs = []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for k in range(args.sets):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                ctx.decode_device_gather_indirect(dplan, d_streams[k], d_ranges, dsts[k], count=d_count, workspace=spaces[k], stream_length=m, stream=side)
        graphs.append(g)
    torch.cuda.synchronize()
    for d in dsts:
        d.zero_()
    rec["graph_us"] = round(event_us(lambda k: graphs[k % args.sets].replay(), args.iters), 2)
    check(ranges, dsts[0])
    assert ctx.status(dplan) == 0
    rec["indirect_over_host"] = round(rec["indirect_us"] / rec["host_us"], 3)
    rec["graph_over_host"] = round(rec["graph_us"] / rec["host_us"], 3)

    # ranges that start on the device, by the host's clock, every gather waited for
    def roundtrip(k):
        ctx.decode_device_gather(dplan, d_streams[k % args.sets], d_ranges.cpu().numpy().view(np.uint64), dsts[k % args.sets], stream_length=m)
        torch.cuda.synchronize()

    def direct(k):
        indirect(k)
        torch.cuda.synchronize()

    for name, fn in (("host_clock_roundtrip_us", roundtrip), ("host_clock_indirect_us", direct)):
        for k in range(args.sets):
            fn(k)
        t0 = time.perf_counter()
        for k in range(args.iters):
            fn(k)
        rec[name] = round((time.perf_counter() - t0) * 1e6 / args.iters, 1)
    return rec


rng = np.random.default_rng(10)
if args.indirect:
    for container in ("raw", "mt_"):
        m, plan, d_streams = make_stream(container)
        dplan = ctx.make_device_plan(plan)
        for length, fraction in ((4096, 0.01), (65536, 0.1)):
            for packing in ("aligned", "packed"):
                emit(run_indirect_case(container, m, plan, d_streams, dplan, length, fraction, packing, np.random.default_rng(length)))
    sys.exit(0)
for container in ("raw", "mt_"):
    m, plan, d_streams = make_stream(container)
    dplan = ctx.make_device_plan(plan)
    for length in (4096, 65536, 1 << 20):
        for fraction in (0.01, 0.1, 1.0):
            for packing in ("aligned", "packed"):
                emit(run_case(container, m, plan, d_streams, dplan, length, fraction, packing, rng))
    for floor in [int(v) for v in args.segments.split(",") if v]:
        os.environ["HSRANS_GATHER_MIN_SEGMENT"] = str(floor)  # (read when the device plan is made)
        dp = ctx.make_device_plan(plan)
        del os.environ["HSRANS_GATHER_MIN_SEGMENT"]
        for length, fraction in ((4096, 0.01), (65536, 0.1)):
            for packing in ("aligned", "packed"):
                emit(run_case(container, m, plan, d_streams, dp, length, fraction, packing, np.random.default_rng(length), floor=floor))
