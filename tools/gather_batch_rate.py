"""hsrans_decode_device_gather_batch against what the library offered for the same request before it — one hsrans_decode_device_gather
per stream — in ONE process on one MI355X: K streams of 1 MB each (raw, 64 states, 11 bits, a checkpoint every 32 groups; and the same
data as mt_ in 64 KiB blocks with the same checkpoints) stay compressed in HBM, and 1 % / 10 % of every stream is fetched in 4 KiB ranges,
packed back to back into one destination.  Both legs use the same device plans and the same ranges; the measurements rotate over --sets
(streams, destination) sets, as tools/gather_rate.py's do, and alternate between the legs repetition by repetition.
Per case one JSON line with
  single_us        K decode_device_gather calls, HIP events around the K calls; the median of --reps repetitions after --warmup
  batch_us         one decode_device_gather_batch call, measured the same way
  single_spread_us / batch_spread_us   the interquartile range of the repetitions: the run-to-run spread of each leg
  batch_over_single   the ratio of the medians;  launches: what the batch call queued
Run on the GPU box: python tools/gather_batch_rate.py --out profiles/r12_gather_batch_rate.jsonl
--indirect: the same rows with three other legs — the host-ranges batch call (the yardstick), hsrans_decode_device_gather_batch_indirect
with the ranges already in device memory, and that call captured once and replayed from a graph — rotated leg by leg within a repetition
(the starting leg moves on by one every repetition).  Per case one JSON line with batch_us / indirect_us / graph_us (medians), the three
*_spread_us (interquartile ranges), indirect_over_batch and graph_over_batch.  What the host-ranges leg pays and the others do not: the
cut on the CPU and the upload of the task lists; what it is spared: the device-side cut and the table reloads of a workgroup that serves
several members.  python tools/gather_batch_rate.py --indirect --out profiles/r13_gather_batch_indirect_rate.jsonl"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1_000_000)
ap.add_argument("--streams", default="8,32,128")
ap.add_argument("--sets", type=int, default=4)
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--indirect", action="store_true")
args = ap.parse_args()
assert args.reps >= 20 and args.warmup >= 5
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL, RANGE = 64, 11, 1 << 16, 32, 4096
N = args.size
BASE = synth.enwik8_shaped(N, seed=5)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def timed(fn):
    """fn() between two HIP events, microseconds"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def make_streams(container, K):
    datas, lengths, plans = [], [], []
    sets = [[] for _ in range(args.sets)]
    for k in range(K):
        d = BASE ^ np.uint8(k & 0xFF)  # (every stream other bytes, the same statistics)
        if container == "raw":
            s, plan = H.encode(H.RAW, S, BITS, d, index_interval=INTERVAL)
        else:
            s, plan = H.encode(H.MT, S, BITS, d, block_size=BLOCK, index_interval=INTERVAL)
        pad = np.concatenate([s, np.zeros((-s.size) % 16, np.uint8)])
        datas.append(d)
        lengths.append(s.size)
        plans.append(ctx.make_device_plan(plan))
        for q in range(args.sets):
            sets[q].append(torch.from_numpy(pad).cuda())
    # one gather set per rotation set: the members are the same plans over that set's copies of the streams
    gsets = [ctx.make_gather_set(plans, sets[q], lengths) for q in range(args.sets)]
    return datas, lengths, plans, sets, gsets


def run_case(container, K, fraction, datas, lengths, plans, sets, gsets):
    rng = np.random.default_rng(1000 * K + int(fraction * 100))
    per = max(1, int(N * fraction) // RANGE)
    rows, pos = [], 0
    for k in range(K):
        for off in np.sort(rng.integers(0, N - RANGE, per)).tolist():
            rows.append((k, off, RANGE, pos))
            pos += RANGE
    ranges = np.array(rows, np.uint64)
    by_member = [np.ascontiguousarray(ranges[ranges[:, 0] == k][:, 1:]) for k in range(K)]
    dsts = [torch.zeros(pos, dtype=torch.uint8, device="cuda") for _ in range(args.sets)]

    def single(q):
        for k in range(K):
            ctx.decode_device_gather(plans[k], sets[q][k], by_member[k], dsts[q], stream_length=lengths[k])

    def batch(q):
        ctx.decode_device_gather_batch(gsets[q], ranges, dsts[q])

    def check(q):
        got = dsts[q].cpu().numpy()
        for k, off, length, dst in ranges[:: max(1, len(ranges) // 97)].tolist():
            assert np.array_equal(got[dst:dst + length], datas[k][off:off + length])
        dsts[q].zero_()

    single(0)
    torch.cuda.synchronize()
    check(0)
    batch(0)
    torch.cuda.synchronize()
    check(0)
    assert ctx.gather_set_status(gsets[0]) == [0] * K
    if args.indirect:
        return run_indirect(container, K, fraction, ranges, pos, dsts, gsets, batch, check)
    t_single, t_batch = [], []
    for r in range(args.warmup + args.reps):
        q = r % args.sets
        a, b = timed(lambda: single(q)), timed(lambda: batch(q))
        if r >= args.warmup:
            t_single.append(a)
            t_batch.append(b)
    iqr = lambda t: float(np.percentile(t, 75) - np.percentile(t, 25))
    info = gsets[0].info()
    rec = {"container": container, "streams": K, "stream_bytes": N, "fraction": fraction, "range_bytes": RANGE, "ranges": int(len(ranges)),
           "tasks": int(sum(info["kind_tasks"])), "launches": info["launches"], "reps": args.reps, "sets": args.sets,
           "single_us": round(float(np.median(t_single)), 2), "batch_us": round(float(np.median(t_batch)), 2),
           "single_spread_us": round(iqr(t_single), 2), "batch_spread_us": round(iqr(t_batch), 2),
           "single_min_us": round(min(t_single), 2), "batch_min_us": round(min(t_batch), 2)}
    rec["batch_over_single"] = round(rec["batch_us"] / rec["single_us"], 4)
    rec["batch_not_slower"] = bool(rec["batch_us"] <= rec["single_us"] + rec["single_spread_us"])
    return rec


def run_indirect(container, K, fraction, ranges, size, dsts, gsets, batch, check):
    """the three legs of --indirect over the rows `ranges` (member, offset, length, dst_offset)"""
    rows = np.stack([ranges[:, 1], ranges[:, 2], ranges[:, 3], ranges[:, 0]], axis=1).astype(np.int64)
    d_rows = [torch.from_numpy(rows).cuda() for _ in range(args.sets)]
    d_count = torch.tensor(len(rows), dtype=torch.int32, device="cuda")
    workspaces = [torch.empty(H.gather_batch_workspace_bytes(K, len(rows)), dtype=torch.uint8, device="cuda") for _ in range(args.sets)]

    def indirect(q):
        ctx.decode_device_gather_batch_indirect(gsets[q], d_rows[q], dsts[q], count=d_count, workspace=workspaces[q])

    graphs = []
    side = torch.cuda.Stream()
    for q in range(args.sets):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                ctx.decode_device_gather_batch_indirect(gsets[q], d_rows[q], dsts[q], count=d_count, workspace=workspaces[q], stream=side)
        graphs.append(g)
    torch.cuda.synchronize()
    for leg in (indirect, lambda q: graphs[q].replay()):
        leg(0)
        torch.cuda.synchronize()
        check(0)
    assert ctx.gather_set_status(gsets[0]) == [0] * K and ctx.gather_set_refused(gsets[0]) == 0
    legs = (("batch", batch), ("indirect", indirect), ("graph", lambda q: graphs[q].replay()))
    times = {name: [] for name, _ in legs}
    for r in range(args.warmup + args.reps):
        q = r % args.sets
        for j in range(3):
            name, fn = legs[(r + j) % 3]
            t = timed(lambda: fn(q))
            if r >= args.warmup:
                times[name].append(t)
    iqr = lambda t: float(np.percentile(t, 75) - np.percentile(t, 25))
    batch(0)
    torch.cuda.synchronize()
    host, info = gsets[0].info(), gsets[0].indirect_info(len(rows), size)
    rec = {"container": container, "streams": K, "stream_bytes": N, "fraction": fraction, "range_bytes": RANGE, "ranges": int(len(rows)),
           "tasks": int(sum(host["kind_tasks"])), "launches": info["launches"], "grid": info["kind_grid"], "waves": info["kind_waves"], "reps": args.reps,
           "sets": args.sets}
    for name, _ in legs:
        rec[name + "_us"] = round(float(np.median(times[name])), 2)
        rec[name + "_spread_us"] = round(iqr(times[name]), 2)
        rec[name + "_min_us"] = round(min(times[name]), 2)
    rec["indirect_over_batch"] = round(rec["indirect_us"] / rec["batch_us"], 4)
    rec["graph_over_batch"] = round(rec["graph_us"] / rec["batch_us"], 4)
    return rec


for container in ("raw", "mt_"):
    for K in [int(v) for v in args.streams.split(",") if v]:
        made = make_streams(container, K)
        for fraction in (0.01, 0.1):
            emit(run_case(container, K, fraction, *made))
        del made
