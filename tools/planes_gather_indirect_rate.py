"""hsrans_decode_device_planes_gather_indirect against hsrans_decode_device_planes_gather, in ONE process on one MI355X, with the tensors,
settings and rows of tools/planes_gather_rate.py: the Gaussian bf16 (2^26 elements) and fp32 (2^25) tensors (128 MiB each, 64 states, 11 bits,
64 KiB blocks, a checkpoint every 32 groups), as frames without and with stored planes, stay compressed in HBM; 1 % and 10 % of the table's
rows of 4096 elements, at random row indices, are fetched into a packed destination.  Per configuration, HIP events around each leg:
  host      hsrans_decode_device_planes_gather, the ranges in host memory (the yardstick: the entry as the parent commit has it);
  indirect  hsrans_decode_device_planes_gather_indirect, the same ranges in device memory, count word included;
  graph     the same indirect call captured once per buffer set and replayed.
Beside them, on the same ranges:
  floor         the indirect call with as many EMPTY ranges: both single-workgroup cuts (k_planes_cut, the set's k_set_cut) run over the rows,
                every launch behind them finds nothing to do — what the line of kernels costs before a byte moves;
  cut           the same on a frame whose planes are ALL stored (the split tensor): k_planes_cut and an idle merge launch, no set;
  merge         that all-stored frame with the real ranges, through both entries: indirect = k_planes_cut + k_planes_merge_indirect (the
                merge finds its tasks in the cut's prefix), host = the task list's upload + k_planes_merge_ranges on the same tasks;
  d2h_sync      the host clock around copying the ranges down and synchronising — what a caller whose ranges are made on the device pays
                in front of the host-ranges call and the indirect entry removes; charged to no leg.
--sets buffer sets are rotated; median and interquartile range of --reps repetitions after a warm-up of every set.  *_host_side_us: the host
clock around the asynchronous call alone, the device idle before it.  Every leg's output is compared with the tensor's rows before anything
is timed.  Prints one JSON line per configuration and appends it to --out.  Nothing is gated.
Run on the GPU box: python tools/planes_gather_indirect_rate.py --out profiles/r19_planes_gather_indirect_rate.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--log2-bytes", type=int, default=27, help="tensor size (27: 128 MiB)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P = args.sets
INT = {2: torch.int16, 4: torch.int32}
ROW = 4096


def up(v, a):
    return (v + a - 1) // a * a


def spread(ms):
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return round(float(med) * 1e3, 2), round(float(q3 - q1) * 1e3, 2)  # microseconds


def timed_device(fn):
    """fn(set) queues work on the current stream: (median, IQR) in microseconds between two events around it"""
    for i in range(P):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for r in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r % P)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return spread(ms)


def timed_host_side(fn):
    """(median, IQR) in microseconds of the host clock around fn(set) alone, the device idle before it"""
    ms = []
    for r in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r % P)
        ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return spread(ms)


def gaussian(name, n):
    g = torch.Generator(device="cuda").manual_seed(41)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    if name == "fp32":
        return x.view(torch.int32)
    return (x.view(torch.int32) >> 16).to(torch.int16)  # truncated to bf16


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    tensor = gaussian(name, n)
    enc_work = torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
    # the all-stored frame: the split tensor
    stride_all = up(n, 256)
    ctx.planes_split_device(tensor, [enc_work[p * stride_all: p * stride_all + n] for p in range(W)])
    raw_desc = api.PlanesDesc()
    raw_desc.elem_size, raw_desc.states, raw_desc.bits, raw_desc.block_size, raw_desc.index_interval = W, S, BITS, BLOCK, INTERVAL
    raw_desc.stored_mask, raw_desc.elements = (1 << W) - 1, n
    for p in range(W):
        raw_desc.offset[p], raw_desc.length[p] = p * stride_all, n
    raw_desc.frame_length = (W - 1) * stride_all + n
    raw_frames = [enc_work.clone() for _ in range(P)]
    raw_planes = ctx.make_planes(raw_desc, [None] * W)
    raw_pgs = [ctx.make_planes_gather(raw_planes, f) for f in raw_frames]

    for store in (False, True):
        frame0 = torch.empty(H.planes_capacity(W, S, n), dtype=torch.uint8, device="cuda")
        total, desc, plans = ctx.encode_device_planes(tensor, frame0, enc_work, states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)
        frames = [frame0] + [frame0.clone() for _ in range(P - 1)]
        planes = ctx.make_planes(desc, plans)
        pgs = [ctx.make_planes_gather(planes, f) for f in frames]
        coded = [p for p in range(W) if plans[p] is not None]

        for share in (0.01, 0.1):
            table_rows = n // ROW
            table = tensor[: table_rows * ROW].view(table_rows, ROW)
            count = max(1, int(table_rows * share))
            picked = np.random.default_rng(1000 * ROW + int(share * 1000)).permutation(table_rows)[:count]
            ranges = np.stack([picked * ROW, np.full(count, ROW), np.arange(count) * ROW], axis=1).astype(np.uint64)
            empty = ranges.copy()
            empty[:, 1] = 0
            want = table[torch.from_numpy(picked.astype(np.int64)).cuda()]
            max_elements = count * ROW
            flats = [torch.zeros(count * ROW, dtype=INT[W], device="cuda") for _ in range(P)]
            outs = [f.view(count, ROW) for f in flats]
            works = [torch.empty(H.planes_gather_workspace_bytes(W, count, max_elements), dtype=torch.uint8, device="cuda") for _ in range(P)]
            controls = [torch.empty(H.planes_gather_indirect_workspace_bytes(W, count), dtype=torch.uint8, device="cuda") for _ in range(P)]
            d_ranges = [torch.from_numpy(ranges.view(np.int64)).cuda() for _ in range(P)]
            d_empty = [torch.from_numpy(empty.view(np.int64)).cuda() for _ in range(P)]
            d_counts = [torch.full((1,), count, dtype=torch.int32, device="cuda") for _ in range(P)]

            def checked(what):
                torch.cuda.synchronize()
                for o in outs:
                    assert torch.equal(o, want), what
                    o.zero_()

            def untouched(what):
                torch.cuda.synchronize()
                for o in outs:
                    assert not bool(o.any()), what

            def host(i, objs=pgs):
                ctx.decode_device_planes_gather(objs[i], ranges, flats[i], works[i])

            def indirect(i, objs=pgs, rows=d_ranges):
                ctx.decode_device_planes_gather_indirect(objs[i], rows[i], flats[i], works[i], count=d_counts[i], max_count=count, max_elements=max_elements,
                                                         workspace=controls[i])

            # the three legs
            t_host = timed_device(host)
            t_host_side = timed_host_side(host)
            checked("the host-ranges call")
            t_ind = timed_device(indirect)
            t_ind_side = timed_host_side(indirect)
            assert ctx.planes_gather_refused(pgs[0]) == 0 and ctx.planes_gather_status(pgs[0]) == [0] * W
            checked("the indirect call")
            graphs = []
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            for i in range(P):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.stream(side):
                    with torch.cuda.graph(g, stream=side):
                        ctx.decode_device_planes_gather_indirect(pgs[i], d_ranges[i], flats[i], works[i], count=d_counts[i], max_count=count, max_elements=max_elements,
                                                                 workspace=controls[i], stream=side)
                graphs.append(g)
            torch.cuda.synchronize()
            untouched("capturing runs nothing")
            t_graph = timed_device(lambda i: graphs[i].replay())
            t_graph_side = timed_host_side(lambda i: graphs[i].replay())
            assert ctx.planes_gather_refused(pgs[0]) == 0
            checked("the replayed graph")
            del graphs
            # beside them
            t_floor = timed_device(lambda i: indirect(i, rows=d_empty))
            untouched("empty ranges write nothing")
            t_cut = timed_device(lambda i: indirect(i, objs=raw_pgs, rows=d_empty))
            untouched("empty ranges write nothing (all planes stored)")
            t_merge_ind = timed_device(lambda i: indirect(i, objs=raw_pgs))
            checked("cut and merge, all planes stored")
            t_merge_host = timed_device(lambda i: host(i, objs=raw_pgs))
            checked("upload and merge, all planes stored")

            def d2h(i):
                d_ranges[i].cpu()
                d_counts[i].cpu()
                torch.cuda.synchronize()

            t_d2h = timed_host_side(d2h)
            info = pgs[0].indirect_info(count, max_elements, flats[0].numel() * W)
            nbytes = count * ROW * W
            emit(dict(tool="tools/planes_gather_indirect_rate.py", tensor=f"gaussian {name}", elements=n, elem_size=W, bytes=n * W, codec=f"mt_ rANS32x64 16w {BITS}",
                      block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, stored_mask=int(desc.stored_mask), coded_planes=len(coded),
                      row_elements=ROW, share_of_rows=share, ranges=count, fetched_bytes=nbytes, max_rows=info["max_rows"], merge_grid=info["merge_grid"],
                      launches=info["launches"], set_launches=info["set_launches"],
                      host_ranges_us=t_host, host_ranges_host_side_us=t_host_side, indirect_us=t_ind, indirect_host_side_us=t_ind_side, graph_replay_us=t_graph,
                      graph_replay_host_side_us=t_graph_side, indirect_over_host=round(t_ind[0] / t_host[0], 3), graph_over_host=round(t_graph[0] / t_host[0], 3),
                      floor_empty_ranges_us=t_floor, cut_and_idle_merge_all_stored_us=t_cut, merge_all_stored_indirect_us=t_merge_ind,
                      merge_all_stored_host_ranges_us=t_merge_host, d2h_copy_and_sync_host_clock_us=t_d2h,
                      us="[median, interquartile range]", reps=args.reps, sets_rotated=P, checked="every leg's rows == tensor[rows]"))
            del outs, flats, works, controls, want
        for pg in pgs:
            pg.close()
        planes.close()
        for p in plans:
            if p is not None:
                p.close()
        del frames, frame0, pgs
    for pg in raw_pgs:
        pg.close()
    raw_planes.close()
    del raw_frames, enc_work, tensor
    torch.cuda.empty_cache()
