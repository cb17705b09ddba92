"""hsrans_decode_device_planes_gather_batch_indirect against the host-rows call, in ONE process on one MI355X.  Tensors, settings and rows are
tools/planes_gather_batch_rate.py's: K in {8, 32, 128} Gaussian bf16 tensors of 2^19 elements and fp32 tensors of 2^18 (1 MiB each), 64
states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, as frames without and with stored planes; every tensor is read as a table of
rows of 1024 elements; 1 % and 10 % of each tensor's rows, at random row indices, are fetched into one packed destination.  Per
configuration, on the same buffers:
  (a) the host-rows call: hsrans_decode_device_planes_gather_batch with the rows in host memory;
  (b) the indirect call: hsrans_decode_device_planes_gather_batch_indirect with the same rows in device memory;
  (c) the indirect call replayed from a graph captured once per buffer set;
  (h) what a caller whose rows are made on the GPU pays in front of (a): the host clock of copying the rows down and synchronising.
--sets buffer sets (frames, outputs, workspaces, rows) are rotated; HIP events around each leg; median and interquartile range of --reps
repetitions after a warm-up of every set.  *_host_side_us: the host clock around the asynchronous calls alone, the device idle before them.
Every leg's result is compared with the tensors' rows before it is timed, and the indirect call's workspace with the host-rows call's.
Prints one JSON line per configuration and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_gather_batch_indirect_rate.py --out profiles/r22_planes_gather_batch_indirect_rate.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--counts", type=int, nargs="+", default=[8, 32, 128])
ap.add_argument("--shares", type=float, nargs="+", default=[0.01, 0.1])
ap.add_argument("--log2-bytes", type=int, default=20, help="bytes of one tensor (20: 1 MiB)")
ap.add_argument("--row-elements", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P, ROW = args.sets, args.row_elements
INT = {2: torch.int16, 4: torch.int32}


def spread(ms):
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return [round(float(med) * 1e3, 2), round(float(q3 - q1) * 1e3, 2), round(float(q1) * 1e3, 2), round(float(q3) * 1e3, 2)]  # microseconds


def timed_device(fn):
    """fn(set) queues work on the current stream: microseconds between two events around it"""
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
    """fn(set) runs on the host: microseconds of the host clock around it, the device idle before it"""
    ms = []
    for r in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r % P)
        ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return spread(ms)


def gaussian(name, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
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
    table_rows = n // ROW
    assert n == table_rows * ROW, "a tensor is a whole number of rows"
    for K in args.counts:
        tensors = [gaussian(name, n, 41 + k) for k in range(K)]  # K different tensors
        cap = H.planes_capacity(W, S, n)
        enc_work = torch.empty(H.planes_batch_workspace_bytes([W] * K, [n] * K), dtype=torch.uint8, device="cuda")
        for store in (False, True):
            frames = [[torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)] for _ in range(P)]
            got = ctx.encode_device_planes_batch(tensors, frames[0], enc_work, states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)
            for i in range(1, P):
                for k in range(K):
                    frames[i][k].copy_(frames[0][k])
            descs, plans = [g[1] for g in got], [g[2] for g in got]
            pset = ctx.make_planes_set(descs, plans)
            pgss = [ctx.make_planes_gather_set(pset, f) for f in frames]
            n_coded = sum(p is not None for pl in plans for p in pl)

            for share in args.shares:
                count = max(1, int(table_rows * share))  # rows of each tensor
                rng = np.random.default_rng(1000 * K + int(share * 1000))
                picked = [rng.permutation(table_rows)[:count] for _ in range(K)]
                rows = np.asarray([(k, int(r) * ROW, ROW, (k * count + j) * ROW) for k in range(K) for j, r in enumerate(picked[k])], np.uint64)
                d_picked = torch.from_numpy(np.concatenate([k * table_rows + picked[k] for k in range(K)]).astype(np.int64)).cuda()
                want = torch.cat(tensors).view(K * table_rows, ROW)[d_picked]
                N = K * count
                nbytes = N * ROW * W
                outs = [torch.zeros(N, ROW, dtype=INT[W], device="cuda") for _ in range(P)]
                wb = H.planes_gather_batch_workspace_bytes(W, N, N * ROW)
                works = [torch.zeros(wb, dtype=torch.uint8, device="cuda") for _ in range(P)]
                # the rows in device memory, in hsrans_member_range's layout: (offset, length, dst_offset, member)
                d_rows = [torch.from_numpy(np.ascontiguousarray(rows[:, [1, 2, 3, 0]]).view(np.int64)).cuda() for _ in range(P)]
                control = [torch.empty(H.planes_gather_batch_indirect_workspace_bytes(n_coded, W, N), dtype=torch.uint8, device="cuda") for _ in range(P)]

                def checked(what):
                    torch.cuda.synchronize()
                    for o in outs:
                        assert torch.equal(o, want), what
                        o.zero_()

                # (a)
                def host_rows(i):
                    ctx.decode_device_planes_gather_batch(pgss[i], rows, outs[i], works[i])

                for i in range(P):
                    host_rows(i)
                assert ctx.planes_gather_set_status(pgss[0]) == [0] * K
                checked("the host-rows call")
                host_works = [w.clone() for w in works]
                a_host_rows = timed_device(host_rows)
                a_host = timed_host_side(host_rows)
                info = pgss[0].info()

                # (h) the rows are on the GPU: copy them down and wait for them
                def copy_down(i):
                    d_rows[i].cpu()
                    torch.cuda.synchronize()

                h_copy = timed_host_side(copy_down)

                # (b)
                def indirect(i):
                    ctx.decode_device_planes_gather_batch_indirect(pgss[i], d_rows[i], outs[i], works[i], workspace=control[i])

                for o, w in zip(outs, works):
                    o.zero_()
                    w.zero_()
                for i in range(P):
                    indirect(i)
                assert all(ctx.planes_gather_set_refused(x) == 0 for x in pgss) and ctx.planes_gather_set_status(pgss[0]) == [0] * K
                assert all(torch.equal(w, hw) for w, hw in zip(works, host_works)), "the indirect call's workspace"
                checked("the indirect call")
                b_indirect = timed_device(indirect)
                b_host = timed_host_side(indirect)
                shape = pgss[0].indirect_info(N, nbytes, wb)

                # (c) one graph per buffer set, captured once
                graphs = []
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for i in range(P):
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g, stream=side):
                            ctx.decode_device_planes_gather_batch_indirect(pgss[i], d_rows[i], outs[i], works[i], workspace=control[i], stream=side)
                        graphs.append(g)
                torch.cuda.synchronize()
                for g in graphs:
                    g.replay()
                assert all(ctx.planes_gather_set_refused(x) == 0 for x in pgss)
                checked("the replayed graph")
                c_graph = timed_device(lambda i: graphs[i].replay())
                c_host = timed_host_side(lambda i: graphs[i].replay())
                del graphs

                emit(dict(tool="tools/planes_gather_batch_indirect_rate.py", tensor=f"gaussian {name}", members=K, elements=n, elem_size=W,
                          codec=f"mt_ rANS32x64 16w {BITS}", block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, coded_planes=n_coded,
                          stored_planes=K * W - n_coded, row_elements=ROW, share_of_rows=share, rows_per_tensor=count, rows=N, fetched_bytes=nbytes,
                          gather_rows=info["rows"], merge_tasks=info["merge_tasks"], host_rows_launches=info["launches"], indirect_launches=shape["launches"],
                          indirect_set_launches=shape["set_launches"], indirect_merge_grid=shape["merge_grid"],
                          a_host_rows_us=a_host_rows, a_host_side_us=a_host, h_copy_down_and_sync_host_us=h_copy, b_indirect_us=b_indirect, b_host_side_us=b_host,
                          c_graph_replay_us=c_graph, c_host_side_us=c_host,
                          indirect_minus_host_rows_us=round(b_indirect[0] - a_host_rows[0], 2), graph_minus_host_rows_us=round(c_graph[0] - a_host_rows[0], 2),
                          host_rows_plus_copy_down_us=round(a_host_rows[0] + h_copy[0], 2),
                          # the indirect call's third quartile below the sum of the first quartiles of what it replaces
                          indirect_below_host_rows_plus_copy_down_ranges_apart=b_indirect[3] < a_host_rows[2] + h_copy[2],
                          graph_below_host_rows_plus_copy_down_ranges_apart=c_graph[3] < a_host_rows[2] + h_copy[2],
                          indirect_below_host_rows_ranges_apart=b_indirect[3] < a_host_rows[2], host_rows_below_indirect_ranges_apart=a_host_rows[3] < b_indirect[2],
                          us="[median, interquartile range, first quartile, third quartile]", reps=args.reps, sets_rotated=P,
                          checked="every leg's rows == the tensors' rows; the indirect call's workspace == the host-rows call's"))
                del outs, works, want, host_works, d_rows, control
            for x in pgss:
                x.close()
            pset.close()
            for pl in plans:
                for p in pl:
                    if p is not None:
                        p.close()
            del frames, pgss
        del tensors, enc_work
        torch.cuda.empty_cache()
