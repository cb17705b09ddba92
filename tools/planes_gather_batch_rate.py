"""hsrans_decode_device_planes_gather_batch against what a caller had before it, in ONE process on one MI355X: K in {8, 32, 128} Gaussian
bf16 tensors of 2^19 elements and fp32 tensors of 2^18 (1 MiB each), 64 states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, as
frames without and with stored planes, stay compressed in HBM.  Every tensor is read as a table of rows of 1024 elements; 1 % and 10 % of
each tensor's rows, at random row indices, are fetched into one packed destination.  Per configuration, on the same buffers:
  (a) the new call: one hsrans_decode_device_planes_gather_batch over all K tensors' rows;
  (b) today's route: K hsrans_decode_device_planes_gather calls, one per tensor, into the same destination;
  (c) hsrans_decode_device_planes_batch of the whole set, then a device copy of the same rows out of the decoded tensors
      (one torch.index_select over all K tensors into the packed destination);
  (d) hsrans_decode_device_gather_batch of the same gather rows of the coded planes alone, into the call's workspace layout: what the merge
      and its upload add is (a) - (d).
--sets buffer sets (frames, outputs, workspaces) are rotated; HIP events around each leg; median and interquartile range of --reps
repetitions after a warm-up of every set.  *_host_side_us: the host clock around the asynchronous calls alone (the cut of the rows, the
uploads and the launches being queued), the device idle before them.  Every leg's result is compared with the tensors' rows before it is
timed.  Prints one JSON line per configuration and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_gather_batch_rate.py --out profiles/r21_planes_gather_batch_rate.jsonl"""
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
    """fn(set) queues work and returns: microseconds of the host clock around the calls alone, the device idle before them"""
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


def apart(a, b):
    """the faster leg's third quartile below the slower leg's first: the interquartile ranges do not overlap"""
    return a[3] < b[2]


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
        # (c)'s outputs: the K decoded tensors of a set lie in one buffer, so that one copy kernel fetches the rows of all of them
        wholes = [torch.empty(K * n, dtype=INT[W], device="cuda") for _ in range(P)]
        whole_outs = [[w[k * n: (k + 1) * n] for k in range(K)] for w in wholes]
        for store in (False, True):
            frames = [[torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)] for _ in range(P)]
            got = ctx.encode_device_planes_batch(tensors, frames[0], enc_work, states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)
            for i in range(1, P):
                for k in range(K):
                    frames[i][k].copy_(frames[0][k])
            descs, plans = [g[1] for g in got], [g[2] for g in got]
            pset = ctx.make_planes_set(descs, plans)
            pgss = [ctx.make_planes_gather_set(pset, f) for f in frames]
            singles = [ctx.make_planes(descs[k], plans[k]) for k in range(K)]
            pgs = [[ctx.make_planes_gather(singles[k], f[k]) for k in range(K)] for f in frames]
            coded = [(k, p) for k in range(K) for p in range(W) if plans[k][p] is not None]
            gsets = [ctx.make_gather_set([plans[k][p] for k, p in coded], [f[k][descs[k].offset[p]: descs[k].offset[p] + descs[k].length[p]] for k, p in coded])
                     for f in frames] if coded else None
            whole_work = torch.empty(pset.info()["work_bytes"], dtype=torch.uint8, device="cuda")

            for share in args.shares:
                count = max(1, int(table_rows * share))  # rows of each tensor
                rng = np.random.default_rng(1000 * K + int(share * 1000))
                picked = [rng.permutation(table_rows)[:count] for _ in range(K)]
                # (the rows as arrays, made outside the clocks: the calls are given what a caller that cares for the host's time gives them)
                rows = np.asarray([(k, int(r) * ROW, ROW, (k * count + j) * ROW) for k in range(K) for j, r in enumerate(picked[k])], np.uint64)
                per_tensor = [np.ascontiguousarray(rows[rows[:, 0] == k][:, 1:]) for k in range(K)]
                d_picked = torch.from_numpy(np.concatenate([k * table_rows + picked[k] for k in range(K)]).astype(np.int64)).cuda()
                want = torch.cat(tensors).view(K * table_rows, ROW)[d_picked]
                nbytes = K * count * ROW * W
                outs = [torch.zeros(K * count, ROW, dtype=INT[W], device="cuda") for _ in range(P)]
                wb = H.planes_gather_batch_workspace_bytes(W, K * count, K * count * ROW)
                wb1 = H.planes_gather_workspace_bytes(W, count, count * ROW)
                works = [torch.empty(max(wb, K * wb1), dtype=torch.uint8, device="cuda") for _ in range(P)]

                def checked(what):
                    torch.cuda.synchronize()
                    for o in outs:
                        assert torch.equal(o, want), what
                        o.zero_()

                # (a)
                def batch(i):
                    ctx.decode_device_planes_gather_batch(pgss[i], rows, outs[i], works[i])

                for i in range(P):
                    batch(i)
                assert ctx.planes_gather_set_status(pgss[0]) == [0] * K
                checked("the batch call")
                a_new = timed_device(batch)
                a_host = timed_host_side(batch)
                info = pgss[0].info()

                # (b)
                def single_calls(i):
                    for k in range(K):
                        ctx.decode_device_planes_gather(pgs[i][k], per_tensor[k], outs[i].view(-1), works[i][k * wb1: (k + 1) * wb1])

                for o in outs:
                    o.zero_()
                for i in range(P):
                    single_calls(i)
                checked("K single calls")
                b_singles = timed_device(single_calls)
                b_host = timed_host_side(single_calls)
                single_launches = sum(pg.info()["launches"] for pg in pgs[0])

                # (c)
                def whole_then_copy(i):
                    ctx.decode_device_planes_batch(pset, frames[i], whole_outs[i], whole_work)
                    torch.index_select(wholes[i].view(K * table_rows, ROW), 0, d_picked, out=outs[i])

                for o in outs:
                    o.zero_()
                for i in range(P):
                    whole_then_copy(i)
                assert ctx.planes_set_status(pset) == [0] * K
                checked("the whole decode and the copy of the rows")
                c_whole = timed_device(whole_then_copy)

                # (d) the same gather rows of the coded planes alone, into the call's layout (include/hsrans_hip.h): C_r = r * W * ROW, slot ROW
                d_gather = None
                if coded:
                    member_of = {kp: j for j, kp in enumerate(coded)}
                    grows = np.asarray([(member_of[(k, p)], off, ln, r * W * ROW + p * ROW) for r, (k, off, ln, _) in enumerate(rows.tolist()) for p in range(W)
                                        if (k, p) in member_of], np.uint64)
                    assert grows.shape[0] == info["rows"]
                    d_gather = timed_device(lambda i: ctx.decode_device_gather_batch(gsets[i], grows, works[i]))
                    assert ctx.gather_set_status(gsets[0]) == [0] * len(coded)

                emit(dict(tool="tools/planes_gather_batch_rate.py", tensor=f"gaussian {name}", members=K, elements=n, elem_size=W, codec=f"mt_ rANS32x64 16w {BITS}",
                          block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, coded_planes=len(coded), stored_planes=K * W - len(coded),
                          row_elements=ROW, share_of_rows=share, rows_per_tensor=count, rows=K * count, fetched_bytes=nbytes, gather_rows=info["rows"],
                          merge_tasks=info["merge_tasks"], launches=info["launches"], single_calls_launches=single_launches,
                          a_batch_us=a_new, a_host_side_us=a_host, b_single_calls_us=b_singles, b_host_side_us=b_host, c_whole_batch_then_copy_us=c_whole,
                          d_gather_batch_alone_us=d_gather, merge_share_us=None if d_gather is None else round(a_new[0] - d_gather[0], 2),
                          singles_over_batch=round(b_singles[0] / a_new[0], 2), singles_ranges_apart=apart(a_new, b_singles) or apart(b_singles, a_new),
                          whole_over_batch=round(c_whole[0] / a_new[0], 2), a_fetched_GB_s=round(nbytes / a_new[0] / 1e3, 2),
                          us="[median, interquartile range, first quartile, third quartile]", reps=args.reps, sets_rotated=P,
                          checked="every leg's rows == the tensors' rows"))
                del outs, works, want
            for g in gsets or []:
                g.close()
            for row_of_pg in pgs:
                for pg in row_of_pg:
                    pg.close()
            for s in singles:
                s.close()
            for x in pgss:
                x.close()
            pset.close()
            for pl in plans:
                for p in pl:
                    if p is not None:
                        p.close()
            del frames, pgss, pgs, gsets, singles
        del tensors, wholes, whole_outs, enc_work
        torch.cuda.empty_cache()
