"""The byte-plane layer over many tensors: K in {8, 32, 128} Gaussian bf16 tensors of 2^19 elements and fp32 tensors of 2^18 (1 MiB each),
64 states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, with and without stored planes.  Per case:
  (a) hsrans_encode_device_planes_batch against K hsrans_encode_device_planes calls on the same buffers (host clock: both synchronise);
  (b) hsrans_decode_device_planes_batch against K hsrans_decode_device_planes calls (device events around all K);
  (c) the batch decode against hsrans_decode_device_batch of the same plans alone: the merge launch and its table upload;
  (d) the batch encode without plans: what the codec batch spends on making the planes' device plans.
--sets buffer sets (tensors, frames, workspaces, outputs) are rotated.  Median and interquartile range over --reps repetitions after a
warm-up of every set.  Every member's frame is compared with its single call's and the set is decoded back to the tensors before anything
is timed.  Prints one JSON line per case and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_batch_rate.py --out profiles/r20_planes_batch_rate.jsonl"""
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
ap.add_argument("--log2-bytes", type=int, default=20, help="bytes of one tensor (20: 1 MiB)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P = args.sets


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


def timed_host(fn):
    """fn(set) returns with its work done: microseconds on the host clock"""
    for i in range(P):
        fn(i)
    ms = []
    for r in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r % P)
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def gaussian(name, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    if name == "fp32":
        return x
    return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)  # truncated


def close(plans):
    for p in plans:
        if p is not None:
            p.close()


def apart(a, b):
    """the faster leg's third quartile below the slower leg's first: the interquartile ranges do not overlap"""
    return a[3] < b[2]


for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    for K in args.counts:
        first = [gaussian(name, n, 41 + k) for k in range(K)]  # K different tensors
        tensors = [first] + [[t.clone() for t in first] for _ in range(P - 1)]
        cap, wb1 = H.planes_capacity(W, S, n), H.planes_workspace_bytes(W, n)
        wb = H.planes_batch_workspace_bytes([W] * K, [n] * K)
        frames = [[torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)] for _ in range(P)]
        works = [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(P)]
        outs = [[torch.empty_like(t) for t in first] for _ in range(P)]
        for store in (False, True):
            kw = dict(states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)

            # ---- (a) the encoders ----
            def enc_batch(i, keep=False, want_plans=True):
                stats = {}
                r = ctx.encode_device_planes_batch(tensors[i], frames[i], works[i], stats=stats, want_plans=want_plans, **kw)
                if keep:
                    return r, stats
                for g in r:
                    close(g[2])

            def enc_singles(i, keep=False):
                r = [ctx.encode_device_planes(tensors[i][k], frames[i][k], works[i][k * wb1: (k + 1) * wb1], **kw) for k in range(K)]
                if keep:
                    return r
                for g in r:
                    close(g[2])

            a_singles = timed_host(enc_singles)
            want = enc_singles(0, keep=True)
            want_frames = [f.clone() for f in frames[0]]
            for f in frames[0]:
                f.zero_()
            a_batch = timed_host(enc_batch)
            a_batch_no_plans = timed_host(lambda i: enc_batch(i, want_plans=False))  # (the codec batch makes and reads back every plan: its share)
            got, stats = enc_batch(0, keep=True)
            for k in range(K):  # every member is its single call
                assert got[k][0] == want[k][0] and bytes(got[k][1]) == bytes(want[k][1]), k
                for p in range(W):
                    lo, hi = got[k][1].offset[p], got[k][1].offset[p] + got[k][1].length[p]
                    assert torch.equal(frames[0][k][lo:hi], want_frames[k][lo:hi]), (k, p)
                close(want[k][2])
            for i in range(1, P):
                for k in range(K):
                    frames[i][k].copy_(frames[0][k])

            # ---- (b) the decoders: the set, and K planes objects ----
            pset = ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
            info = pset.info()
            b_batch = timed_device(lambda i: ctx.decode_device_planes_batch(pset, frames[i], outs[i], works[i]))
            assert ctx.planes_set_status(pset) == [0] * K
            for i in range(P):
                for k in range(K):
                    assert torch.equal(outs[i][k].view(torch.uint8), tensors[i][k].view(torch.uint8)), "the set does not decode to the tensors"
                    outs[i][k].zero_()
            pset.close()
            singles = [ctx.make_planes(g[1], g[2]) for g in got]
            single_launches = sum(s.info()["launches"] for s in singles)

            def dec_singles(i):
                for k in range(K):
                    ctx.decode_device_planes(singles[k], frames[i][k], outs[i][k], works[i][k * wb1: (k + 1) * wb1])

            b_singles = timed_device(dec_singles)
            for k in range(K):
                assert ctx.planes_status(singles[k]) == [0] * W
                assert torch.equal(outs[0][k].view(torch.uint8), tensors[0][k].view(torch.uint8))
                singles[k].close()

            # ---- (c) the codec batch of the same plans alone, into the same workspace regions ----
            coded = [(k, p) for k in range(K) for p in range(W) if got[k][2][p] is not None]
            stride = wb1 // W
            batch = ctx.make_batch([got[k][2][p] for k, p in coded])
            streams = [[frames[i][k][got[k][1].offset[p]: got[k][1].offset[p] + got[k][1].length[p]] for k, p in coded] for i in range(P)]  # (sliced outside the clock)
            regions = [[works[i][k * wb1 + p * stride: k * wb1 + p * stride + n] for k, p in coded] for i in range(P)]
            c_batch = timed_device(lambda i: ctx.decode_device_batch(batch, streams[i], regions[i]))
            assert ctx.batch_status(batch) == [0] * len(coded)
            batch.close()
            for g in got:
                close(g[2])

            row = dict(tool="tools/planes_batch_rate.py", tensor=f"gaussian {name}", members=K, elements=n, elem_size=W, bytes=K * n * W, codec=f"mt_ rANS32x64 16w {BITS}",
                       block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, stored_planes=stats["stored"], coded_planes=info["coded"],
                       encode_launches=stats["launches"], decode_launches=info["launches"], single_decode_launches=single_launches, merge_tasks=info["merge_tasks"],
                       a_encode_batch_us=a_batch, a_encode_batch_without_plans_us=a_batch_no_plans, a_encode_singles_us=a_singles, encode_singles_over_batch=round(a_singles[0] / a_batch[0], 2),
                       encode_ranges_apart=apart(a_batch, a_singles),
                       b_decode_batch_us=b_batch, b_decode_singles_us=b_singles, decode_singles_over_batch=round(b_singles[0] / b_batch[0], 2),
                       decode_ranges_apart=apart(b_batch, b_singles),
                       c_codec_batch_alone_us=c_batch, merge_share_us=round(b_batch[0] - c_batch[0], 2), decode_batch_over_codec_batch=round(b_batch[0] / c_batch[0], 2),
                       encode_batch_GB_s=round(K * n * W / a_batch[0] / 1e3, 2), decode_batch_GB_s=round(K * n * W / b_batch[0] / 1e3, 1),
                       us="[median, interquartile range, first quartile, third quartile]", reps=args.reps, sets_rotated=P,
                       checked="every member's frame and descriptor equal its single call's; the set decoded back to the tensors")
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        del tensors, frames, works, outs, first
        torch.cuda.empty_cache()
