"""hsrans_decode_device_planes_gather against what a caller had before it, in ONE process on one MI355X: the Gaussian bf16 (2^26 elements)
and fp32 (2^25) tensors of tools/planes_rate.py with its settings (128 MiB each, 64 states, 11 bits, 64 KiB blocks, a checkpoint every 32
groups), as frames without and with stored planes, stay compressed in HBM.  The tensor is read as a table of rows; a share of the rows, at
random row indices, is fetched into a packed destination: rows of 4096 elements (aligned to the source's 16-element grid, 16-byte aligned
destinations) for 1 % and 10 % of the rows — and for --more-shares, to bracket the crossover — and two legs with rows of 1000 elements for
1 %: packed from element 0 (the rows start at phase 0 or 8 of the grid, so half of them have byte-wise heads and tails of 8 elements; the
whole blocks' output addresses are still 16-byte aligned) and packed from element 1 (every output address only element-aligned: the
element-wide store path throughout).  Per configuration, from the same process:
  (a) the new call;
  (b) what a caller does today: hsrans_decode_device_planes of the whole frame, then a device copy of the same rows out of the decoded
      tensor (torch.index_select into the packed destination);
  (c) hsrans_decode_device_gather_batch of the same rows of the coded planes alone, into the call's workspace layout;
  (d) the merge launch alone — the new call on a frame whose planes are ALL stored (the split tensor), which is its task upload and its one
      launch — against a hipMemcpyAsync device-to-device of the same number of bytes.
--sets buffer sets (frame, outputs, workspaces) are rotated; HIP events around each leg; median and interquartile range of --reps
repetitions after a warm-up of every set.  a_host_side_us / d_merge_host_side_us: the host clock around the asynchronous call alone (the cut of
the ranges, the uploads and the launches being queued) — the device waits for that much of a call that finds it idle.  Every leg's result is
compared with the tensor's rows before anything is timed.
crossover_share: the share of rows at which (b) starts to win, interpolated between the two measured shares that bracket it (null when (a)
wins or loses at every share measured).  Prints one JSON line per configuration and appends it to --out.  Nothing is gated.
Run on the GPU box: python tools/planes_gather_rate.py --out profiles/r18_planes_gather_rate.jsonl"""
import argparse
import ctypes
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
ap.add_argument("--more-shares", default="0.3,0.6", help="shares of 4096-element rows measured besides 1 % and 10 %")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch loaded)
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P = args.sets
INT = {2: torch.int16, 4: torch.int32}


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
    """fn(set) queues work and returns: (median, IQR) in microseconds of the host clock around the call alone, the device idle before it"""
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


def crossover(points):
    """points: [(share, a_us, b_us)] by share; the share at which a - b changes sign, linear between the two points around it"""
    for (f0, a0, b0), (f1, a1, b1) in zip(points, points[1:]):
        d0, d1 = a0 - b0, a1 - b1
        if d0 < 0 <= d1:
            return round(f0 + (f1 - f0) * (-d0) / (d1 - d0), 3)
    return None


shares = [0.01, 0.1] + [float(v) for v in args.more_shares.split(",") if v]
for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    tensor = gaussian(name, n)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    enc_work = torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda")
    wholes = [torch.empty_like(tensor) for _ in range(P)]
    whole_works = [torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    # (d)'s frame: the split tensor, every plane stored
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
        gsets = [ctx.make_gather_set([plans[p] for p in coded], [f[desc.offset[p]: desc.offset[p] + desc.length[p]] for p in coded]) for f in frames] if coded else None
        b_whole = timed_device(lambda i: ctx.decode_device_planes(planes, frames[i], wholes[i], whole_works[i]))
        assert ctx.planes_status(planes) == [0] * W and all(torch.equal(w, tensor) for w in wholes)

        points = []
        for row_len, share, dst_first in [(4096, f, 0) for f in shares] + [(1000, 0.01, 0), (1000, 0.01, 1)]:
            table_rows = n // row_len
            table = tensor[: table_rows * row_len].view(table_rows, row_len)
            count = max(1, int(table_rows * share))
            picked = np.random.default_rng(1000 * row_len + int(share * 1000)).permutation(table_rows)[:count]
            ranges = np.stack([picked * row_len, np.full(count, row_len), np.arange(count) * row_len + dst_first], axis=1).astype(np.uint64)
            d_picked = torch.from_numpy(picked.astype(np.int64)).cuda()
            want = table[d_picked]
            nbytes = count * row_len * W
            flats = [torch.zeros(count * row_len + 16, dtype=INT[W], device="cuda") for _ in range(P)]  # (what the call is given: 16-byte aligned)
            outs = [f[dst_first: dst_first + count * row_len].view(count, row_len) for f in flats]
            works = [torch.empty(H.planes_gather_workspace_bytes(W, count, count * row_len), dtype=torch.uint8, device="cuda") for _ in range(P)]

            def checked(what):
                torch.cuda.synchronize()
                for o in outs:
                    assert torch.equal(o, want), what
                    o.zero_()

            # (a)
            a_new = timed_device(lambda i: ctx.decode_device_planes_gather(pgs[i], ranges, flats[i], works[i]))
            a_host = timed_host_side(lambda i: ctx.decode_device_planes_gather(pgs[i], ranges, flats[i], works[i]))
            assert ctx.planes_gather_status(pgs[0]) == [0] * W
            info = pgs[0].info()
            checked("the new call")
            # (b)
            def today(i):
                ctx.decode_device_planes(planes, frames[i], wholes[i], whole_works[i])
                torch.index_select(wholes[i][: table_rows * row_len].view(table_rows, row_len), 0, d_picked, out=outs[i])

            b_today = timed_device(today)
            checked("the whole decode and the copy of the rows")
            # (c) the same rows of the coded planes, into the call's layout (include/hsrans_hip.h)
            c_gather = None
            if coded:
                phase = ranges[:, 0] % 16
                slot = (phase + ranges[:, 1] + 15) // 16 * 16
                base = np.concatenate([[0], np.cumsum(slot)[:-1]]).astype(np.uint64)
                stride = up(int(slot.sum()), 256)
                rows = np.concatenate([np.stack([np.full(count, k, np.uint64), ranges[:, 0], ranges[:, 1], np.uint64(p * stride) + base + phase], axis=1)
                                       for k, p in enumerate(coded)])
                c_gather = timed_device(lambda i: ctx.decode_device_gather_batch(gsets[i], rows, works[i]))
                assert ctx.gather_set_status(gsets[0]) == [0] * len(coded)
            # (d)
            d_merge = timed_device(lambda i: ctx.decode_device_planes_gather(raw_pgs[i], ranges, flats[i], works[i]))
            d_host = timed_host_side(lambda i: ctx.decode_device_planes_gather(raw_pgs[i], ranges, flats[i], works[i]))
            assert raw_pgs[0].info()["launches"] == 1
            checked("the merge alone")

            def copy(i):
                assert hip.hipMemcpyAsync(outs[i].data_ptr(), wholes[i].data_ptr(), nbytes, 3, stream) == 0  # (3: hipMemcpyDeviceToDevice)

            d_copy = timed_device(copy)
            if row_len == 4096 and dst_first == 0:
                points.append((share, a_new[0], b_today[0]))
            emit(dict(tool="tools/planes_gather_rate.py", tensor=f"gaussian {name}", elements=n, elem_size=W, bytes=n * W, codec=f"mt_ rANS32x64 16w {BITS}",
                      block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, stored_mask=int(desc.stored_mask), coded_planes=len(coded),
                      row_elements=row_len, share_of_rows=share, dst_first_element=dst_first, ranges=count, fetched_bytes=nbytes, gather_rows=info["rows"], merge_tasks=info["merge_tasks"],
                      launches=info["launches"], a_planes_gather_us=a_new, a_host_side_us=a_host, d_merge_host_side_us=d_host, b_whole_decode_then_copy_us=b_today, b_whole_decode_alone_us=b_whole,
                      c_gather_batch_alone_us=c_gather, d_merge_alone_us=d_merge, d_memcpy_same_bytes_us=d_copy, a_over_b=round(a_new[0] / b_today[0], 3),
                      merge_over_memcpy=round(d_merge[0] / d_copy[0], 2), a_fetched_GB_s=round(nbytes / a_new[0] / 1e3, 1),
                      us="[median, interquartile range]", reps=args.reps, sets_rotated=P, checked="every leg's rows == tensor[rows]"))
            del outs, flats, works, want
        emit(dict(tool="tools/planes_gather_rate.py", tensor=f"gaussian {name}", store_incompressible=store, row_elements=4096,
                  shares=[p[0] for p in points], a_us=[p[1] for p in points], b_us=[p[2] for p in points], crossover_share=crossover(points),
                  note="share of 4096-element rows at which the whole decode and a copy of the rows starts to win; linear between the measured shares around it"))
        for g in gsets or []:
            g.close()
        for pg in pgs:
            pg.close()
        planes.close()
        for p in plans:
            if p is not None:
                p.close()
        del frames, frame0, pgs, gsets
    for pg in raw_pgs:
        pg.close()
    raw_planes.close()
    del raw_frames, wholes, whole_works, enc_work, tensor
    torch.cuda.empty_cache()
