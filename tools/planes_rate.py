"""The byte-plane layer's rates: a Gaussian bf16 tensor of 2^26 elements and a Gaussian fp32 tensor of 2^25 (128 MiB each), 64 states,
11 bits, 64 KiB blocks, a checkpoint every 32 groups, with and without stored planes.  Per case:
  (a) k_planes_split / k_planes_merge alone against a hipMemcpyAsync device-to-device of the same byte count on the same buffers;
  (b) hsrans_decode_device_planes against hsrans_decode_device_batch of the same plans alone: the price of the separate interleave pass;
  (c) what a user has without the layer: the tensor's bytes as ONE mt_ stream through hsrans_encode_device / hsrans_decode_device,
      its time and its compressed size next to the frame's;
  (d) hsrans_encode_device_planes end to end.
--sets buffer sets (tensor, frame, workspace, output; > 500 MB each) are rotated, so no call finds its data in the 256 MB Infinity
Cache.  Asynchronous legs are timed with device events around the one call, the synchronous encoders with a host clock; median and
interquartile range over --reps repetitions after a warm-up of every set.  The frame is decoded and compared with the tensor before
anything is timed.  Prints one JSON line per case and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_rate.py --out profiles/r17_planes_rate.jsonl"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--log2-bytes", type=int, default=27, help="tensor size (27: 128 MiB)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch loaded)
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P = args.sets


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


def timed_host(fn):
    """fn(set) returns with its work done: (median, IQR) in microseconds on the host clock"""
    for i in range(P):
        fn(i)
    ms = []
    for r in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r % P)
        ms.append((time.perf_counter() - t0) * 1e3)
    return spread(ms)


def gaussian(name, n):
    g = torch.Generator(device="cuda").manual_seed(41)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    if name == "fp32":
        return x
    return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)  # truncated


def close(plans):
    for p in plans:
        if p is not None:
            p.close()


for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    nbytes = n * W
    first = gaussian(name, n)
    tensors = [first] + [first.clone() for _ in range(P - 1)]
    frames = [torch.empty(H.planes_capacity(W, S, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    works = [torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    outs = [torch.empty_like(first) for _ in range(P)]
    singles = [torch.empty(H.capacity(H.MT, S, nbytes), dtype=torch.uint8, device="cuda") for _ in range(P)]
    stride = works[0].numel() // W
    planes_of = [[w[p * stride: p * stride + n] for p in range(W)] for w in works]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- (a) the kernels alone and the copy, on the same buffers ----
    def copy(i):
        assert hip.hipMemcpyAsync(outs[i].data_ptr(), tensors[i].data_ptr(), nbytes, 3, stream) == 0  # (3: hipMemcpyDeviceToDevice)

    a_copy = timed_device(copy)
    a_split = timed_device(lambda i: ctx.planes_split_device(tensors[i], planes_of[i]))
    a_merge = timed_device(lambda i: ctx.planes_merge_device(planes_of[i], outs[i]))
    for i in range(P):
        assert torch.equal(outs[i].view(torch.uint8), tensors[i].view(torch.uint8)), "merge(split(x)) != x"

    # ---- (c) the bytes as they lie, one mt_ stream ----
    as_bytes = [t.view(torch.uint8) for t in tensors]
    one_len, one_plan = ctx.encode_device(H.MT, S, BITS, as_bytes[0], singles[0], block_size=BLOCK, index_interval=INTERVAL, want_plan=True)
    for i in range(1, P):
        singles[i][:one_len] = singles[0][:one_len]

    def one_encode(i):
        m, p = ctx.encode_device(H.MT, S, BITS, as_bytes[i], singles[i], block_size=BLOCK, index_interval=INTERVAL, want_plan=True)
        p.close()

    c_encode = timed_host(one_encode)
    c_decode = timed_device(lambda i: ctx.decode_device(one_plan, singles[i], outs[i].view(torch.uint8)))
    assert ctx.status(one_plan) == 0 and torch.equal(outs[0].view(torch.uint8), as_bytes[0])
    one_plan.close()

    for store in (False, True):
        # ---- (d) the encoder end to end ----
        def enc(i, keep=False):
            r = ctx.encode_device_planes(tensors[i], frames[i], works[i], states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)
            if keep:
                return r
            close(r[2])

        d_encode = timed_host(enc)
        total, desc, plans = enc(0, keep=True)
        for i in range(1, P):
            frames[i].copy_(frames[0])
        # ---- (b) the frame decoded, against the batch decode of its coded planes alone ----
        planes = ctx.make_planes(desc, plans)
        info = planes.info()
        for o in outs:
            o.zero_()
        b_planes = timed_device(lambda i: ctx.decode_device_planes(planes, frames[i], outs[i], works[i]))
        assert ctx.planes_status(planes) == [0] * W
        for i in range(P):
            assert torch.equal(outs[i].view(torch.uint8), tensors[i].view(torch.uint8)), "the frame does not decode to the tensor"
        planes.close()
        coded = [p for p in range(W) if plans[p] is not None]
        batch = ctx.make_batch([plans[p] for p in coded])
        b_batch = timed_device(lambda i: ctx.decode_device_batch(batch, [frames[i][desc.offset[p]: desc.offset[p] + desc.length[p]] for p in coded],
                                                                  [planes_of[i][p] for p in coded]))
        assert ctx.batch_status(batch) == [0] * len(coded)
        batch.close()
        close(plans)

        payload = int(sum(desc.length[p] for p in range(W)))
        row = dict(tool="tools/planes_rate.py", tensor=f"gaussian {name}", elements=n, elem_size=W, bytes=nbytes, codec=f"mt_ rANS32x64 16w {BITS}", block_size=BLOCK,
                   index_interval=INTERVAL, store_incompressible=store, stored_mask=int(desc.stored_mask), coded_planes=info["coded"], decode_launches=info["launches"],
                   plane_bytes=[int(desc.length[p]) for p in range(W)], frame_payload_bytes=payload, frame_payload_ratio=round(payload / nbytes, 4),
                   one_stream_bytes=int(one_len), one_stream_ratio=round(one_len / nbytes, 4), frame_over_one_stream=round(payload / one_len, 4),
                   a_copy_us=a_copy, a_split_us=a_split, a_merge_us=a_merge, split_over_copy=round(a_split[0] / a_copy[0], 2), merge_over_copy=round(a_merge[0] / a_copy[0], 2),
                   b_decode_planes_us=b_planes, b_decode_batch_us=b_batch, interleave_price_us=round(b_planes[0] - b_batch[0], 2),
                   decode_planes_over_batch=round(b_planes[0] / b_batch[0], 2), decode_planes_GB_s=round(nbytes / b_planes[0] / 1e3, 1),
                   c_one_stream_encode_us=c_encode, c_one_stream_decode_us=c_decode, decode_planes_over_one_stream=round(b_planes[0] / c_decode[0], 2),
                   d_encode_planes_us=d_encode, encode_planes_GB_s=round(nbytes / d_encode[0] / 1e3, 1), encode_planes_over_one_stream=round(d_encode[0] / c_encode[0], 2),
                   us="[median, interquartile range]", reps=args.reps, sets_rotated=P, checked="frame decoded back to the tensor; merge(split(x)) == x")
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    del tensors, frames, works, outs, singles, planes_of, as_bytes, first
    torch.cuda.empty_cache()
