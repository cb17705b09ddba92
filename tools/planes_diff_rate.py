"""The diff byte-plane entries' rates against their XOR twins: a bf16 tensor of 2^26 elements and an fp32 tensor of 2^25 (128 MiB each),
`tuned` = base * (1 + 0.01 * standard_normal) coded against `base` (standard normal), 64 states, 11 bits, 64 KiB blocks, a checkpoint every
32 groups, stored planes allowed.  The rival of every leg is the delta (XOR) path on the same buffers in the same process.  Per tensor:
  (a) k_planes_split_diff against k_planes_split_delta, k_planes_merge_diff against k_planes_merge_delta, and both merges in place
      (each 3 tensor-sizes of traffic);
  (b) hsrans_encode_device_planes_diff against hsrans_encode_device_planes_delta, end to end;
  (c) hsrans_decode_device_planes_diff of the diff frame against hsrans_decode_device_planes_delta of the delta frame, end to end;
  (d) the two frames' plane lengths and their share of the tensor.
--sets buffer sets (> 700 MB each) are rotated, so no call finds its data in the 256 MB Infinity Cache.  Asynchronous legs are timed with
device events around the one call, the synchronous encoders with a host clock; median and interquartile range over --reps repetitions
after a warm-up of every set.  Every frame is decoded and compared with the tensor before anything is timed.  Prints one JSON line per
tensor and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box, one tensor per process: python tools/planes_diff_rate.py --tensor bf16 --out profiles/r26_planes_diff_rate.jsonl"""
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
ap.add_argument("--log2-bytes", type=int, default=27, help="tensor size (27: 128 MiB)")
ap.add_argument("--tensor", choices=["bf16", "fp32", "both"], default="both")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
SETTINGS = dict(states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=True)
P = args.sets


def spread(ms):
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return round(float(med) * 1e3, 2), round(float(q3 - q1) * 1e3, 2)  # microseconds


def timed_device(fn, before=None):
    """fn(set) queues work on the current stream: (median, IQR) in microseconds between two events around it; before(set) runs untimed"""
    for i in range(P):
        if before:
            before(i)
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for r in range(args.reps):
        if before:
            before(r % P)
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


def pair(name, n):
    g = torch.Generator(device="cuda").manual_seed(29)
    base = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    tuned = base * (1 + 0.01 * torch.randn(n, generator=g, device="cuda", dtype=torch.float32))
    if name == "fp32":
        return tuned, base
    bf16 = lambda x: (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)  # noqa: E731  (truncated)
    return bf16(tuned), bf16(base)


def close(plans):
    for p in plans:
        if p is not None:
            p.close()


def same(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def ratio(a, b):
    return round(a[0] / b[0], 3)


def apart(a, b):
    """the two legs' interquartile ranges do not meet"""
    return bool(abs(a[0] - b[0]) > (a[1] + b[1]) / 2)


for name, W in (("bf16", 2), ("fp32", 4)):
    if args.tensor not in (name, "both"):
        continue
    n = (1 << args.log2_bytes) // W
    nbytes = n * W
    first, first_base = pair(name, n)
    tensors = [first] + [first.clone() for _ in range(P - 1)]
    bases = [first_base] + [first_base.clone() for _ in range(P - 1)]
    frames = [torch.empty(H.planes_capacity(W, S, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    works = [torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    outs = [torch.empty_like(first) for _ in range(P)]
    scratch = [torch.empty_like(first) for _ in range(P)]  # the in-place legs' copies of the base
    stride = works[0].numel() // W
    planes_of = [[w[p * stride: p * stride + n] for p in range(W)] for w in works]
    restore = lambda i: scratch[i].copy_(bases[i])  # noqa: E731

    # ---- (a) the kernels alone, diff against delta, on the same buffers (the merges read the planes their own split left) ----
    a_split_delta = timed_device(lambda i: ctx.planes_split_delta_device(tensors[i], bases[i], planes_of[i]))
    a_merge_delta = timed_device(lambda i: ctx.planes_merge_delta_device(planes_of[i], bases[i], outs[i]))
    for i in range(P):
        assert same(outs[i], tensors[i]), "merge_delta(split_delta(x, base), base) != x"
    a_merge_delta_in_place = timed_device(lambda i: ctx.planes_merge_delta_device(planes_of[i], scratch[i], scratch[i]), before=restore)
    a_split_diff = timed_device(lambda i: ctx.planes_split_diff_device(tensors[i], bases[i], planes_of[i]))
    for o in outs:
        o.zero_()
    a_merge_diff = timed_device(lambda i: ctx.planes_merge_diff_device(planes_of[i], bases[i], outs[i]))
    for i in range(P):
        assert same(outs[i], tensors[i]), "merge_diff(split_diff(x, base), base) != x"
    a_merge_diff_in_place = timed_device(lambda i: ctx.planes_merge_diff_device(planes_of[i], scratch[i], scratch[i]), before=restore)
    for i in range(P):
        assert same(scratch[i], tensors[i]), "the diff merge in place"

    # ---- (b) the encoders, end to end; (c) the decoders, each over its own frame ----
    legs = {}
    for rule in ("delta", "diff"):
        encode = getattr(ctx, f"encode_device_planes_{rule}")
        decode = getattr(ctx, f"decode_device_planes_{rule}")
        enc_us = timed_host(lambda i: close(encode(tensors[i], bases[i], frames[i], works[i], **SETTINGS)[2]))
        total, desc, plans = encode(tensors[0], bases[0], frames[0], works[0], **SETTINGS)
        for i in range(1, P):
            frames[i].copy_(frames[0])
        planes = ctx.make_planes(desc, plans)
        for o in outs:
            o.zero_()
        dec_us = timed_device(lambda i: decode(planes, frames[i], bases[i], outs[i], works[i]))
        assert ctx.planes_status(planes) == [0] * W
        for i in range(P):
            assert same(outs[i], tensors[i]), f"the {rule} frame does not decode to the tensor"
        dec_in_place_us = timed_device(lambda i: decode(planes, frames[i], scratch[i], scratch[i], works[i]), before=restore)
        assert ctx.planes_status(planes) == [0] * W
        for i in range(P):
            assert same(scratch[i], tensors[i]), f"the {rule} frame decoded in place"
        legs[rule] = dict(encode=enc_us, decode=dec_us, decode_in_place=dec_in_place_us, plane_bytes=[int(desc.length[p]) for p in range(W)],
                          stored_mask=int(desc.stored_mask), launches=planes.info()["launches"])
        planes.close()
        close(plans)

    d, z = legs["delta"], legs["diff"]
    row = dict(tool="tools/planes_diff_rate.py", tensor=f"{name}: base * (1 + 0.01 * standard_normal) against base", elements=n, elem_size=W, bytes=nbytes,
               codec=f"mt_ rANS32x64 16w {BITS}", block_size=BLOCK, index_interval=INTERVAL, store_incompressible=True, rival="the XOR delta path, same buffers, same process",
               delta_stored_mask=d["stored_mask"], diff_stored_mask=z["stored_mask"], decode_launches=[d["launches"], z["launches"]],
               delta_plane_bytes=d["plane_bytes"], diff_plane_bytes=z["plane_bytes"], delta_frame_bytes=sum(d["plane_bytes"]), diff_frame_bytes=sum(z["plane_bytes"]),
               delta_share_of_tensor=round(sum(d["plane_bytes"]) / nbytes, 4), diff_share_of_tensor=round(sum(z["plane_bytes"]) / nbytes, 4),
               diff_over_delta_frame=round(sum(z["plane_bytes"]) / sum(d["plane_bytes"]), 4),
               a_split_delta_us=a_split_delta, a_split_diff_us=a_split_diff, split_diff_over_delta=ratio(a_split_diff, a_split_delta),
               split_ranges_apart=apart(a_split_diff, a_split_delta),
               a_merge_delta_us=a_merge_delta, a_merge_diff_us=a_merge_diff, merge_diff_over_delta=ratio(a_merge_diff, a_merge_delta),
               merge_ranges_apart=apart(a_merge_diff, a_merge_delta),
               a_merge_delta_in_place_us=a_merge_delta_in_place, a_merge_diff_in_place_us=a_merge_diff_in_place,
               merge_in_place_diff_over_delta=ratio(a_merge_diff_in_place, a_merge_delta_in_place),
               split_diff_GB_s=round(3 * nbytes / a_split_diff[0] / 1e3, 1), merge_diff_GB_s=round(3 * nbytes / a_merge_diff[0] / 1e3, 1),
               split_delta_GB_s=round(3 * nbytes / a_split_delta[0] / 1e3, 1), merge_delta_GB_s=round(3 * nbytes / a_merge_delta[0] / 1e3, 1),
               b_encode_delta_us=d["encode"], b_encode_diff_us=z["encode"], encode_diff_over_delta=ratio(z["encode"], d["encode"]),
               c_decode_delta_us=d["decode"], c_decode_diff_us=z["decode"], decode_diff_over_delta=ratio(z["decode"], d["decode"]),
               c_decode_delta_in_place_us=d["decode_in_place"], c_decode_diff_in_place_us=z["decode_in_place"],
               decode_in_place_diff_over_delta=ratio(z["decode_in_place"], d["decode_in_place"]),
               encode_diff_GB_s=round(nbytes / z["encode"][0] / 1e3, 1), decode_diff_GB_s=round(nbytes / z["decode"][0] / 1e3, 1),
               us="[median, interquartile range]", reps=args.reps, sets_rotated=P,
               checked="both frames decoded back to the tensor, apart and in place; merge(split(x)) == x under both rules, apart and in place")
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del tensors, bases, frames, works, outs, scratch, planes_of, first, first_base
    torch.cuda.empty_cache()
