"""The delta byte-plane entries' rates: a bf16 tensor of 2^26 elements and an fp32 tensor of 2^25 (128 MiB each), `tuned` = base * (1 + 0.01 *
standard_normal) coded against `base` (standard normal), 64 states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, stored planes
allowed.  Per tensor:
  (a) k_planes_split_delta / k_planes_merge_delta alone against the plain k_planes_split / k_planes_merge on the same buffers (by traffic
      3 tensor-sizes against 2), and the merge in place;
  (b) hsrans_decode_device_planes_delta against hsrans_decode_device_planes of the same frame, against the route without the entry —
      the plain decode into a scratch tensor, then torch.bitwise_xor with the base into the output, which needs that tensor-sized
      scratch — and in place over a copy of the base;
  (c) hsrans_encode_device_planes_delta against a torch.bitwise_xor pass into a scratch tensor followed by the plain encode of it;
  (d) the frame sizes: the tensor alone, the tensor against its base, and their share of the tensor.
--sets buffer sets (> 700 MB each) are rotated, so no call finds its data in the 256 MB Infinity Cache.  Asynchronous legs are timed with
device events around the one call, the synchronous encoders with a host clock; median and interquartile range over --reps repetitions
after a warm-up of every set.  Every frame is decoded and compared with the tensor before anything is timed.  Prints one JSON line per
tensor and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_delta_rate.py --out profiles/r24_planes_delta_rate.jsonl"""
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


for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    nbytes = n * W
    INT = {2: torch.int16, 4: torch.int32}[W]
    first, first_base = pair(name, n)
    tensors = [first] + [first.clone() for _ in range(P - 1)]
    bases = [first_base] + [first_base.clone() for _ in range(P - 1)]
    frames = [torch.empty(H.planes_capacity(W, S, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    works = [torch.empty(H.planes_workspace_bytes(W, n), dtype=torch.uint8, device="cuda") for _ in range(P)]
    outs = [torch.empty_like(first) for _ in range(P)]
    scratch = [torch.empty_like(first) for _ in range(P)]  # what the routes without the entries need: one more tensor
    stride = works[0].numel() // W
    planes_of = [[w[p * stride: p * stride + n] for p in range(W)] for w in works]

    # ---- (a) the kernels alone, delta against plain, on the same buffers ----
    a_split = timed_device(lambda i: ctx.planes_split_device(tensors[i], planes_of[i]))
    a_merge = timed_device(lambda i: ctx.planes_merge_device(planes_of[i], outs[i]))
    a_split_delta = timed_device(lambda i: ctx.planes_split_delta_device(tensors[i], bases[i], planes_of[i]))
    a_merge_delta = timed_device(lambda i: ctx.planes_merge_delta_device(planes_of[i], bases[i], outs[i]))
    for i in range(P):
        assert same(outs[i], tensors[i]), "merge_delta(split_delta(x, base), base) != x"
    a_merge_in_place = timed_device(lambda i: ctx.planes_merge_delta_device(planes_of[i], scratch[i], scratch[i]), before=lambda i: scratch[i].copy_(bases[i]))
    for i in range(P):
        assert same(scratch[i], tensors[i]), "the merge in place"

    # ---- (c) the encoders: delta, and an XOR pass into a scratch tensor with the plain encode behind it ----
    def enc_delta(i, keep=False):
        r = ctx.encode_device_planes_delta(tensors[i], bases[i], frames[i], works[i], **SETTINGS)
        if keep:
            return r
        close(r[2])

    def enc_by_hand(i):
        torch.bitwise_xor(tensors[i].view(INT), bases[i].view(INT), out=scratch[i].view(INT))
        close(ctx.encode_device_planes(scratch[i], frames[i], works[i], **SETTINGS)[2])

    def enc_plain(i, keep=False):
        r = ctx.encode_device_planes(tensors[i], frames[i], works[i], **SETTINGS)
        if keep:
            return r
        close(r[2])

    c_plain = timed_host(enc_plain)
    plain_total, plain_desc, plain_plans = enc_plain(0, keep=True)
    close(plain_plans)
    c_by_hand = timed_host(enc_by_hand)
    c_delta = timed_host(enc_delta)
    total, desc, plans = enc_delta(0, keep=True)
    for i in range(1, P):
        frames[i].copy_(frames[0])

    # ---- (b) the decoders ----
    planes = ctx.make_planes(desc, plans)
    info = planes.info()
    for o in outs:
        o.zero_()
    b_plain = timed_device(lambda i: ctx.decode_device_planes(planes, frames[i], outs[i], works[i]))
    assert ctx.planes_status(planes) == [0] * W
    assert torch.equal(outs[0].view(INT), tensors[0].view(INT) ^ bases[0].view(INT)), "the plain decode of a delta frame is the residue"

    def by_hand(i):
        ctx.decode_device_planes(planes, frames[i], scratch[i], works[i])
        torch.bitwise_xor(scratch[i].view(INT), bases[i].view(INT), out=outs[i].view(INT))

    b_by_hand = timed_device(by_hand)
    for i in range(P):
        assert same(outs[i], tensors[i]), "decode, then XOR"
        outs[i].zero_()
    b_delta = timed_device(lambda i: ctx.decode_device_planes_delta(planes, frames[i], bases[i], outs[i], works[i]))
    assert ctx.planes_status(planes) == [0] * W
    for i in range(P):
        assert same(outs[i], tensors[i]), "the delta frame does not decode to the tensor"
    b_in_place = timed_device(lambda i: ctx.decode_device_planes_delta(planes, frames[i], scratch[i], scratch[i], works[i]), before=lambda i: scratch[i].copy_(bases[i]))
    assert ctx.planes_status(planes) == [0] * W
    for i in range(P):
        assert same(scratch[i], tensors[i]), "the delta frame decoded in place"
    planes.close()
    close(plans)

    payload = int(sum(desc.length[p] for p in range(W)))
    plain_payload = int(sum(plain_desc.length[p] for p in range(W)))
    row = dict(tool="tools/planes_delta_rate.py", tensor=f"{name}: base * (1 + 0.01 * standard_normal) against base", elements=n, elem_size=W, bytes=nbytes,
               codec=f"mt_ rANS32x64 16w {BITS}", block_size=BLOCK, index_interval=INTERVAL, store_incompressible=True,
               plain_stored_mask=int(plain_desc.stored_mask), delta_stored_mask=int(desc.stored_mask), decode_launches=info["launches"],
               plain_plane_bytes=[int(plain_desc.length[p]) for p in range(W)], delta_plane_bytes=[int(desc.length[p]) for p in range(W)],
               plain_frame_bytes=plain_payload, plain_share_of_tensor=round(plain_payload / nbytes, 4), delta_frame_bytes=payload,
               delta_share_of_tensor=round(payload / nbytes, 4), delta_over_plain_frame=round(payload / plain_payload, 4),
               a_split_us=a_split, a_split_delta_us=a_split_delta, split_delta_over_split=round(a_split_delta[0] / a_split[0], 3),
               a_merge_us=a_merge, a_merge_delta_us=a_merge_delta, merge_delta_over_merge=round(a_merge_delta[0] / a_merge[0], 3),
               a_merge_delta_in_place_us=a_merge_in_place, split_delta_GB_s=round(3 * nbytes / a_split_delta[0] / 1e3, 1),
               merge_delta_GB_s=round(3 * nbytes / a_merge_delta[0] / 1e3, 1), split_GB_s=round(2 * nbytes / a_split[0] / 1e3, 1), merge_GB_s=round(2 * nbytes / a_merge[0] / 1e3, 1),
               b_decode_plain_us=b_plain, b_decode_then_xor_us=b_by_hand, b_decode_delta_us=b_delta, b_decode_delta_in_place_us=b_in_place,
               decode_delta_over_plain=round(b_delta[0] / b_plain[0], 3), decode_delta_over_decode_then_xor=round(b_delta[0] / b_by_hand[0], 3),
               decode_delta_GB_s=round(nbytes / b_delta[0] / 1e3, 1), decode_then_xor_extra_buffer_bytes=nbytes,
               c_encode_plain_tensor_us=c_plain, c_xor_then_encode_us=c_by_hand, c_encode_delta_us=c_delta,
               encode_delta_over_xor_then_encode=round(c_delta[0] / c_by_hand[0], 3), encode_delta_GB_s=round(nbytes / c_delta[0] / 1e3, 1),
               xor_then_encode_extra_buffer_bytes=nbytes, us="[median, interquartile range]", reps=args.reps, sets_rotated=P,
               checked="delta frame decoded back to the tensor, apart and in place; plain decode of it is the residue; merge_delta(split_delta(x)) == x")
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    del tensors, bases, frames, works, outs, scratch, planes_of, first, first_base
    torch.cuda.empty_cache()
