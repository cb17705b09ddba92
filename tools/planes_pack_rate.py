"""Many frames of byte planes into one exact-size arena: K in {8, 32, 128} Gaussian bf16 tensors of 2^19 elements and fp32 tensors of 2^18
(1 MiB each), and one tensor of 128 MiB of each type; 64 states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, with and without
stored planes.  The frames are encoded once (hsrans_encode_device_planes_batch); then three legs move them into the same arena:
  (a) hsrans_planes_pack_device: one call, one launch (the C entry on arrays made outside the clock);
  (b) what a caller writes without it: one hipMemcpyAsync device-to-device per plane to the layout's offsets;
  (c) ONE hipMemcpyAsync device-to-device of the arena's total bytes from a buffer of that size: the bandwidth yardstick.
Per leg the device time between two events around it and the host time the calls keep the CPU (the clock around the queueing alone).
--sets buffer sets (frames, arenas) are rotated.  Median and interquartile range over --reps repetitions after a warm-up of every set.
Before anything is timed the arena of (a) is compared with the arena of (b) plane by plane — and its pads with zero — and decoded back to
the tensors through the packed descriptors.  Prints one JSON line per case and appends it to --out.  Nothing is gated.
--variant NAME only labels the rows: the k_pack tuning builds (make -C hypersonic_rans_amd/csrc pack_variants) are run one after the other
with HSRANS_LIB naming the library.
Run on the GPU box: python tools/planes_pack_rate.py --out profiles/r23_planes_pack_rate.jsonl"""
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
ap.add_argument("--counts", type=int, nargs="*", default=[8, 32, 128])
ap.add_argument("--log2-bytes", type=int, default=20, help="bytes of one of the K tensors (20: 1 MiB)")
ap.add_argument("--big-log2-bytes", type=int, default=27, help="bytes of the one large tensor (27: 128 MiB; 0: none)")
ap.add_argument("--variant", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
L = ctx.L
hip = ctypes.CDLL("libamdhip64.so")  # (the runtime torch loaded)
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P = args.sets
CHUNK = (1 << 30) // H.pack_tasks([1 << 30])[0]  # the loaded library's HSRANS_PACK_CHUNK


def up16(v):
    return (int(v) + 15) // 16 * 16


def spread(ms):
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return [round(float(med) * 1e3, 2), round(float(q3 - q1) * 1e3, 2), round(float(q1) * 1e3, 2), round(float(q3) * 1e3, 2)]  # microseconds


def timed(fn):
    """fn(set) queues work on the current stream: (microseconds between two events around it, microseconds fn kept the host)"""
    for i in range(P):
        fn(i)
    torch.cuda.synchronize()
    dev, host = [], []
    for r in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn(r % P)
        host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    return spread(dev), spread(host)


def gaussian(name, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, generator=g, device="cuda", dtype=torch.float32)
    if name == "fp32":
        return x
    return (x.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)  # truncated


def apart(a, b):
    """the faster leg's third quartile below the slower leg's first: the interquartile ranges do not overlap"""
    return a[3] < b[2]


cases = [(name, W, K, args.log2_bytes) for name, W in (("bf16", 2), ("fp32", 4)) for K in args.counts]
if args.big_log2_bytes:
    cases += [(name, W, 1, args.big_log2_bytes) for name, W in (("bf16", 2), ("fp32", 4))]
for name, W, K, log2_bytes in cases:
    n = (1 << log2_bytes) // W
    tensors = [gaussian(name, n, 41 + k) for k in range(K)]
    cap = H.planes_capacity(W, S, n)
    work = torch.empty(H.planes_batch_workspace_bytes([W] * K, [n] * K), dtype=torch.uint8, device="cuda")
    frames = [[torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)] for _ in range(P)]
    for store in (False, True):
        got = ctx.encode_device_planes_batch(tensors, frames[0], work, states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store)
        descs, plans = [g[1] for g in got], [g[2] for g in got]
        for i in range(1, P):
            for k in range(K):
                frames[i][k].copy_(frames[0][k])
        packed_descs, bases, total = H.planes_pack_layout(descs)
        arenas = [torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(P)]
        yard = [torch.empty(total, dtype=torch.uint8, device="cuda") for _ in range(P)]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        # ---- (a) the call: its arrays made once, outside the clock ----
        c_descs, c_out, c_bases = (api.PlanesDesc * K)(*descs), (api.PlanesDesc * K)(), (ctypes.c_uint64 * (K + 1))()
        c_frames = [(ctypes.c_void_p * K)(*[f.data_ptr() for f in frames[i]]) for i in range(P)]
        c_lengths = (ctypes.c_size_t * K)(*([cap] * K))

        def pack(i):
            assert L.hsrans_planes_pack_device(ctx.handle, c_descs, c_frames[i], c_lengths, K, arenas[i].data_ptr(), total, stream, c_out, c_bases) == 0

        a_dev, a_host = timed(pack)
        assert [bytes(d) for d in c_out] == [bytes(d) for d in packed_descs] and list(c_bases) == bases
        packed = [a.clone() for a in arenas]

        # ---- (b) a copy per plane into the same arena ----
        copies = [[(arenas[i].data_ptr() + bases[k] + packed_descs[k].offset[p], frames[i][k].data_ptr() + descs[k].offset[p], int(descs[k].length[p]))
                   for k in range(K) for p in range(W)] for i in range(P)]
        for a in arenas:
            a.zero_()  # (the copies do not write the pads)

        def per_plane(i):
            for dst, src, nbytes in copies[i]:
                assert hip.hipMemcpyAsync(dst, src, nbytes, 3, stream) == 0  # (3: hipMemcpyDeviceToDevice)

        b_dev, b_host = timed(per_plane)
        for i in range(P):
            assert torch.equal(arenas[i], packed[i]), "the pack and the copies per plane disagree"

        # ---- (c) one copy of the arena's bytes ----
        def one_copy(i):
            assert hip.hipMemcpyAsync(arenas[i].data_ptr(), yard[i].data_ptr(), total, 3, stream) == 0

        c_dev, c_host = timed(one_copy)

        # the packed arena decodes back to the tensors
        slices = [packed[0][bases[k]: bases[k] + packed_descs[k].frame_length] for k in range(K)]
        pset = ctx.make_planes_set(packed_descs, plans)
        outs = [torch.empty_like(t) for t in tensors]
        ctx.decode_device_planes_batch(pset, slices, outs, work)
        assert ctx.planes_set_status(pset) == [0] * K
        assert all(torch.equal(o.view(torch.uint8), t.view(torch.uint8)) for o, t in zip(outs, tensors)), "the arena does not decode to the tensors"
        pset.close()
        for g in got:
            for p in g[2]:
                if p is not None:
                    p.close()

        raw = K * n * W
        row = dict(tool="tools/planes_pack_rate.py", tensor=f"gaussian {name}", members=K, elements=n, elem_size=W, bytes=raw, codec=f"mt_ rANS32x64 16w {BITS}",
                   block_size=BLOCK, index_interval=INTERVAL, store_incompressible=store, stored_planes=sum(bin(d.stored_mask).count("1") for d in descs), planes=K * W,
                   frames_bytes=K * cap, arena_bytes=total, arena_over_tensors=round(total / raw, 4), pack_chunk=CHUNK, pack_tasks=H.pack_tasks([d.length[p] for d in descs for p in range(W)])[0],
                   a_pack_device_us=a_dev, a_pack_host_us=a_host, b_copies_device_us=b_dev, b_copies_host_us=b_host, c_one_copy_device_us=c_dev, c_one_copy_host_us=c_host,
                   copies_host_over_pack_host=round(b_host[0] / a_host[0], 2), host_ranges_apart=apart(a_host, b_host),
                   copies_device_over_pack_device=round(b_dev[0] / a_dev[0], 2), device_ranges_apart=apart(a_dev, b_dev),
                   pack_device_over_one_copy=round(a_dev[0] / c_dev[0], 2), pack_GB_s=round(total / a_dev[0] / 1e3, 1), one_copy_GB_s=round(total / c_dev[0] / 1e3, 1),
                   us="[median, interquartile range, first quartile, third quartile]", reps=args.reps, sets_rotated=P,
                   checked="the call's arena equals the per-plane copies' over zeroed pads; its descriptors equal the layout's; the arena decoded back to the tensors")
        if args.variant:
            row["variant"] = args.variant
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del arenas, yard, packed, slices, outs
    del tensors, frames, work
    torch.cuda.empty_cache()
