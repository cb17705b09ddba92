"""Every GPU encoder leg in one short process, for A/B runs of two builds (HSRANS_LIB=other/libhsrans_hip.so):  python tools/encode_legs_rate.py [--tag NAME] [--out FILE]

The calls are those of tools/encode_rate.py (mt_ in independent blocks: 100 MB at 32 and 64 KiB blocks, 2^30 bytes at 256 KiB; the raw
format), tools/encode_ex_rate.py (block_ and mt_ chains) and tools/encode_batch_rate.py (32 x 1 MiB raw and mt_), without their host
encoders, decodes and checks, on bytes made on the device.  One JSON line: milliseconds per leg, host clock around the synchronising call, best of --reps."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import hypersonic_rans_amd as H

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS = 64, 11


def best_ms(fn, reps):
    fn()  # warm-up
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(min(ts) * 1e3, 4)


rec = {"tool": "encode_legs_rate", "tag": args.tag, "lib": H.lib_path(), "device": ctx.device_name}
# Zipf-ish bytes made on the device (the host generator takes 80 s for 2^30 bytes)
u = torch.rand(1 << 30, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
d_big = (u.pow_(6).mul_(205)).to(torch.uint8)
del u
n = 100_000_000
d_in = d_big[:n]
d_out = torch.empty(H.capacity(H.MT, S, 1 << 30), dtype=torch.uint8, device="cuda")
for states, block in ((64, 1 << 15), (64, 1 << 16), (32, 1 << 16)):
    rec[f"mt{states}_100MB_{block >> 10}K_ms"] = best_ms(lambda: ctx.encode_device(H.MT, states, BITS, d_in, d_out, block_size=block), args.reps)
rec["mt64_100MB_64K_plan32_ms"] = best_ms(lambda: ctx.encode_device(H.MT, S, BITS, d_in, d_out, block_size=1 << 16, index_interval=32, want_plan=True), args.reps)
rec["mt64_1GiB_256K_ms"] = best_ms(lambda: ctx.encode_device(H.MT, S, BITS, d_big, d_out, block_size=1 << 18), args.reps)
rec["raw64_100MB_ms"] = best_ms(lambda: ctx.encode_device_raw(S, BITS, d_in, d_out), 3)
groups = H.index_boundaries(S, BITS, n, ctx)
for cont, name in ((H.BLOCK, "block"), (H.MT, "mt")):
    rec[f"chain_{name}_100MB_ms"] = best_ms(lambda: ctx.encode_device_ex(cont, S, BITS, d_in, d_out, index_groups=groups, want_plan=True), 3)
K, m = 32, 1 << 20
ins = [d_big[k * m + 16 * k: k * m + 16 * k + m].clone() for k in range(K)]
for cont, name, opts in ((H.RAW, "raw", {}), (H.MT, "mt", {"block_size": 1 << 16, "index_interval": 0})):
    outs = [torch.empty(H.capacity(cont, S, m), dtype=torch.uint8, device="cuda") for _ in range(K)]
    members = [(cont, S, BITS, ins[k], outs[k], opts) for k in range(K)]
    rec[f"batch_{name}_32x1MiB_ms"] = best_ms(lambda: ctx.encode_device_batch(members, want_plans=False), args.reps)
line = json.dumps(rec)
print(line, flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
