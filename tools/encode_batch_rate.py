"""hsrans_encode_device_batch against one single call per member: raw and mt_ (64 KiB independent blocks), 64 states, 11 bits, on
enwik8-shaped data in batches of 32 x 1 MB, 256 x 64 KiB and 8 x 16 MB, without and with plans (raw: the batch-shaped index of
hsrans_index_boundaries_batch; mt_: a checkpoint every 32 groups).  Both forms are synchronous; the time is a host clock around K single
calls or around the one batch call, after a warm-up, best, median and interquartile range over --windows windows.  Every member of the batch is checked bit
for bit (stream and plan) against its single call in the same process first.  Prints one JSON line per case and appends it to --out.
Run on the GPU box: python tools/encode_batch_rate.py --out profiles/r08_encode_batch_rate.jsonl"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=7)
ap.add_argument("--shapes", default="32x1048576,256x65536,8x16777216", help="comma-separated KxBYTES")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK = 64, 11, 1 << 16


def timed(fn):
    fn()  # warm-up
    ms = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return min(ms), float(med), float(q3 - q1)


def plan_bytes(p):
    """the plan blob, None where the call made no plan (a raw member whose batch-shaped index has no entry: too short for one)"""
    return None if p is None or not p.handle else ctx.read_device_plan(p)


def close(plans):
    for p in plans:
        if p is not None:
            p.close()


for shape in args.shapes.split(","):
    K, n = (int(v) for v in shape.split("x"))
    data = synth.enwik8_shaped(K * n + 4096, seed=5)
    d_ins = [torch.from_numpy(data[k * n + 16 * k: k * n + 16 * k + n].copy()).cuda() for k in range(K)]
    for container, name in ((H.RAW, "raw"), (H.MT, "mt_")):
        cap = H.capacity(container, S, n)
        outs_b = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)]
        outs_s = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)]
        for with_plans in (False, True):
            opts = []
            for k in range(K):
                if container == H.RAW:
                    opts.append({"index_groups": H.index_boundaries_batch(S, BITS, [n] * K, k, ctx)} if with_plans else {})
                else:
                    opts.append({"block_size": BLOCK, "index_interval": 32 if with_plans else 0})
            members = [(container, S, BITS, d_ins[k], outs_b[k], opts[k]) for k in range(K)]

            def singles():
                got = []
                for k in range(K):
                    if container == H.RAW:
                        r = ctx.encode_device_raw(S, BITS, d_ins[k], outs_s[k], index_groups=opts[k].get("index_groups"), want_device_plan=with_plans)
                    else:
                        r = ctx.encode_device(H.MT, S, BITS, d_ins[k], outs_s[k], block_size=BLOCK, index_interval=opts[k]["index_interval"], want_plan=with_plans)
                    got.append(r if with_plans else (r, None))
                return got

            def batch(stats=None):
                r = ctx.encode_device_batch(members, want_plans=with_plans, stats=stats)
                return r if with_plans else (r, [None] * K)

            # ---- the check: every member bit for bit against its single call ----
            stats = {}
            lengths, plans = batch(stats)
            one = singles()
            for k in range(K):
                m, p = one[k]
                assert lengths[k] == m, (name, shape, k)
                assert torch.equal(outs_b[k][:m], outs_s[k][:m]), (name, shape, k)
                if with_plans:
                    a, b = plan_bytes(plans[k]), plan_bytes(p)
                    assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), (name, shape, k)
            close(plans)
            close([p for _, p in one])
            # ---- the clock ----
            s_best, s_med, s_iqr = timed(lambda: close([p for _, p in singles()]))
            b_best, b_med, b_iqr = timed(lambda: close(batch()[1]))
            total = K * n
            row = dict(tool="tools/encode_batch_rate.py", codec=f"{name} rANS32x64 16w {BITS}", block_size=BLOCK if container == H.MT else None,
                       members=K, member_bytes=n, plans=with_plans, members_with_plans=sum(p is not None for p in plans),
                       launches=stats["launches"], mt_blocks=stats["mt_blocks"],
                       stream_bytes=int(sum(lengths)), singles_ms_best=round(s_best, 3), singles_ms_median=round(s_med, 3), singles_ms_iqr=round(s_iqr, 3),
                       batch_ms_best=round(b_best, 3), batch_ms_median=round(b_med, 3), batch_ms_iqr=round(b_iqr, 3),
                       singles_GB_s_best=round(total / s_best / 1e6, 2), batch_GB_s_best=round(total / b_best / 1e6, 2),
                       batch_GB_s_median=round(total / b_med / 1e6, 2), speedup_best=round(s_best / b_best, 2), speedup_median=round(s_med / b_med, 2),
                       windows=args.windows, checked="bit-exact vs single calls (streams and plans)")
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
