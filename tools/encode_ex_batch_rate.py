"""hsrans_encode_device_ex_batch against one hsrans_encode_device_ex call per member, and against the largest member's single call alone:
block_ and mt_ streams with the reference's adaptive blocks, 64 states, 11 bits, on enwik8-shaped data in batches of 8 / 32 / 128 x 1 MB
and 8 x 16 MB, without an index and with a checkpoint every 32 groups (plan blobs and device plans asked for).  All three legs are
synchronous; the time is a host clock around the one batch call, around the K single calls, or around the one single call, after a
warm-up: median and interquartile range over --reps repetitions, and the batch's four phase times (medians of its stats).  Every member
of the batch is checked byte for byte (stream and plan) against its single call in the same process before anything is timed.  Prints
one JSON line per case and appends it to --out.
Run on the GPU box: python tools/encode_ex_batch_rate.py --out profiles/r16_encode_ex_batch_rate.jsonl"""
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
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--shapes", default="8x1048576,32x1048576,128x1048576,8x16777216", help="comma-separated KxBYTES")
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, INTERVAL = 64, 11, 32
PHASES = ("summaries_us", "walk_us", "chain_us", "plans_us")


def timed(fn):
    """median and interquartile range (ms) of args.reps calls after a warm-up, and what the calls returned"""
    fn()
    ms, got = [], []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got.append(fn())
        ms.append((time.perf_counter() - t0) * 1e3)
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return float(med), float(q3 - q1), got


def close(plans):
    for p in plans or ():
        if p is not None:
            p.close()


for shape in args.shapes.split(","):
    K, n = (int(v) for v in shape.split("x"))
    data = synth.enwik8_shaped(K * n + 4096, seed=5)
    d_ins = [torch.from_numpy(data[k * n + 16 * k: k * n + 16 * k + n].copy()).cuda() for k in range(K)]
    for container, name in ((H.BLOCK, "block_"), (H.MT, "mt_")):
        cap = H.capacity(container, S, n)
        outs_b = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)]
        outs_s = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)]
        for indexed in (False, True):
            opts = {"index_interval": INTERVAL} if indexed else {}
            members = [(container, S, BITS, d_ins[k], outs_b[k], opts) for k in range(K)]

            def single(k):
                """(length, plan blob or None); the device plan is closed"""
                r = ctx.encode_device_ex(container, S, BITS, d_ins[k], outs_s[k], want_plan=indexed, want_device_plan=indexed, **opts)
                if not indexed:
                    return r, None
                r[2].close()
                return r[0], r[1]

            def batch():
                stats = {}
                r = ctx.encode_device_ex_batch(members, want_plans=indexed, want_device_plans=indexed, stats=stats)
                if not indexed:
                    return r, [None] * K, stats
                close(r[2])
                return r[0], r[1], stats

            # ---- the check: every member byte for byte against its single call ----
            lengths, plans, stats = batch()
            for k in range(K):
                m, p = single(k)
                assert lengths[k] == m, (name, shape, k)
                assert torch.equal(outs_b[k][:m], outs_s[k][:m]), (name, shape, k)
                assert (plans[k] is None) == (p is None) and (p is None or np.array_equal(plans[k], p)), (name, shape, k)
            # ---- the clock ----
            b_med, b_iqr, got = timed(batch)
            s_med, s_iqr, _ = timed(lambda: [single(k) for k in range(K)])
            o_med, o_iqr, _ = timed(lambda: single(0))  # (all members are n bytes: the first is a largest one)
            phases = {p: round(float(np.median([g[2][p] for g in got])) / 1e3, 3) for p in PHASES}
            total = K * n
            row = dict(tool="tools/encode_ex_batch_rate.py", codec=f"{name} rANS32x64 16w {BITS}", blocks="adaptive", members=K, member_bytes=n,
                       index_interval=INTERVAL if indexed else 0, launches=stats["launches"], units=stats["units"], blocks_coded=stats["blocks"],
                       stream_bytes=int(sum(lengths)), batch_ms_median=round(b_med, 3), batch_ms_iqr=round(b_iqr, 3), singles_ms_median=round(s_med, 3),
                       singles_ms_iqr=round(s_iqr, 3), largest_single_ms_median=round(o_med, 3), largest_single_ms_iqr=round(o_iqr, 3),
                       batch_phase_ms_median={p[:-3]: v for p, v in phases.items()}, batch_GB_s_median=round(total / b_med / 1e6, 2),
                       singles_GB_s_median=round(total / s_med / 1e6, 2), speedup_median=round(s_med / b_med, 2),
                       batch_over_largest_single=round(b_med / o_med, 2), reps=args.reps, checked="byte-exact vs single calls (streams and plans)")
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
