"""hsrans_encode_device_ex rate: 100 MB, block_ and mt_, the reference's adaptive blocks (block_size 0) with the one-chain-per-wave index
(hsrans_index_boundaries), on config-2 data (enwik8-shaped) and on non-stationary data.  Beside it, on the same data in the same run:
hsrans_encode_device_raw (the one-wavefront raw encoder) and the host hsrans_encode_ex (wall clock).  The device times are device
events around the call after a warm-up; the walk's host time and the block count come from the call's HSRANS_DEBUG_STAMPS line.
Prints one JSON line per configuration (and appends it to --out).  Run on the GPU box: python tools/encode_ex_rate.py"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, n = 64, 11, args.size


def device_ms(fn):
    fn()  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def stamps_of(fn):
    """the HSRANS_DEBUG_STAMPS line one call fn(context) prints to stderr (fd 2, captured in-process), on a fresh context: a context
    reads the switch when it is made"""
    os.environ["HSRANS_DEBUG_STAMPS"] = "1"
    try:
        c = H.Context(0)
    finally:
        del os.environ["HSRANS_DEBUG_STAMPS"]
    with tempfile.TemporaryFile(mode="w+b") as f:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            fn(c)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    m = re.search(r"blocks (\d+)\s+units (\d+)\s+summaries ([\d.]+) us\s+walk ([\d.]+) us\s+chain\+gather ([\d.]+) us", text)
    return dict(blocks=int(m.group(1)), units=int(m.group(2)), summaries_us=float(m.group(3)), walk_us=float(m.group(4)), chain_us=float(m.group(5))) if m else {}


for kind in ("config2", "nonstationary"):
    data = synth.enwik8_shaped(n, seed=7) if kind == "config2" else synth.nonstationary(n)
    d_in = torch.from_numpy(data).cuda()
    groups = H.index_boundaries(S, BITS, n, ctx)
    d_raw = torch.empty(H.capacity(H.RAW, S, n), dtype=torch.uint8, device="cuda")
    raw_ms = device_ms(lambda: ctx.encode_device_raw(S, BITS, d_in, d_raw, index_groups=groups, want_plan=True))
    for cont, name in ((H.BLOCK, "block_"), (H.MT, "mt_")):
        d_out = torch.empty(H.capacity(cont, S, n), dtype=torch.uint8, device="cuda")
        call = lambda c=ctx: c.encode_device_ex(cont, S, BITS, d_in, d_out, index_groups=groups, want_plan=True)  # noqa: E731
        ms = device_ms(call)
        st = stamps_of(call)
        t0 = time.perf_counter()
        host, _ = H.encode(cont, S, BITS, data, index_groups=groups)
        host_s = time.perf_counter() - t0
        m = call()[0]
        same = bool(np.array_equal(d_out[:m].cpu().numpy(), host))
        rec = dict(tool="encode_ex_rate", data=kind, container=name, states=S, bits=BITS, bytes=n, block_size=0, index="index_boundaries",
                   chain_groups=int(groups.size), device_ex_ms=round(ms, 3), device_ex_GBps=round(n / ms / 1e6, 3), raw_device_ms=round(raw_ms, 3),
                   raw_device_GBps=round(n / raw_ms / 1e6, 3), host_encode_ex_s=round(host_s, 3), speedup_vs_host=round(host_s * 1e3 / ms, 2),
                   walk_host_ms=round(st.get("walk_us", float("nan")) / 1e3, 3), walk_share=round(st.get("walk_us", float("nan")) / 1e3 / ms, 4),
                   summaries_ms=round(st.get("summaries_us", float("nan")) / 1e3, 3), chain_gather_ms=round(st.get("chain_us", float("nan")) / 1e3, 3),
                   blocks=st.get("blocks"), units=st.get("units"), stream_bytes=int(m), identical_to_host=same, device=ctx.device_name)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
