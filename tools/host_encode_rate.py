"""End-to-end encode rate with the input and the stream in host memory (BASELINE config 5 shape, the encode direction):
hsrans_encode_host_pipelined (upload / encode / download overlapped over slices) against the same work done one leg after the other
(upload, hsrans_encode_device, download), the pipeline with pageable buffers, and the host encoder (hsrans_encode_ex, one core).
mt_, 64 states, 11 bits, 64 KiB independent blocks, enwik8-shaped input.  Every line carries bit_exact against hsrans_encode_device.
Run on the GPU box: python tools/host_encode_rate.py [--sizes N,...] [--intervals 0,32] [--modes serial,pipelined,pageable,host] > profiles/r09_host_encode_rate.jsonl
Trace of the pipelined 2^30-byte case (profiles/r09_host_encode_*.csv, r09_host_encode_overlap.txt):
rocprofv3 --kernel-trace --memory-copy-trace --stats --output-format csv -d <dir> -o r09 -- python tools/host_encode_rate.py --sizes 1073741824
--intervals 0 --modes pipelined --slices 0 --reps 3, then python tools/trace_overlap.py <dir> 16"""
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
from hypersonic_rans_amd import synth

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default=f"{1 << 30},100000000")
ap.add_argument("--intervals", default="0,32")
ap.add_argument("--modes", default="serial,pipelined,pageable,host")
ap.add_argument("--slices", default="0,2,4,8,16")
ap.add_argument("--reps", type=int, default=8)
args = ap.parse_args()
modes = set(args.modes.split(","))
S, BITS, BLOCK = 64, 11, 1 << 16
ctx = H.Context(0)
L = H.load_library()


def timed(fn, reps):
    fn()  # warm-up (buffers grown, kernels loaded)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print("   runs ms:", " ".join(f"{t * 1e3:.1f}" for t in ts), file=sys.stderr)
    return min(ts), sum(ts) / len(ts)


def line(mode, n, interval, m, best, mean, exact, **extra):
    print(json.dumps({"mode": mode, "size": n, "states": S, "bits": BITS, "block_size": BLOCK, "index_interval": interval, "compressed": m,
                      "ms_best": round(best * 1e3, 2), "ms_mean": round(mean * 1e3, 2), "input_GB_s": round(n / best / 1e9, 2),
                      "bit_exact": bool(exact), **extra}), flush=True)


for n in (int(v) for v in args.sizes.split(",")):
    t0 = time.perf_counter()
    data = synth.enwik8_shaped(n, seed=20241008)
    print(f"input {n} bytes made in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    h_in = torch.from_numpy(data).pin_memory()
    cap = H.capacity(H.MT, S, n)
    h_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
    d_in = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    for interval in (int(v) for v in args.intervals.split(",")):
        # what hsrans_encode_device writes for the same bytes in HBM: the yardstick of every line
        d_in.copy_(h_in)
        r = ctx.encode_device(H.MT, S, BITS, d_in, d_out, block_size=BLOCK, index_interval=interval, want_plan=interval != 0)
        m = r[0] if interval else r
        want = d_out[:m].cpu()
        pcap = L.hsrans_plan_capacity(H.MT, S, n, interval, BLOCK) if interval else 1
        want_plan = torch.from_numpy(ctx.read_device_plan(r[1], capacity=pcap)) if interval else None
        del r
        h_plan = torch.empty(pcap, dtype=torch.uint8).pin_memory()

        if "serial" in modes:
            def serial():
                d_in.copy_(h_in, non_blocking=True)
                rr = ctx.encode_device(H.MT, S, BITS, d_in, d_out, block_size=BLOCK, index_interval=interval, want_plan=interval != 0)
                k = rr[0] if interval else rr
                h_out[:k].copy_(d_out[:k], non_blocking=True)
                if interval:
                    psz = L.hsrans_dplan_read_plan(rr[1].handle, h_plan.data_ptr(), h_plan.numel())
                    assert psz == want_plan.numel()
                torch.cuda.synchronize()
                return k
            h_out.fill_(0)
            k = serial()
            exact = k == m and torch.equal(h_out[:m], want) and (not interval or torch.equal(h_plan[: want_plan.numel()], want_plan))
            best, mean = timed(serial, args.reps)
            line("serial: upload, encode_device, download", n, interval, m, best, mean, exact)

        def run_pipe(src, dst, plan_buf, k):
            """the C entry on raw buffers (torch tensors or numpy arrays); returns (stream length, plan bytes)"""
            ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data
            size = lambda a: a.numel() if isinstance(a, torch.Tensor) else a.size
            opts = H.api.EncodeOpts(BLOCK, interval, ptr(plan_buf) if interval else None, size(plan_buf) if interval else 0, 0, H.api.ENC_INDEPENDENT_BLOCKS, 0, None, 0)
            got = L.hsrans_encode_host_pipelined(ctx.handle, H.MT, S, BITS, ptr(src), size(src), ptr(dst), size(dst), ctypes.byref(opts), k)
            assert got != 0, "hsrans_encode_host_pipelined failed"
            return got, opts.plan_size

        def plan_ok(plan_buf, psize):
            if not interval:
                return True
            got = plan_buf[:psize] if isinstance(plan_buf, np.ndarray) else plan_buf[:psize].numpy()
            return psize == want_plan.numel() and np.array_equal(got, want_plan.numpy())

        if "pipelined" in modes:  # every buffer page-locked, the stream's and the plan's included (as the serial mode's)
            for k in (int(v) for v in args.slices.split(",")):
                h_out.fill_(0)
                got, psize = run_pipe(h_in, h_out, h_plan, k)
                exact = got == m and torch.equal(h_out[:m], want) and plan_ok(h_plan, psize)
                best, mean = timed(lambda: run_pipe(h_in, h_out, h_plan, k), args.reps)
                line(f"pipelined, {k} slices", n, interval, m, best, mean, exact, pinned=True)

        if "pageable" in modes:  # every buffer pageable (numpy)
            p_in, p_out, p_plan = data, np.zeros(cap, np.uint8), np.zeros(pcap, np.uint8)
            got, psize = run_pipe(p_in, p_out, p_plan, 0)
            exact = got == m and np.array_equal(p_out[:m], want.numpy()) and plan_ok(p_plan, psize)
            best, mean = timed(lambda: run_pipe(p_in, p_out, p_plan, 0), args.reps)
            line("pipelined, 0 slices, pageable buffers", n, interval, m, best, mean, exact, pinned=False)
            del p_out, p_plan

        if "host" in modes and n <= 100_000_000:
            res = H.encode(H.MT, S, BITS, data, block_size=BLOCK, index_interval=interval, independent_blocks=True)
            stream = res[0] if interval else res
            exact = stream.size == m and np.array_equal(stream, want.numpy()) and (not interval or np.array_equal(res[1], want_plan.numpy()))
            best, mean = timed(lambda: H.encode(H.MT, S, BITS, data, block_size=BLOCK, index_interval=interval, independent_blocks=True), min(args.reps, 3))
            line("host encoder (hsrans_encode_ex, one core)", n, interval, m, best, mean, exact)
    del h_in, h_out, d_in, d_out
    torch.cuda.empty_cache()
