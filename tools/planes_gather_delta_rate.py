"""The three delta gathers — hsrans_decode_device_planes_gather_indirect_delta, _gather_batch_delta and _gather_batch_indirect_delta — each
against its plain twin and against the route a caller had without them, in ONE process on one MI355X.  K in {8, 32, 128} bf16 / fp32
tensors of 1 MiB, tuned = base * (1 + 0.01 * N(0, 1)), K / 4 distinct bases shared four ways, coded against their bases in one
encode_device_planes_delta_batch (64 states, 11 bits, 64 KiB blocks, a checkpoint every 32 groups, stored planes allowed); every tensor is
read as a table of rows of 1024 elements; 1 % and 10 % of each tensor's rows, at random row indices, are fetched into one packed
destination.  Per configuration and entry, on the same buffers:
  (d) the delta entry: the tensors' rows;
  (a) its plain twin on the same rows: the residues' rows — what the XOR in the merge costs on top of it;
  (b) today's route to the tensors' rows: the plain twin into a scratch, torch.index_select of the same rows of the bases, torch.bitwise_xor
      (every buffer allocated beforehand; the row indices already on the device).
The one-frame entry fetches member 0's rows alone.  --sets buffer sets are rotated; HIP events around each leg; median and interquartile
range of --reps repetitions after a warm-up of every set.  Every leg's output is compared before it is timed.  Prints one JSON line per
configuration and appends it to --out.  Ratios are recorded, not gated.
Run on the GPU box: python tools/planes_gather_delta_rate.py --out profiles/r25_planes_gather_delta_rate.jsonl"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import hypersonic_rans_amd as H

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--sets", type=int, default=3)
ap.add_argument("--counts", type=int, nargs="+", default=[8, 32, 128])
ap.add_argument("--shares", type=float, nargs="+", default=[0.01, 0.1])
ap.add_argument("--log2-bytes", type=int, default=20, help="bytes of one tensor (20: 1 MiB)")
ap.add_argument("--row-elements", type=int, default=1024)
ap.add_argument("--out", default=None)
args = ap.parse_args()
ctx = H.Context(0)
S, BITS, BLOCK, INTERVAL = 64, 11, 1 << 16, 32
P, ROW = args.sets, args.row_elements
INT = {2: torch.int16, 4: torch.int32}


def spread(ms):
    q1, med, q3 = np.percentile(ms, (25, 50, 75))
    return [round(float(med) * 1e3, 2), round(float(q3 - q1) * 1e3, 2), round(float(q1) * 1e3, 2), round(float(q3) * 1e3, 2)]  # microseconds


def timed_device(fn):
    """fn(set) queues work on the current stream: microseconds between two events around it"""
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


def as_items(x, name):
    """float32 values as the tensor's items: fp32 as they are, bf16 truncated to the top 16 bits"""
    return x.view(torch.int32) if name == "fp32" else (x.view(torch.int32) >> 16).to(torch.int16)


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def legs(plain, delta, route, outs, want, want_residue, after):
    """the three legs of one entry, each checked on every buffer set and then timed: {leg: spread}"""
    got = {}
    for leg, fn, expect in (("a_plain_us", plain, want_residue), ("d_delta_us", delta, want), ("b_route_us", route, want)):
        for o in outs:
            o.zero_()
        for i in range(P):
            fn(i)
        torch.cuda.synchronize()
        after(leg)
        for o in outs:
            assert torch.equal(o.view(expect.shape), expect), leg
        got[leg] = timed_device(fn)
    got["delta_over_plain"] = round(got["d_delta_us"][0] / got["a_plain_us"][0], 3)
    got["delta_over_route"] = round(got["d_delta_us"][0] / got["b_route_us"][0], 3)
    got["delta_below_route_ranges_apart"] = got["d_delta_us"][3] < got["b_route_us"][2]
    got["plain_below_delta_ranges_apart"] = got["a_plain_us"][3] < got["d_delta_us"][2]
    return got


for name, W in (("bf16", 2), ("fp32", 4)):
    n = (1 << args.log2_bytes) // W
    table_rows = n // ROW
    assert n == table_rows * ROW, "a tensor is a whole number of rows"
    for K in args.counts:
        assert K % 4 == 0
        gen = torch.Generator(device="cuda").manual_seed(41 + K)
        base_values = [torch.randn(n, generator=gen, device="cuda", dtype=torch.float32) for _ in range(K // 4)]
        bases = [as_items(b, name) for b in base_values]
        tensors = [as_items(base_values[k // 4] * (1 + 0.01 * torch.randn(n, generator=gen, device="cuda", dtype=torch.float32)), name) for k in range(K)]
        member_bases = [bases[k // 4] for k in range(K)]  # one base shared four ways
        del base_values
        cap = H.planes_capacity(W, S, n)
        enc_work = torch.empty(H.planes_batch_workspace_bytes([W] * K, [n] * K), dtype=torch.uint8, device="cuda")
        frames = [[torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(K)] for _ in range(P)]
        got = ctx.encode_device_planes_delta_batch(tensors, member_bases, frames[0], enc_work, states=S, bits=BITS, block_size=BLOCK, index_interval=INTERVAL,
                                                   store_incompressible=True)
        for i in range(1, P):
            for k in range(K):
                frames[i][k].copy_(frames[0][k])
        descs, plans = [g[1] for g in got], [g[2] for g in got]
        plane_bytes = sum(int(d.length[p]) for d in descs for p in range(W))  # (what a packed frame holds, but for its 16-byte rounding)
        pset = ctx.make_planes_set(descs, plans)
        pgss = [ctx.make_planes_gather_set(pset, f) for f in frames]
        bss = [ctx.make_planes_base_set(x, member_bases) for x in pgss]
        planes0 = ctx.make_planes(descs[0], plans[0])
        pg0 = [ctx.make_planes_gather(planes0, f[0]) for f in frames]
        n_coded = sum(p is not None for pl in plans for p in pl)
        tensor_table = torch.cat(tensors).view(K * table_rows, ROW)
        base_table = torch.cat(bases).view(K // 4 * table_rows, ROW)

        for share in args.shares:
            count = max(1, int(table_rows * share))  # rows of each tensor
            rng = np.random.default_rng(1000 * K + int(share * 1000))
            picked = [rng.permutation(table_rows)[:count] for _ in range(K)]
            common = dict(tool="tools/planes_gather_delta_rate.py", tensor=f"{name}: base * (1 + 0.01 N(0,1)) against its base", members=K, distinct_bases=K // 4, elements=n,
                          elem_size=W, codec=f"mt_ rANS32x64 16w {BITS}", block_size=BLOCK, index_interval=INTERVAL, store_incompressible=True, coded_planes=n_coded,
                          stored_planes=K * W - n_coded, plane_bytes_over_tensor_bytes=round(plane_bytes / (K * n * W), 4), row_elements=ROW, share_of_rows=share,
                          rows_per_tensor=count, us="[median, interquartile range, first quartile, third quartile]", reps=args.reps, sets_rotated=P,
                          # what the merge kernel moves for 16 W output bytes: planes in and elements out, and with a base its 16 W bytes in as well
                          merge_kernel_bytes_delta_over_plain=1.5,
                          checked="every leg's rows before it is timed: the delta entry's and the route's == the tensors' rows, the plain twin's == the residues' rows")

            for entry, members in (("hsrans_decode_device_planes_gather_batch_delta", K), ("hsrans_decode_device_planes_gather_batch_indirect_delta", K),
                                   ("hsrans_decode_device_planes_gather_indirect_delta", 1)):
                N = members * count
                rows = np.asarray([(k, int(r) * ROW, ROW, (k * count + j) * ROW) for k in range(members) for j, r in enumerate(picked[k])], np.uint64)
                d_tensor_rows = torch.from_numpy(np.concatenate([k * table_rows + picked[k] for k in range(members)]).astype(np.int64)).cuda()
                d_base_rows = torch.from_numpy(np.concatenate([k // 4 * table_rows + picked[k] for k in range(members)]).astype(np.int64)).cuda()
                want = tensor_table[d_tensor_rows]
                want_residue = want ^ base_table[d_base_rows]
                outs = [torch.zeros(N, ROW, dtype=INT[W], device="cuda") for _ in range(P)]
                scratch = [torch.zeros(N, ROW, dtype=INT[W], device="cuda") for _ in range(P)]
                base_rows = [torch.zeros(N, ROW, dtype=INT[W], device="cuda") for _ in range(P)]

                def finish_route(i):
                    torch.index_select(base_table, 0, d_base_rows, out=base_rows[i])
                    torch.bitwise_xor(scratch[i], base_rows[i], out=outs[i])

                if members == 1:  # one frame, ranges on the device
                    wb = H.planes_gather_workspace_bytes(W, N, N * ROW)
                    d_ranges = [torch.from_numpy(np.ascontiguousarray(rows[:, 1:]).view(np.int64)).cuda() for _ in range(P)]
                    control = [torch.empty(H.planes_gather_indirect_workspace_bytes(W, N), dtype=torch.uint8, device="cuda") for _ in range(P)]
                    kw = dict(max_count=N, max_elements=N * ROW)

                    def plain(i, to=outs):
                        ctx.decode_device_planes_gather_indirect(pg0[i], d_ranges[i], to[i].view(-1), works[i], workspace=control[i], **kw)

                    def delta(i):
                        ctx.decode_device_planes_gather_indirect_delta(pg0[i], d_ranges[i], member_bases[0], outs[i].view(-1), works[i], workspace=control[i], **kw)

                    def after(leg):
                        assert all(ctx.planes_gather_refused(x) == 0 for x in pg0) and ctx.planes_gather_status(pg0[0]) == [0] * W, leg
                else:
                    wb = H.planes_gather_batch_workspace_bytes(W, N, N * ROW)
                    d_rows = [torch.from_numpy(np.ascontiguousarray(rows[:, [1, 2, 3, 0]]).view(np.int64)).cuda() for _ in range(P)]
                    control = [torch.empty(H.planes_gather_batch_indirect_workspace_bytes(n_coded, W, N), dtype=torch.uint8, device="cuda") for _ in range(P)]
                    if "indirect" in entry:
                        def plain(i, to=outs):
                            ctx.decode_device_planes_gather_batch_indirect(pgss[i], d_rows[i], to[i], works[i], workspace=control[i])

                        def delta(i):
                            ctx.decode_device_planes_gather_batch_indirect_delta(pgss[i], bss[i], d_rows[i], outs[i], works[i], workspace=control[i])
                    else:
                        def plain(i, to=outs):
                            ctx.decode_device_planes_gather_batch(pgss[i], rows, to[i], works[i])

                        def delta(i):
                            ctx.decode_device_planes_gather_batch_delta(pgss[i], bss[i], rows, outs[i], works[i])

                    def after(leg):
                        assert all(ctx.planes_gather_set_refused(x) == 0 for x in pgss) and ctx.planes_gather_set_status(pgss[0]) == [0] * K, leg

                works = [torch.zeros(wb, dtype=torch.uint8, device="cuda") for _ in range(P)]

                def route(i):
                    plain(i, to=scratch)
                    finish_route(i)

                emit(dict(common, entry=entry, rows=N, fetched_bytes=N * ROW * W, **legs(plain, delta, route, outs, want, want_residue, after)))
                del outs, scratch, base_rows, works, control, want, want_residue
        for x in bss + pg0 + [planes0] + pgss + [pset]:
            x.close()
        for pl in plans:
            for p in pl:
                if p is not None:
                    p.close()
        del frames, pgss, bss, pg0, tensors, bases, member_bases, enc_work, tensor_table, base_table
        torch.cuda.empty_cache()
