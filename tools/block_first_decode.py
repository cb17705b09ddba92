"""The first decode of a block_ (or, --container mt, an mt_) stream without an index, and what it leaves behind.  One 100 MB enwik8-shaped
input, 64 states, 11 bits, adaptive blocks from the host encoder (byte-identical to the reference's stream).  Legs, rotated, wall clock around
each call including its synchronisation, the decoded bytes compared on every leg of every repetition:
  device  a  decode_device with the base plan (block_: the walk plan, one wavefront follows the inline headers; mt_: one chain per block,
             planned on the device)
          b  decode_device_indexing at interval 64: the same pass, recording; the indexed plan assembled on the device
          c  the same in a context made under HSRANS_INDEX_ASSEMBLE_ON_HOST=1 (records down, blob built by one core, blob up)
          d  decode_device with the plan b left
  host    e  decode_host, first call on the stream (the context's index cache holds another stream's index)
          f  decode_host, later calls
          g  decode_host with plan= the hsrans_index_build blob
          h  hsrans_index_build at interval 64 from the host copy of the stream
  parent  a, b, e, f, h against another build of the library (HSRANS_PARENT_LIB=<path to the parent commit's libhsrans_hip.so>), in the same
          rotation: the "before" figures.  Left out when the variable is not set.
  direct  a, b of THIS build through the same bare ctypes calls the parent legs make (the package's wrappers add some 50 us to a call of
          a few hundred): what parent a and b compare with.  e, f and h are bare calls for both builds already.
The two roles are not equal: on mt_ the library in the "parent" role measured 3 % (a), 18 % (b) and 11 % (h) faster than the one under test
whichever build it was (profiles/r15_first_decode_refactor_mt*.jsonl).  For a comparison of two builds run it a second time with the roles
swapped (HSRANS_LIB=<parent> HSRANS_PARENT_LIB=<this build>): the builds differ by the square root of the quotient of the two ratios.
One JSON line per leg (median and quartiles over the repetitions), then one line of ratios.  Run on the GPU box:
  python tools/block_first_decode.py [--container block|mt] [--size N] [--reps R] [--out profiles/r14_block_first_decode.jsonl]"""
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
ap.add_argument("--size", type=int, default=100_000_000)
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--container", choices=("block", "mt"), default="block")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_%s_first_decode.jsonl" % args.container)
CONTAINER = H.BLOCK if args.container == "block" else H.MT
assert args.reps >= 16, "medians and quartiles of at least 16 repetitions"
n, S, BITS, INTERVAL = args.size, 64, 11, 64

data = synth.enwik8_shaped(n)
stream = np.ascontiguousarray(H.encode(CONTAINER, S, BITS, data))
other = np.ascontiguousarray(H.encode(CONTAINER, S, BITS, data[: 2 << 20][::-1].copy()))  # another stream of >= 1 MiB: decoding it replaces the cached index
m = stream.size
d_in = torch.from_numpy(np.concatenate([stream, np.zeros((-m) % 16, np.uint8)])).cuda()
d_ref = torch.from_numpy(data).cuda()
d_out = torch.zeros(n, dtype=torch.uint8, device="cuda")
cur = torch.cuda.current_stream().cuda_stream

ctx = H.Context(0)
os.environ["HSRANS_INDEX_ASSEMBLE_ON_HOST"] = "1"
ctx_host_asm = H.Context(0)  # (the switch is read when a context is made)
del os.environ["HSRANS_INDEX_ASSEMBLE_ON_HOST"]
walk_blob = H.plan_build(CONTAINER, S, BITS, stream)
walk = ctx.make_device_plan_from_stream(CONTAINER, S, BITS, d_in, m, n)
walk_c = ctx_host_asm.make_device_plan(walk_blob) if CONTAINER == H.BLOCK else ctx_host_asm.make_device_plan_from_stream(CONTAINER, S, BITS, d_in, m, n)
index_blob = ctx.index_build(CONTAINER, S, BITS, stream, INTERVAL)
index_room = np.zeros(index_blob.size + 4096, np.uint8)
state = {"indexed": None}


class Parent:
    """the few entries the parent legs need, straight through ctypes (the package's classes are bound to the library under test); also
    made for the library under test itself: the "direct" legs"""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        vp, sz, u32, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
        L.hsrans_ctx_create.argtypes = [i, ctypes.POINTER(vp)]
        L.hsrans_dplan_create.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
        L.hsrans_decode_device.argtypes = [vp, vp, vp, sz, vp, sz, vp]
        L.hsrans_dplan_status.argtypes = [vp, vp, ctypes.POINTER(u32)]
        L.hsrans_decode_host.restype = sz
        L.hsrans_decode_host.argtypes = [vp, i, i, u32, vp, sz, vp, sz, vp, sz]
        L.hsrans_dplan_create_from_device_stream.argtypes = [vp, i, i, u32, vp, sz, sz, vp, ctypes.POINTER(vp)]
        L.hsrans_decode_device_indexing.argtypes = [vp, vp, vp, sz, vp, sz, u32, vp, ctypes.POINTER(vp)]
        L.hsrans_dplan_destroy.restype = None
        L.hsrans_dplan_destroy.argtypes = [vp]
        L.hsrans_index_build.restype = sz
        L.hsrans_index_build.argtypes = [vp, i, i, u32, vp, sz, u32, vp, sz]
        self.ctx, self.walk = vp(), vp()
        assert L.hsrans_ctx_create(0, ctypes.byref(self.ctx)) == 0
        if CONTAINER == H.BLOCK:
            assert L.hsrans_dplan_create(self.ctx, walk_blob.ctypes.data, walk_blob.size, ctypes.byref(self.walk)) == 0
        else:
            assert L.hsrans_dplan_create_from_device_stream(self.ctx, CONTAINER, S, BITS, d_in.data_ptr(), m, n, ctypes.c_void_p(cur), ctypes.byref(self.walk)) == 0

    def decode_device(self):
        assert self.L.hsrans_decode_device(self.ctx, self.walk, d_in.data_ptr(), m, d_out.data_ptr(), n, ctypes.c_void_p(cur)) == 0

    def decode_device_indexing(self):
        indexed = ctypes.c_void_p()
        assert self.L.hsrans_decode_device_indexing(self.ctx, self.walk, d_in.data_ptr(), m, d_out.data_ptr(), n, INTERVAL, ctypes.c_void_p(cur), ctypes.byref(indexed)) == 0
        self.L.hsrans_dplan_destroy(indexed)

    def decode_host(self, s, out):
        return self.L.hsrans_decode_host(self.ctx, CONTAINER, S, BITS, s.ctypes.data, s.size, out.ctypes.data, out.size, None, 0)


parent = Parent(os.environ["HSRANS_PARENT_LIB"]) if os.environ.get("HSRANS_PARENT_LIB") else None
direct = Parent(H.lib_path()) if parent is not None else None
h_out = np.zeros(n, np.uint8)
h_other = np.zeros(2 << 20, np.uint8)
L = H.load_library()


def host_call(handle_lib, handle, s, out, plan=None):
    return handle_lib.hsrans_decode_host(handle, CONTAINER, S, BITS, s.ctypes.data, s.size, out.ctypes.data, out.size, None if plan is None else plan.ctypes.data,
                                         0 if plan is None else plan.size)


def leg_a():
    ctx.decode_device(walk, d_in, d_out, stream_length=m)


def leg_b():
    if state["indexed"] is not None:
        state["indexed"].close()
    state["indexed"] = ctx.decode_device_indexing(walk, d_in, d_out, INTERVAL, stream_length=m)


def leg_c():
    ctx_host_asm.decode_device_indexing(walk_c, d_in, d_out, INTERVAL, stream_length=m).close()


def leg_d():
    ctx.decode_device(state["indexed"], d_in, d_out, stream_length=m)


def host_leg(lib, handle, plan=None):
    def run():
        assert host_call(lib, handle, stream, h_out, plan) == n
    return run


def index_leg(lib, handle):
    def run():
        got = lib.hsrans_index_build(handle, CONTAINER, S, BITS, stream.ctypes.data, stream.size, INTERVAL, index_room.ctypes.data, index_room.size)
        assert got == index_blob.size and np.array_equal(index_room[:got], index_blob)
    return run


def evict(lib, handle):
    def run():
        assert host_call(lib, handle, other, h_other) == h_other.size
    return run


# (name, library, what, un-timed step before it, timed call, where the bytes land)
LEGS = [("a", "this", "decode_device, base plan", None, leg_a, "device"),
        ("b", "this", "decode_device_indexing, interval 64, assembled on the device", None, leg_b, "device"),
        ("c", "this", "decode_device_indexing, interval 64, HSRANS_INDEX_ASSEMBLE_ON_HOST=1", None, leg_c, "device"),
        ("d", "this", "decode_device, the plan b left", None, leg_d, "device"),
        ("e", "this", "decode_host, first call", evict(L, ctx.handle), host_leg(L, ctx.handle), "host"),
        ("f", "this", "decode_host, later call", None, host_leg(L, ctx.handle), "host"),
        ("g", "this", "decode_host, plan= the hsrans_index_build blob", None, host_leg(L, ctx.handle, index_blob), "host"),
        ("h", "this", "index_build, interval 64", None, index_leg(L, ctx.handle), None)]
if parent is not None:
    LEGS += [("a", "direct", "decode_device, base plan", None, direct.decode_device, "device"),
             ("b", "direct", "decode_device_indexing, interval 64, assembled on the device", None, direct.decode_device_indexing, "device"),
             ("a", "parent", "decode_device, base plan", None, parent.decode_device, "device"),
             ("b", "parent", "decode_device_indexing, interval 64, assembled on the device", None, parent.decode_device_indexing, "device"),
             ("h", "parent", "index_build, interval 64", None, index_leg(parent.L, parent.ctx), None),
             ("e", "parent", "decode_host, first call", evict(parent.L, parent.ctx), lambda: parent.decode_host(stream, h_out) == n or sys.exit("parent decode_host failed"), "host"),
             ("f", "parent", "decode_host, later call", None, lambda: parent.decode_host(stream, h_out) == n or sys.exit("parent decode_host failed"), "host")]

times = {(name, lib): [] for name, lib, *_ in LEGS}
leg_b()  # (d needs a plan before b's first turn in a rotated order; f needs e's index)
host_leg(L, ctx.handle)()
for rep in range(args.reps + 1):  # (the first round warms buffers and code objects up and is dropped)
    order = LEGS[rep % len(LEGS):] + LEGS[:rep % len(LEGS)]
    for name, lib, _, before, call, where in order:
        if name == "f":  # a later call is one that follows a call on the same stream
            host_leg(L, ctx.handle)() if lib == "this" else parent.decode_host(stream, h_out)
        if before is not None:
            before()
        if where == "device":
            d_out.zero_()
        elif where == "host":
            h_out[:] = 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert where is None or (torch.equal(d_out, d_ref) if where == "device" else np.array_equal(h_out, data)), (name, lib)
        if rep:
            times[(name, lib)].append(dt * 1e3)
assert ctx.status(walk) == 0 and ctx.status(state["indexed"]) == 0 and ctx.host_index_chains() > 100

med = {}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for name, lib, what, *_ in LEGS:
        q1, q2, q3 = (float(v) for v in np.percentile(times[(name, lib)], (25, 50, 75)))
        med[(name, lib)] = q2
        line = {"leg": name, "library": lib, "what": what, "median_ms": round(q2, 4), "q1_ms": round(q1, 4), "q3_ms": round(q3, 4), "iqr_ms": round(q3 - q1, 4),
                "reps": len(times[(name, lib)]), "size": n, "stream": int(m), "states": S, "bits": BITS, "interval": INTERVAL, "container": args.container}
        if name == "d":
            line["launch"] = state["indexed"].launch_info()
            line["chains"] = line["launch"]["chains"]
        f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)
    ratios = {"b_over_a": med[("b", "this")] / med[("a", "this")], "c_over_b": med[("c", "this")] / med[("b", "this")], "d_ms": med[("d", "this")],
              "f_over_g": med[("f", "this")] / med[("g", "this")], "e_over_f": med[("e", "this")] / med[("f", "this")]}
    if parent is not None:
        ratios.update({"b_over_parent_a": med[("b", "this")] / med[("a", "parent")], "a_over_parent_a": med[("a", "direct")] / med[("a", "parent")],
                       "b_over_parent_b": med[("b", "direct")] / med[("b", "parent")], "h_over_parent_h": med[("h", "this")] / med[("h", "parent")],
                       "f_over_parent_f": med[("f", "this")] / med[("f", "parent")], "e_over_parent_e": med[("e", "this")] / med[("e", "parent")]})
    line = {"ratios": {k: round(v, 4) for k, v in ratios.items()}, "device": ctx.device_name,
            "note": "wall clock around each call including its synchronisation; legs rotated; medians over the repetitions after one dropped round"}
    f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
