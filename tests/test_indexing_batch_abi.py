"""hsrans_decode_device_indexing_batch's host side, without a GPU: the exported symbol and its declaration, the layout of its member struct
against the Python mirror (a C99 caller), the refusals that need no device, and the Python wrapper — its signature, and the type checks
that come before any C call."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

E_ARG = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hsrans_hip.h")

MEMBER = """typedef struct hsrans_indexing_member
{
  hsrans_dplan *dplan;
  const void *d_stream;
  size_t stream_length;
  void *d_out;
  size_t out_capacity;
  uint32_t index_interval;
  int rc;
  hsrans_dplan *indexed;
} hsrans_indexing_member;"""
STATS = """typedef struct hsrans_indexing_batch_stats
{
  uint32_t launches, walk_members, mt_members, tasks;
} hsrans_indexing_batch_stats;"""
ENTRY = ("int hsrans_decode_device_indexing_batch(hsrans_ctx *ctx, hsrans_indexing_member *members, uint32_t count, void *hip_stream, "
         "hsrans_indexing_batch_stats *stats);")


def _squeeze(text):
    return " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split()).replace(" ,", ",").replace(" )", ")").replace(" ;", ";")


def test_symbol_and_signature():
    L = H.load_library()
    assert hasattr(L, "hsrans_decode_device_indexing_batch")
    assert len(L.hsrans_decode_device_indexing_batch.argtypes) == 5


def test_header_declares_it_behind_the_single_call():
    text = _squeeze(open(HEADER).read())
    for want in (MEMBER, STATS, ENTRY):
        assert _squeeze(want) in text, want
    single = text.index("int hsrans_decode_device_indexing(")
    assert single < text.index("typedef struct hsrans_indexing_member") < text.index("int hsrans_decode_device_indexing_batch(")
    # directly behind it: no other declaration in between
    between = text[text.index(";", single) + 1:text.index("typedef struct hsrans_indexing_member")]
    assert between.strip() == "", between


CALLER = r"""
#include "hsrans_hip.h"
#include <stddef.h>
#include <stdio.h>

int main(void)
{
  hsrans_indexing_member members[2] = {{0}};
  hsrans_indexing_batch_stats stats = {0};
  int (*entry)(hsrans_ctx *, hsrans_indexing_member *, uint32_t, void *, hsrans_indexing_batch_stats *) = hsrans_decode_device_indexing_batch;
  stats.launches = 9;
  if (entry(NULL, members, 2, NULL, &stats) != HSRANS_E_ARG || stats.launches != 0)
    return 1;
  printf("ok %u %u %u %u\n", (unsigned)sizeof(hsrans_indexing_member), (unsigned)offsetof(hsrans_indexing_member, rc),
         (unsigned)offsetof(hsrans_indexing_member, indexed), (unsigned)sizeof(hsrans_indexing_batch_stats));
  return 0;
}
"""


def test_a_c99_caller_agrees_with_the_python_mirror_on_the_layout(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    exe = tmp_path / "caller"
    lib = os.path.join(ROOT, "hypersonic_rans_amd", "lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
           str(src), "-o", str(exe), "-L" + lib, "-lhsrans_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout, r.stderr[-2000:])
    size, at_rc, at_indexed, stats = (int(v) for v in r.stdout.split()[1:])
    assert (size, at_rc, at_indexed, stats) == (ctypes.sizeof(api.IndexingMember), api.IndexingMember.rc.offset, api.IndexingMember.indexed.offset,
                                               ctypes.sizeof(api.IndexingBatchStats))
    assert [n for n, _ in api.IndexingMember._fields_] == ["dplan", "d_stream", "stream_length", "d_out", "out_capacity", "index_interval", "rc", "indexed"]


def test_refusals_that_touch_no_device():
    L = H.load_library()
    members = (api.IndexingMember * 2)()
    fake = 0x1000  # (never dereferenced: the handles and the count come first)
    stats = api.IndexingBatchStats()
    stats.launches = 5
    assert L.hsrans_decode_device_indexing_batch(None, members, 2, None, ctypes.byref(stats)) == E_ARG  # no context
    assert stats.launches == 0
    assert L.hsrans_decode_device_indexing_batch(fake, None, 2, None, None) == E_ARG                     # no members
    assert L.hsrans_decode_device_indexing_batch(fake, members, 0, None, None) == E_ARG                  # count == 0
    assert L.hsrans_decode_device_indexing_batch(fake, members, 65_537, None, None) == E_ARG             # count > 65,536
    assert L.hsrans_decode_device_indexing_batch(None, None, 0, None, None) == E_ARG


def test_python_mirror():
    sig = inspect.signature(api.Context.decode_device_indexing_batch)
    assert list(sig.parameters) == ["self", "members", "stream", "stats"]
    assert sig.parameters["stream"].default is None and sig.parameters["stats"].default is None
    assert H.IndexingMember is api.IndexingMember and "IndexingMember" in H.__all__
    assert H.IndexingBatchStats is api.IndexingBatchStats and "IndexingBatchStats" in H.__all__


class _NoCalls:
    """stands in for the library: any C call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("C call " + name)


class _FakeCuda:
    """a CPU tensor that says it is on the GPU: the wrapper's checks read attributes only"""

    def __init__(self, t, device="cuda:0"):
        self.t = t
        self.is_cuda = True
        self.device = torch.device(device)

    def __getattr__(self, name):
        return getattr(self.t, name)


def test_wrapper_refuses_bad_members_before_any_c_call():
    ctx = object.__new__(api.Context)
    ctx.L = _NoCalls()
    plan = object.__new__(api.DevicePlan)
    plan.ctx, plan.handle, plan.owned = ctx, None, False
    stream = object()  # (given, so that torch is not asked for a current stream)
    good = _FakeCuda(torch.zeros(64, dtype=torch.uint8))

    def refused(*members):
        with pytest.raises(TypeError):
            ctx.decode_device_indexing_batch(list(members), stream=stream)

    refused((plan, torch.zeros(64, dtype=torch.uint8), good, 32))                      # the stream: not on the GPU
    refused((plan, good, torch.zeros(64, dtype=torch.uint8), 32))                      # the output: not on the GPU
    refused((plan, _FakeCuda(torch.zeros(64, dtype=torch.int32)), good, 32))           # wrongly typed
    refused((plan, good, _FakeCuda(torch.zeros(64, dtype=torch.float32)), 32))
    refused((plan, good, good))                                                        # malformed tuples
    refused((plan, good, good, 32, 64, 1))
    refused(plan)
    refused((None, good, good, 32))                                                    # not a DevicePlan
    refused((plan, good, good, 32.0))                                                  # an interval that is no integer
    refused((plan, good, good, 32), (plan, good, _FakeCuda(torch.zeros(64, dtype=torch.uint8), "cuda:1"), 32))  # two devices
