"""hsrans_encode_device_ex_batch on the CPU side: exported by the built library, prototyped in include/hsrans_hip.h, callable from C99,
and refusing what needs no GPU to refuse."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HSRANS_E_ARG = 2

CALLER = r"""
#include "hsrans_hip.h"
#include <stddef.h>
#include <stdio.h>

int main(void)
{
  hsrans_encode_ex_member members[2] = {{0}};
  hsrans_encode_ex_batch_stats stats = {0};
  hsrans_encode_opts opts = {0};
  hsrans_dplan *plans[2] = {NULL, NULL};
  int (*entry)(hsrans_ctx *, hsrans_encode_ex_member *, uint32_t, void *, hsrans_dplan **, hsrans_encode_ex_batch_stats *) = hsrans_encode_device_ex_batch;
  members[0].container = HSRANS_BLOCK;
  members[0].states = 64;
  members[0].bits = 11;
  members[0].stream_length = 7;
  members[1].container = HSRANS_MT;
  members[1].states = 32;
  members[1].bits = 12;
  members[1].opts = &opts;
  members[1].stream_length = 7;
  opts.plan_size = 9;
  stats.launches = 3;
  /* no context: refused before anything is launched, every stream_length cleared, every rc the refusal */
  if (entry(NULL, members, 2, NULL, plans, &stats) != HSRANS_E_ARG || members[0].stream_length != 0 || members[1].stream_length != 0)
    return 1;
  if (members[0].rc != HSRANS_E_ARG || members[1].rc != HSRANS_E_ARG || opts.plan_size != 0)
    return 2;
  if (stats.launches != 0 || plans[0] != NULL || plans[1] != NULL)
    return 3;
  printf("ok %u %u %u %u\n", (unsigned)sizeof(hsrans_encode_ex_member), (unsigned)offsetof(hsrans_encode_ex_member, stream_length),
         (unsigned)offsetof(hsrans_encode_ex_member, rc), (unsigned)sizeof(hsrans_encode_ex_batch_stats));
  return 0;
}
"""


def test_encode_device_ex_batch_is_exported_and_prototyped():
    import hypersonic_rans_amd as H

    L = H.load_library()
    assert hasattr(L, "hsrans_encode_device_ex_batch")
    with open(os.path.join(ROOT, "include", "hsrans_hip.h")) as f:
        text = f.read()
    assert "int hsrans_encode_device_ex_batch(hsrans_ctx *ctx, hsrans_encode_ex_member *members, uint32_t count, void *hip_stream," in text
    assert "} hsrans_encode_ex_member;" in text and "} hsrans_encode_ex_batch_stats;" in text


def test_a_c99_caller_of_encode_device_ex_batch_compiles_links_and_agrees_on_the_layout(tmp_path):
    import hypersonic_rans_amd as H

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
    size, at_length, at_rc, stats = (int(v) for v in r.stdout.split()[1:])
    # the Python mirrors have the C layout
    M = H.api.EncodeExMember
    assert (size, at_length, at_rc, stats) == (ctypes.sizeof(M), M.stream_length.offset, M.rc.offset, ctypes.sizeof(H.api.EncodeExBatchStats))


def test_encode_device_ex_batch_refuses_without_a_gpu():
    import hypersonic_rans_amd as H

    L = H.load_library()
    members = (H.api.EncodeExMember * 3)()
    for m in members:
        m.container, m.states, m.bits, m.stream_length, m.rc = H.BLOCK, 64, 11, 99, 0
    stats = H.api.EncodeExBatchStats()
    stats.launches = 5
    plans = (ctypes.c_void_p * 3)(1, 2, 3)
    # a NULL context
    assert L.hsrans_encode_device_ex_batch(None, members, 3, None, plans, ctypes.byref(stats)) == HSRANS_E_ARG
    assert [m.stream_length for m in members] == [0, 0, 0] and [m.rc for m in members] == [HSRANS_E_ARG] * 3
    assert stats.launches == 0 and [p for p in plans] == [None, None, None]
    # count == 0 and NULL members (no context needed to refuse them)
    assert L.hsrans_encode_device_ex_batch(None, members, 0, None, None, None) == HSRANS_E_ARG
    assert L.hsrans_encode_device_ex_batch(None, None, 3, None, None, None) == HSRANS_E_ARG
    # more than 65,536 members
    assert L.hsrans_encode_device_ex_batch(None, members, 65537, None, None, None) == HSRANS_E_ARG
