"""hsrans_encode_host_pipelined on the CPU side: exported by the built library, prototyped in include/hsrans_hip.h, callable from C99,
and a call without a context refused before anything is touched."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLER = r"""
#include "hsrans_hip.h"
#include <stdio.h>
#include <string.h>

int main(void)
{
  static uint8_t in[4096], out[1 << 16];
  hsrans_encode_opts opts;
  size_t (*entry)(hsrans_ctx *, int, int, uint32_t, const uint8_t *, size_t, uint8_t *, size_t, hsrans_encode_opts *, uint32_t) =
      hsrans_encode_host_pipelined;
  size_t k;
  memset(&opts, 0, sizeof(opts));
  memset(out, 0x5A, sizeof(out));
  opts.block_size = 1024;
  opts.flags = HSRANS_ENC_INDEPENDENT_BLOCKS;
  /* no context: refused before anything is launched, nothing written */
  if (entry(NULL, HSRANS_MT, 64, 11, in, sizeof(in), out, sizeof(out), &opts, 0) != 0)
    return 1;
  for (k = 0; k < sizeof(out); k++)
    if (out[k] != 0x5A)
      return 2;
  printf("ok\n");
  return 0;
}
"""


def test_encode_host_pipelined_is_exported_and_prototyped():
    import hypersonic_rans_amd as H

    L = H.load_library()
    assert hasattr(L, "hsrans_encode_host_pipelined")
    with open(os.path.join(ROOT, "include", "hsrans_hip.h")) as f:
        text = f.read()
    assert "size_t hsrans_encode_host_pipelined(hsrans_ctx *ctx, int container, int states, uint32_t bits, const uint8_t *in, size_t length, uint8_t *out," in text
    assert "size_t out_capacity, hsrans_encode_opts *opts, uint32_t n_slices);" in text


def test_a_c99_caller_of_encode_host_pipelined_compiles_and_links(tmp_path):
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    exe = tmp_path / "caller"
    lib = os.path.join(ROOT, "hypersonic_rans_amd", "lib")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-isystem", "/opt/rocm/include",
           str(src), "-o", str(exe), "-L" + lib, "-lhsrans_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])


def test_encode_host_pipelined_refuses_a_null_context_and_leaves_out_untouched():
    import hypersonic_rans_amd as H

    L = H.load_library()
    data = np.arange(100_000, dtype=np.uint32).astype(np.uint8)
    out = np.full(H.capacity(H.MT, 64, data.size), 0xA5, np.uint8)
    plan = np.full(1 << 16, 0xA5, np.uint8)
    opts = H.api.EncodeOpts(1 << 16, 32, plan.ctypes.data, plan.size, 0, H.api.ENC_INDEPENDENT_BLOCKS, 0, None, 0)
    n = L.hsrans_encode_host_pipelined(None, H.MT, 64, 11, data.ctypes.data, data.size, out.ctypes.data, out.size, ctypes.byref(opts), 0)
    assert n == 0 and opts.plan_size == 0
    assert np.all(out == 0xA5) and np.all(plan == 0xA5)
