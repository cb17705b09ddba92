"""hsrans_encode_device_ex on the CPU side: exported by the built library, prototyped in include/hsrans_hip.h, callable from C99."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CALLER = r"""
#include "hsrans_hip.h"
#include <stdio.h>

int main(void)
{
  hsrans_encode_opts opts = {0};
  size_t (*entry)(hsrans_ctx *, int, int, uint32_t, const void *, size_t, void *, size_t, const hsrans_hist *, hsrans_encode_opts *, void *,
                  hsrans_dplan **) = hsrans_encode_device_ex;
  opts.block_size = 0;
  /* no context: refused before anything is launched */
  if (entry(NULL, HSRANS_MT, 64, 11, NULL, 0, NULL, 0, NULL, &opts, NULL, NULL) != 0)
    return 1;
  printf("ok\n");
  return 0;
}
"""


def test_encode_device_ex_is_exported_and_prototyped():
    import hypersonic_rans_amd as H

    L = H.load_library()
    assert hasattr(L, "hsrans_encode_device_ex")
    with open(os.path.join(ROOT, "include", "hsrans_hip.h")) as f:
        assert "size_t hsrans_encode_device_ex(hsrans_ctx *ctx, int container, int states, uint32_t bits" in f.read()


def test_a_c99_caller_of_encode_device_ex_compiles_and_links(tmp_path):
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


def test_encode_device_ex_refuses_a_null_context_without_a_gpu():
    import hypersonic_rans_amd as H

    L = H.load_library()
    opts = H.api.EncodeOpts()
    n = L.hsrans_encode_device_ex(None, H.MT, 64, 11, None, 0, None, 0, None, ctypes.byref(opts), None, None)
    assert n == 0


def test_host_block_choices_tile_the_input():
    """hsrans_block_choices: the host encoder's block choice, contiguous, codable (counts sum to 2^bits), single blocks of one symbol."""
    import numpy as np

    import hypersonic_rans_amd as H
    from hypersonic_rans_amd import synth

    data = synth.nonstationary(3_000_000)
    for container in (H.BLOCK, H.MT):
        for bits in (11, 14):
            for block_size in (0, 65536):
                ch = H.block_choices(container, 64, bits, data, block_size=block_size)
                assert ch["begin"][0] == 0 and ch["end"][-1] == data.size
                assert np.array_equal(ch["begin"][1:], ch["end"][:-1])
                for c in ch:
                    if c["single"]:
                        assert np.all(data[c["begin"]: c["end"]] == c["symbol"])
                    else:
                        assert int(c["counts"].sum()) == 1 << bits
            if container == H.MT:
                assert ch.size > 1
