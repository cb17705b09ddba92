"""Every HsransError that stems from a C return code carries it as ``.code``: one refusal per entry that the host checks before anything
is launched (include/hsrans_hip.h: a stream that is not 16-byte aligned, a plan that is a batch member twice, a destination the ranges do
not fit, an output below elem_size * elements are HSRANS_E_ARG), on a stream of a few KiB.  Nothing a refused call was given is written."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

pytestmark = pytest.mark.gpu

E_ARG = 2
N = 4102  # bytes; 2051 16-bit elements


def test_refusals_carry_the_documented_code(gpu_ctx):
    data = synth.enwik8_shaped(N, seed=11)
    s, plan = H.encode(H.RAW, 64, 11, data, index_interval=32)
    padded = torch.from_numpy(np.concatenate([np.zeros(16, np.uint8), s, np.zeros((-s.size) % 16, np.uint8)])).cuda()
    d_stream, d_odd = padded[16:], padded[15:-1]  # (d_odd: one byte off a 16-byte boundary; the call is refused before the bytes matter)
    dplans = [gpu_ctx.make_device_plan(plan) for _ in range(2)]
    out = torch.full((N,), 0xCC, dtype=torch.uint8, device="cuda")

    def refused(call, *args, **kw):
        with pytest.raises(H.HsransError) as e:
            call(*args, **kw)
        assert e.value.code == E_ARG and str(e.value).endswith(f"failed with code {E_ARG}"), (call.__name__, str(e.value), e.value.code)

    refused(gpu_ctx.decode_device, dplans[0], d_odd, out, stream_length=s.size)
    refused(gpu_ctx.make_batch, [dplans[0], dplans[0]])
    batch = gpu_ctx.make_batch(dplans)
    refused(gpu_ctx.decode_device_batch, batch, [d_stream, d_odd], [out, out.clone()], stream_lengths=[s.size, s.size])
    refused(gpu_ctx.decode_device_gather, dplans[0], d_stream, [(0, 100, N - 99)], out, stream_length=s.size)  # one byte past the destination

    t = torch.from_numpy(data.view(np.int16)).cuda()
    frame = torch.empty(H.planes_capacity(2, 64, t.numel()), dtype=torch.uint8, device="cuda")
    work = torch.empty(H.planes_workspace_bytes(2, t.numel()), dtype=torch.uint8, device="cuda")
    _, desc, plans = gpu_ctx.encode_device_planes(t, frame, work)
    planes = gpu_ctx.make_planes(desc, plans)
    small = torch.full((t.numel() - 8,), 0x4CCC, dtype=torch.int16, device="cuda")
    refused(gpu_ctx.decode_device_planes, planes, frame, small, work)

    torch.cuda.synchronize()
    assert bool((out == 0xCC).all()) and bool((small == 0x4CCC).all())
    assert gpu_ctx.status(dplans[0]) == 0 and gpu_ctx.batch_status(batch) == [0, 0] and gpu_ctx.planes_status(planes) == [0, 0]
    # and the calls that were refused go through with arguments that pass
    gpu_ctx.decode_device(dplans[0], d_stream, out, stream_length=s.size)
    back = torch.empty_like(t)
    gpu_ctx.decode_device_planes(planes, frame, back, work)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), data) and torch.equal(back, t)
