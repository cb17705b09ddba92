"""The block choice of hsrans_encode_device_ex — unit summaries and every unit's own code length computed on the device, the walk on the
host — against the host encoder's, decision by decision: every block's begin, end, single flag, symbol and normalised histogram."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    zipf = synth.enwik8_shaped(1 << 20, seed=11)
    nonstat = synth.nonstationary(3_000_000)
    runs = np.concatenate([np.full(70_000, 7, np.uint8), zipf[:100_000], np.full(200_000, 200, np.uint8), zipf[:33]])
    out = {f"zipf[:{n}]": zipf[:n] for n in (65537, 65560, 65599, 65600, 131073, 524300)}
    out.update(zipf=zipf, nonstat=nonstat, runs=runs, one=np.full(300_000, 42, np.uint8), tiny=zipf[:27], drift=synth.nonstationary(4_000_000, seed=5))
    return out


@pytest.mark.parametrize("container", (H.BLOCK, H.MT))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (10, 11, 12, 13, 14, 15))
def test_device_walk_decisions_equal_the_host_walk(gpu_ctx, inputs, container, states, bits):
    for name, data in inputs.items():
        d_in = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        for block_size in (0, 65536):
            host = H.block_choices(container, states, bits, data, block_size=block_size)
            dev = gpu_ctx.block_choices_device(container, states, bits, d_in, block_size=block_size)
            assert host.size == dev.size, (name, block_size, host.size, dev.size)
            for f in ("begin", "end", "single", "symbol", "counts"):
                assert np.array_equal(host[f], dev[f]), (name, block_size, f, int(np.argmax(np.any((host[f] != dev[f]).reshape(host.size, -1), axis=1))))
        if container == H.MT and name in ("nonstat", "runs", "drift"):
            assert host.size > 1
