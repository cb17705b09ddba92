"""The helpers every entry of hypersonic_rans_amd/api.py is written with, without a GPU: the handle owners' close / __del__ on a stub
library that counts destroy calls, the structure-to-dict conversion, and the checks the three *_indirect calls share (CPU tensors; no
library call is reached)."""
import types

import pytest
import torch

from hypersonic_rans_amd import api


class Counting:
    """a stand-in for the loaded library: every hsrans_*_destroy counts its calls (and raises where told to)"""

    def __init__(self, raises=False):
        self.calls, self.raises = [], raises

    def __getattr__(self, name):
        def destroy(handle):
            self.calls.append((name, handle))
            if self.raises:
                raise OSError("destroy failed")
        return destroy


def stub_ctx(**kw):
    return types.SimpleNamespace(L=Counting(**kw), handle=1)


@pytest.mark.parametrize("make,destroy", (
    (lambda c: api.DevicePlan(c, 7), "hsrans_dplan_destroy"),
    (lambda c: api.Batch(c, 7, []), "hsrans_dplan_batch_destroy"),
    (lambda c: api.GatherSet(c, 7, [], []), "hsrans_gather_set_destroy"),
    (lambda c: api.Planes(c, 7, api.PlanesDesc(), []), "hsrans_planes_destroy"),
    (lambda c: api.PlanesGather(c, 7, None, None), "hsrans_planes_gather_destroy"),
))
def test_close_twice_destroys_once(make, destroy):
    ctx = stub_ctx()
    obj = make(ctx)
    obj.close()
    obj.close()
    assert ctx.L.calls == [(destroy, 7)] and obj.handle is None
    obj.__del__()
    del obj
    assert ctx.L.calls == [(destroy, 7)]


def test_del_destroys_what_was_not_closed():
    ctx = stub_ctx()
    api.DevicePlan(ctx, 9).__del__()
    assert ctx.L.calls == [("hsrans_dplan_destroy", 9)]


def test_every_owner_names_its_destroy_function():
    for cls, name in ((api.Context, "hsrans_ctx_destroy"), (api.Comm, "hsrans_comm_destroy"), (api.Queue, "hsrans_queue_destroy"),
                      (api.Sharded, "hsrans_sharded_destroy")):
        assert issubclass(cls, api._Handle) and cls._destroy == name
        assert "close" not in vars(cls) and "__del__" not in vars(cls)
    # an object whose constructor raised before it had a handle closes without a call
    ctx = stub_ctx()
    q = api.Queue.__new__(api.Queue)
    q.ctx = ctx
    q.close()
    q.__del__()
    assert ctx.L.calls == []


def test_unowned_device_plan_never_destroys():
    ctx = stub_ctx()
    view = api.DevicePlan(ctx, 7, owned=False)
    view.close()
    assert view.handle is None
    view.__del__()
    api.DevicePlan(ctx, 8, owned=False).__del__()
    assert ctx.L.calls == []


def test_a_destroy_that_raises_does_not_escape_del():
    ctx = stub_ctx(raises=True)
    obj = api.DevicePlan(ctx, 7)
    obj.__del__()
    assert ctx.L.calls == [("hsrans_dplan_destroy", 7)]
    with pytest.raises(OSError):  # close() itself does not hide it
        api.DevicePlan(ctx, 8).close()


def test_launch_info_dict():
    plan = dict(container=api.RAW, states=64, bits=11, flags=2 | 4, decoded_len=100_000_000, n_chains=8192, n_pieces=8192, shared_hist=1)
    name, info = api.launch_choice(plan, persistent=1, table_mode=3)
    assert name == "hsrans::k_decode_direct<3>"
    assert list(info) == [n for n, _ in api.LaunchInfo._fields_]
    weights = info["class_weights"]
    assert type(weights) is list and len(weights) == 8 and all(type(w) is int for w in weights)
    assert all(type(v) is int for n, v in info.items() if n != "class_weights")


def test_gather_set_info_dict():
    info = api.GatherSetInfo(members=3, launches=2)
    kinds = [n for n, _ in api.GatherSetInfo._fields_ if n.startswith("kind_")]
    assert len(kinds) == 6
    for i, n in enumerate(kinds):
        getattr(info, n)[:] = [10 * i + k for k in range(6)]
    d = api._as_dict(info)
    assert list(d) == [n for n, _ in api.GatherSetInfo._fields_]
    assert d["members"] == 3 and d["launches"] == 2 and type(d["members"]) is int
    for i, n in enumerate(kinds):
        assert type(d[n]) is list and d[n] == [10 * i + k for k in range(6)] and all(type(v) is int for v in d[n])
    stats = api._as_dict(api.EncodeExBatchStats(launches=4, plans_us=1.5))
    assert stats["launches"] == 4 and type(stats["plans_us"]) is float and list(stats) == [n for n, _ in api.EncodeExBatchStats._fields_]
    assert all(type(v) is int for v in api._as_dict(api.QueueStats(submitted=2 ** 40)).values())


class CudaLike:
    """what _indirect_args looks at of a tensor, claiming to be on a GPU: a CPU tensor underneath, no device call"""

    def __init__(self, t):
        self.t, self.is_cuda = t, True

    def __getattr__(self, name):
        return getattr(self.t, name)


@pytest.mark.parametrize("columns", (3, 4))
def test_indirect_checks(columns):
    ranges_text = f"d_ranges: a contiguous CUDA tensor (N, {columns}) of int64 or uint64"
    good = CudaLike(torch.zeros((5, columns), dtype=torch.int64))
    scratch = CudaLike(torch.zeros(256, dtype=torch.uint8))
    cases = [
        ("not on a GPU", dict(d_ranges=torch.zeros((5, columns), dtype=torch.int64)), TypeError, ranges_text),
        ("columns", dict(d_ranges=CudaLike(torch.zeros((5, 7 - columns), dtype=torch.int64))), TypeError, ranges_text),
        ("one dimension", dict(d_ranges=CudaLike(torch.zeros(5 * columns, dtype=torch.int64))), TypeError, ranges_text),
        ("dtype", dict(d_ranges=CudaLike(torch.zeros((5, columns), dtype=torch.int32))), TypeError, ranges_text),
        ("a view", dict(d_ranges=CudaLike(torch.zeros((5, 2 * columns), dtype=torch.int64)[:, ::2])), TypeError, ranges_text),
        ("count on the host", dict(d_ranges=good, count=torch.zeros(1, dtype=torch.int32)), TypeError, "count: a CUDA int32 or uint32 scalar tensor"),
        ("count of 64 bits", dict(d_ranges=good, count=CudaLike(torch.zeros(1, dtype=torch.int64))), TypeError, "count: a CUDA int32 or uint32 scalar tensor"),
        ("two counts", dict(d_ranges=good, count=CudaLike(torch.zeros(2, dtype=torch.int32))), TypeError, "count: a CUDA int32 or uint32 scalar tensor"),
        ("max_count", dict(d_ranges=good, max_count=6), ValueError, "max_count is larger than d_ranges"),
        ("workspace on the host", dict(d_ranges=good, workspace=torch.zeros(256, dtype=torch.uint8)), TypeError, "workspace: a contiguous CUDA uint8 tensor"),
        ("workspace dtype", dict(d_ranges=good, workspace=CudaLike(torch.zeros(64, dtype=torch.int32))), TypeError, "workspace: a contiguous CUDA uint8 tensor"),
    ]
    for what, kw, exc, text in cases:
        with pytest.raises(exc) as e:
            api._indirect_args(kw["d_ranges"], columns, kw.get("count"), kw.get("max_count"), kw.get("workspace", scratch), None, torch.device("cpu"), None)
        assert type(e.value) is exc and str(e.value) == text, what
    # the order of the checks: d_ranges before count before max_count before the workspace
    with pytest.raises(TypeError) as e:
        api._indirect_args(torch.zeros((5, columns), dtype=torch.int64), columns, torch.zeros(1), 9, torch.zeros(1), None, torch.device("cpu"), None)
    assert str(e.value) == ranges_text
    with pytest.raises(TypeError) as e:
        api._indirect_args(good, columns, torch.zeros(1), 9, torch.zeros(1), None, torch.device("cpu"), None)
    assert str(e.value) == "count: a CUDA int32 or uint32 scalar tensor"
    with pytest.raises(ValueError):
        api._indirect_args(good, columns, None, 9, torch.zeros(1), None, torch.device("cpu"), None)
    # what passes: max_count defaults to the rows, a given one is kept, the caller's workspace comes back
    count = CudaLike(torch.zeros(1, dtype=torch.uint32))
    assert api._indirect_args(good, columns, count, None, scratch, None, torch.device("cpu"), None) == (5, scratch)
    assert api._indirect_args(good, columns, None, 2, scratch, None, torch.device("cpu"), None) == (2, scratch)
    assert api._indirect_args(CudaLike(torch.zeros((0, columns), dtype=torch.uint64)), columns, None, None, scratch, None, torch.device("cpu"), None) == (0, scratch)
