import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")


@pytest.fixture(scope="session")
def oracle():
    from oracle_lib import Oracle

    return Oracle()


@pytest.fixture(scope="session")
def ref():
    """The real reference's results for the tests' seeded inputs, replayed from tests/golden/reference_calls.json.gz: the same in
    every checkout, with or without the reference's sources.  HSRANS_REF_RECORD=<path> (tests/golden/make_golden.py) answers every
    call with the compiled reference (oracle/_ref/libhsrans_ref.so) instead and writes what it returned to <path>."""
    from oracle_lib import RecordedRef, Ref

    record = os.environ.get("HSRANS_REF_RECORD")
    r = RecordedRef(live=Ref() if record else None)
    yield r
    if record:
        r.save(record)


@pytest.fixture(scope="session")
def gpu_ctx():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (the product has no CPU fallback)")
    import hypersonic_rans_amd as H

    return H.Context(0)
