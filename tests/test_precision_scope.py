"""kernels.precision_scope: a per-thread override of kernels.precision() that nests and restores,
beside the process default of kernels.set_precision (no GPU needed)."""
import threading

import pytest

from iclr_17_compression_amd import kernels
from iclr_17_compression_amd._lib import Iclr17Error


@pytest.fixture
def default_h3():
    old = kernels.precision()
    kernels.set_precision("h3")
    yield
    kernels.set_precision(old)


def test_scope_nests_and_restores(default_h3):
    assert kernels.precision() == "h3"
    with kernels.precision_scope("x6"):
        assert kernels.precision() == "x6"
        with kernels.precision_scope("fp32"):
            assert kernels.precision() == "fp32"
            with kernels.precision_scope("fp32"):
                assert kernels.precision() == "fp32"
            assert kernels.precision() == "fp32"
        assert kernels.precision() == "x6"
    assert kernels.precision() == "h3"


def test_scope_restores_on_exception(default_h3):
    with pytest.raises(ZeroDivisionError):
        with kernels.precision_scope("x6"):
            with kernels.precision_scope("bf16"):
                assert kernels.precision() == "bf16"
                1 / 0
    assert kernels.precision() == "h3"
    with kernels.precision_scope("x6"):
        with pytest.raises(ZeroDivisionError):
            with kernels.precision_scope("bf16"):
                1 / 0
        assert kernels.precision() == "x6"


def test_scope_rejects_unknown_mode(default_h3):
    with pytest.raises(Iclr17Error, match="precision must be one of"):
        with kernels.precision_scope("fp64"):
            pass
    with kernels.precision_scope("x6"):
        with pytest.raises(Iclr17Error):
            with kernels.precision_scope("X6"):
                pass
        assert kernels.precision() == "x6"   # the refused scope left the outer one alone
    assert kernels.precision() == "h3"


def test_scope_is_per_thread(default_h3):
    """A thread started inside another thread's scope reads the process default."""
    seen = {}

    def worker():
        seen["plain"] = kernels.precision()
        with kernels.precision_scope("bf16"):
            seen["own"] = kernels.precision()
        seen["after"] = kernels.precision()

    with kernels.precision_scope("x6"):
        t = threading.Thread(target=worker)
        t.start()
        t.join()
        assert kernels.precision() == "x6"   # the worker's scope did not reach this thread
    assert seen == {"plain": "h3", "own": "bf16", "after": "h3"}


def test_set_precision_inside_scope_changes_only_the_default(default_h3):
    seen = {}
    with kernels.precision_scope("x6"):
        kernels.set_precision("fp32")
        assert kernels.precision() == "x6"
        t = threading.Thread(target=lambda: seen.update(other=kernels.precision()))
        t.start()
        t.join()
    assert seen == {"other": "fp32"}
    assert kernels.precision() == "fp32"
