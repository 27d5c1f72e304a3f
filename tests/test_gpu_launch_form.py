"""The launch form of the feature entry points and the training path (csrc/drgnn_launch.h) on the device: the checks of
tests/test_launch_form.py on the MI355X, where a grid without blocks is skipped (launching it is an error) and a kernel
that asks for more than 64 KiB of dynamic LDS has its limit raised, and the builder's large tile against the emulation."""
import pytest

import launch_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_partly_empty_call(name, api):
    C.check_case(name, api, "cuda")


def test_iface_pairs_tile_beyond_64k_equals_emulation(api):
    from emu_api import emu
    device, host = C.check_iface_beyond_64k(api, "cuda"), C.check_iface_beyond_64k(emu(), "cpu")
    assert all(C.same_bits(device[k], host[k]) for k in host)
