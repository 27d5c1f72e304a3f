"""The launch form of the feature entry points and the training path (csrc/drgnn_launch.h) on the host-emulation build: calls
in which one launch has an empty grid and the others have not give what the commit before the form gave, and the builder's pairs
kernel with a tile beyond 64 KiB gives the bits of the default tile.  CPU only; tests/test_gpu_launch_form.py runs the same on the
device, where the empty grid is skipped and the dynamic-LDS limit is raised."""
import pytest

import launch_cases as C


@pytest.fixture(scope="module")
def api():
    from emu_api import emu
    return emu()


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_partly_empty_call(name, api):
    C.check_case(name, api, "cpu")


def test_iface_pairs_tile_beyond_64k(api):
    C.check_iface_beyond_64k(api, "cpu")
