"""The refusals of the update entry points (update_refusals.py) on the emulation build and on the product library.  No GPU:
every refused call returns before a device call, and the product library answers host-only calls without one."""
import pytest

from update_refusals import REFUSALS, VALID, case_id, check_refusal, check_valid


def _api(build):
    if build == "emu":
        from emu_api import emu
        return emu()
    from deeprank_gnn_amd import _lib
    return _lib.get()


@pytest.mark.parametrize("build", ["emu", "hip"])
@pytest.mark.parametrize("case", REFUSALS, ids=case_id)
def test_refusal(case, build):
    check_refusal(_api(build), build, case)


@pytest.mark.parametrize("case", VALID, ids=case_id)
def test_valid_call_on_the_emulation_build(case):
    check_valid(_api("emu"), case)
