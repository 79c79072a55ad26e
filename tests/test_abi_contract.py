"""The host layer's contract, device-free: every workspace size and every refusal (return code and dgp_last_error() text) equals
what tests/abi_contract.json records (scripts/abi_contract.py --write, from the build before the entry points moved next to
their kernels).  Equality is exact."""
import os
import sys

import pytest

from discontinuum_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import abi_contract  # noqa: E402


@pytest.fixture(scope="module")
def fixture():
    return abi_contract.load(os.path.join(ROOT, "tests", "abi_contract.json"))


def test_workspace_sizes_are_unchanged(fixture):
    got = abi_contract.record_sizes(_lib.load())
    assert len(got) == len(fixture["sizes"]) >= 39
    diffs = list(abi_contract.differences(fixture["sizes"], got))
    assert not diffs, "\n".join(diffs[:20])


def test_refusals_are_unchanged(fixture):
    """A check for the machine WITHOUT a GPU: every recorded call passes null device addresses and must be refused, so with no
    device a wrongly accepted call can never become a launch."""
    import torch

    if torch.cuda.is_available() or os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is visible: the refusal table is checked on the machine without one")
    got = abi_contract.record_refusals(_lib.load())
    assert len(got) == len(fixture["refusals"]) >= 665
    diffs = list(abi_contract.differences(fixture["refusals"], got))
    assert not diffs, "\n".join(diffs[:20])
