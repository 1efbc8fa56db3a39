"""For the few GPU tests whose buffers only fit an idle device."""
import pytest

from topdogspectrumanalyser_amd import DeviceBuffer
from topdogspectrumanalyser_amd._native import TdsaError


def room_or_skip(nbytes, device=0):
    """A DeviceBuffer of nbytes; skips the test only when the device has no room for it, any other failure raises."""
    try:
        return DeviceBuffer(nbytes, device)
    except TdsaError as e:
        if "out of memory" not in str(e).lower():
            raise
        pytest.skip(f"no room for {nbytes} bytes on the device")
