"""What the ABI tests and the test utilities share: the package on the import path from any start directory, and the literal-size check."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "svt-av1-1_amd", "python")))

import svtav1_hip  # noqa: E402,F401


def assert_sizes(*pairs):
    """(layout of the package, bytes) ...: a numpy dtype or ctypes Structure has the size the test states as a literal"""
    for layout, size in pairs:
        assert (layout.itemsize if isinstance(layout, np.dtype) else ctypes.sizeof(layout)) == size, (layout, size)
