"""Child process of test_deterministic_gpu.py::test_det_library_parity: the parity tests named on the command line (pytest node
ids, optionally `-k`), run as they stand -- their own assertion bodies and tolerances -- in a process that has loaded
libbear_hip_det.so (BEAR_AMD_DETERMINISTIC=1 at import).  Refuses to start under any other library."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv):
    sys.path.insert(0, ROOT)
    from bear_amd import _lib
    assert _lib.lib().bear_deterministic_build() == 1, "not the deterministic build: " + _lib.LIB_PATH
    print("DET_LIBRARY " + _lib.LIB_PATH, flush=True)
    import pytest
    return int(pytest.main(["-m", "gpu", "-q", "-rfEs"] + list(argv)))


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
