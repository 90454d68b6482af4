"""CPU: libslamhip.so asks for its hardware queues when it loads (include/slam_hip.h: slam_hw_queues_requested).

The HIP runtime reads GPU_MAX_HW_QUEUES once per process, so the library's load-time initialiser decides once per process too: every
case runs in a fresh child interpreter.  The initialiser changes the C environment; Python's ``os.environ`` is a snapshot taken at
interpreter start and does not show that, so the child asks libc's ``getenv`` through ctypes."""
import json
import os
import subprocess
import sys

import pytest

from slam_decomposition_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# as tests/test_abi.py: only a machine without ROCm (a hosted CI runner) may lack the library
pytestmark = pytest.mark.skipif(
    not os.path.exists(_ffi.LIB_PATH) and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no ROCm toolchain on this machine"
)

UNSET = None
RAISED = [UNSET, "4", "8", "abc", ""]  # unset, below 16 or not a number: becomes 16
KEPT = ["16", "24", "32"]
ALL_INPUTS = RAISED + KEPT + ["64"]

_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from slam_decomposition_amd import _ffi
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
libc.getenv.argtypes = [ctypes.c_char_p]
before = libc.getenv(b"GPU_MAX_HW_QUEUES")
lib = _ffi.load_library()
after = libc.getenv(b"GPU_MAX_HW_QUEUES")
dec = lambda b: None if b is None else b.decode()
print(json.dumps({"requested": int(lib.slam_hw_queues_requested()), "binding": _ffi.hw_queues_requested(), "before": dec(before),
                  "after": dec(after)}))
"""


def _load(hwq, own=UNSET):
    """Load the library in a fresh interpreter with GPU_MAX_HW_QUEUES = hwq and SLAM_HW_QUEUES = own (None = unset)."""
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "SLAM_HW_QUEUES")}
    if hwq is not UNSET:
        env["GPU_MAX_HW_QUEUES"] = hwq
    if own is not UNSET:
        env["SLAM_HW_QUEUES"] = own
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["before"] == hwq  # the child really started from the input under test
    assert out["binding"] == out["requested"]
    return out


def _written_values_stay_in_range(out):
    if out["after"] != out["before"]:  # the library wrote the variable: a plain number from 4 to 32
        assert out["after"].isdigit() and 4 <= int(out["after"]) <= 32, out


@pytest.mark.parametrize("hwq", RAISED)
def test_unset_low_or_unparsable_becomes_16(hwq):
    out = _load(hwq)
    assert out["requested"] == 16 and out["after"] == "16", out


@pytest.mark.parametrize("hwq", KEPT)
def test_16_to_32_is_kept(hwq):
    out = _load(hwq)
    assert out["requested"] == int(hwq) and out["after"] == hwq, out


def test_a_value_above_32_is_neither_raised_nor_written():
    out = _load("64")
    assert out["requested"] == 64 and out["after"] == "64", out
    for own in ("24", "33", "2", "x"):
        out = _load("64", own)
        assert out["requested"] == 64 and out["after"] == "64", (own, out)


@pytest.mark.parametrize("hwq", ALL_INPUTS)
def test_opt_out_leaves_the_environment_alone(hwq):
    out = _load(hwq, "0")
    assert out["requested"] == 0 and out["after"] == hwq, out


@pytest.mark.parametrize("hwq, want", [(UNSET, 24), ("4", 24), ("abc", 24), ("16", 24), ("24", 24), ("32", 32)])
def test_own_number_is_asked_for_instead_of_16_and_never_lowers(hwq, want):
    out = _load(hwq, "24")
    assert out["requested"] == want and out["after"] == str(want), out
    _written_values_stay_in_range(out)


def test_own_number_may_be_as_low_as_4():
    out = _load(UNSET, "4")
    assert out["requested"] == 4 and out["after"] == "4", out
    out = _load("8", "4")  # never lowered
    assert out["requested"] == 8 and out["after"] == "8", out


@pytest.mark.parametrize("own", ["2", "33", "x"])
@pytest.mark.parametrize("hwq", ALL_INPUTS)
def test_an_own_number_out_of_range_behaves_like_unset(own, hwq):
    out, ref = _load(hwq, own), _load(hwq)
    assert (out["requested"], out["after"]) == (ref["requested"], ref["after"]), (out, ref)
    _written_values_stay_in_range(out)


def test_loading_still_fails_loudly_at_the_first_entry_point_without_a_gpu():
    """The initialiser makes no HIP call: the library loads on a machine without a GPU, and the first real entry point raises
    (tests/test_abi.py::test_no_gpu_fails_loudly), with the queues already asked for."""
    code = (
        "import ctypes, sys; sys.path.insert(0, sys.argv[1])\n"
        "from slam_decomposition_amd import _ffi\n"
        "lib = _ffi.load_library()\n"
        "assert lib.slam_hw_queues_requested() == 16\n"
        "n = ctypes.c_int(-1)\n"
        "rc = lib.slam_device_count(ctypes.byref(n))\n"
        "if rc == 0 and n.value > 0:\n"
        "    _ffi.Context(0).close(); print('gpu'); sys.exit(0)\n"
        "try:\n"
        "    _ffi.Context(0)\n"
        "except _ffi.SlamHipError as e:\n"
        "    print('raised', e.code); sys.exit(0)\n"
        "sys.exit('no GPU and no error')\n"
    )
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "SLAM_HW_QUEUES")}
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert p.stdout.strip().splitlines()[-1].split()[0] in ("raised", "gpu")
