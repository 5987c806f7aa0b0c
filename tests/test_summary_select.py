"""CPU checks of the device get_summary's building blocks: the shared
selection header compiled for the host, and the Python entry point's
behaviour without a GPU and on the host backend."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_summary_select_matches_nth_element(tmp_path):
    """csrc/summary_select.h (key transform, radix select of the three ranks
    and their successors, column summary) built for the host with hipcc, as
    log_unit_check is: every wanted rank bitwise equal to std::nth_element for
    S in {1, 2, 3, 41, 64, 65, 1000} on normals, all-equal, three-valued,
    signed-zero, subnormal / 1e300 and strictly decreasing columns."""
    exe = tmp_path / "summary_select_check"
    inc = next(ROOT.glob("*_amd")) / "csrc"
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", f"-I{inc}",
                    str(ROOT / "tests" / "cpp" / "summary_select_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_summary_hip_backend_without_gpu_fails_loudly(P):
    """No silent host fallback: without a device the hip backend raises
    NNGP_ERR_NODEV."""
    from nngp_amd import _lib

    # the library's own view of the machine (another context-free device entry point)
    seen = P.lib.nngp_device_normals(0, 1, 0, 1, np.zeros(1))
    if seen == _lib.NNGP_OK:
        pytest.skip("GPU present")
    assert seen == _lib.NNGP_ERR_NODEV, seen  # anything else is a broken runtime, not a GPU
    x = np.random.default_rng(0).normal(size=(7, 5))
    with pytest.raises(P.NNGPError) as e:
        P.get_summary(x, backend="hip")
    assert e.value.status == 6


def test_summary_host_backend_blocks_and_offsets(P):
    """The host backend with a list of blocks and row offsets is the plain
    call on the stacked, centred matrix, bitwise; the defaults are the plain
    call; an unknown backend is refused."""
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=(4, 6)), rng.normal(size=(9, 6))
    off = rng.normal(size=13)
    want = P.get_summary(np.vstack([a, b]) - off[:, None])
    np.testing.assert_array_equal(P.get_summary([a, b], row_offset=off), want)
    np.testing.assert_array_equal(P.get_summary([a, b]), P.get_summary(np.vstack([a, b])))
    np.testing.assert_array_equal(P.get_summary(a, backend="host"), P.get_summary(a))
    with pytest.raises(ValueError):
        P.get_summary(a, backend="cuda")
