"""CPU-side checks of the batched solve: the initial-state normaliser, the C-ABI declarations
and the build of the batch kernel's translation unit for gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from raocp.core.solver import normalise_initial_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raocp-toolbox_amd")


def test_normalise_initial_states_shapes():
    a = np.arange(12.0).reshape(4, 3)
    out = normalise_initial_states(a, 3)
    assert out.shape == (4, 3) and out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
    assert np.array_equal(out, a)
    assert np.array_equal(normalise_initial_states(a.reshape(4, 3, 1), 3), a)
    assert np.array_equal(normalise_initial_states([1, 2, 3], 3), np.array([[1.0, 2.0, 3.0]]))
    assert normalise_initial_states(a[:, ::-1], 3).flags["C_CONTIGUOUS"]


@pytest.mark.parametrize("bad", [np.zeros((4, 2)), np.zeros((4, 4)), np.zeros(4), np.zeros((4, 3, 2)),
                                 np.zeros((0, 3)), np.zeros((2, 2, 3, 1))])
def test_normalise_initial_states_rejects(bad):
    with pytest.raises(ValueError):
        normalise_initial_states(bad, 3)


def test_header_declares_batch_entry_points():
    text = open(os.path.join(ROOT, "include", "raocp_hip.h")).read()
    for name in ("raocp_cp_batch_run", "raocp_cp_batch_get", "raocp_cp_batch_first_inputs"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*raocp_ctx\s*\*", text), name


def test_batch_kernel_unit_is_in_the_build_and_compiles(tmp_path):
    # what `make all` would run from scratch: the unit is compiled and its object is linked
    cmds = subprocess.run(["make", "-C", PKG, "-n", "-B", "all"], capture_output=True, text=True, check=True).stdout
    link = [line for line in cmds.splitlines() if " -shared " in line]
    assert len(link) == 1 and "/raocp_cpb.o" in link[0].split(" -o ")[0], link
    assert any(" -c csrc/raocp_cpb.hip " in line for line in cmds.splitlines())
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the batch kernel cannot be built")
    out = tmp_path / "raocp_cpb.o"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-c",
                    os.path.join(PKG, "csrc", "raocp_cpb.hip"), "-o", str(out)], check=True)
    assert out.stat().st_size > 0
