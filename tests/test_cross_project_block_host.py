"""The block form of the projecting cross-sector kernel, the parts that need no device (ls_amd_cross_apply_block_path,
ls_amd_cross_block_kernel_name_path, CrossSectorPlan.apply_block(method=), evolve.thermal_correlation(block_method=)): the ABI and
the build, and what is refused before a plan or a device is looked at -- an unknown path, K outside [1, 64], a bad method."""
import os
import re

import pytest

import cross_groups_reference as G
import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import evolve
from distributed_matvec_amd.evolve import thermal_correlation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")


def test_abi_makefile_and_python_names():
    from distributed_matvec_amd import _lib

    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib.load()
    for name in ("ls_amd_cross_apply_block_path", "ls_amd_cross_block_kernel_name_path"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    m = re.search(r"enum \{ LS_AMD_CROSS_BLOCK_AUTO = (\d+), LS_AMD_CROSS_BLOCK_COLUMNS = (\d+), LS_AMD_CROSS_BLOCK_KERNEL = (\d+) \}", header)
    assert m and [int(v) for v in m.groups()] == [D.CrossSectorPlan.BLOCK_METHODS[k] for k in (None, "columns", "kernel")]
    make = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_cross_project_blk.hip" in ksrc and "k_cross_project_blk_fermi.hip" in ksrc
    assert re.search(r"^k_cross_project_blk\.o k_cross_project_blk_fermi\.o.*: k_cross_project_blk_t\.hpp k_cross_project_t\.hpp "
                     r"k_cross_blk_t\.hpp k_cross_t\.hpp lsk_fermi\.hpp$", make, re.M)
    lsk = open(os.path.join(CSRC, "lsk.h"), encoding="utf-8").read()
    for name in ("lsk_cross_project_blk", "lsk_cross_project_blk_fermi", "lsk_cross_project_blk_kernel_name", "lsk_cross_project_blk_fermi_kernel_name"):
        assert re.search(r"\b%s\(" % name, lsk), name
    assert evolve.PROJECT_BLOCK_METHOD in ("columns", "kernel")


def test_the_kernel_has_no_floating_point_atomics_and_the_chunk_of_its_sibling():
    """a (row, column) is summed in registers in a fixed order: the template adds nothing atomically but the packet counter of
    cross_wave_slot and the error flag, and takes kCrossKC, the loads and the grid from k_cross_blk_t.hpp"""
    text = open(os.path.join(CSRC, "k_cross_project_blk_t.hpp"), encoding="utf-8").read()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "atomicAdd" not in code and re.findall(r"atomic\w+", code) == ["atomicExch"]
    assert '#include "k_cross_blk_t.hpp"' in text and "cross_blk_grid(" in code and "cross_blk_load<" in code
    assert "kCrossKC =" not in code and "asm" not in code


def test_the_path_and_K_are_refused_before_the_plan():
    """no plan can exist on a machine without a device: the two refusals that need none come first, then the NULL plan"""
    from distributed_matvec_amd import _lib

    L = _lib.load()
    for path in (-1, 3, 17):
        assert L.ls_amd_cross_apply_block_path(None, path, 1, None, 1, 0, None, 1, 0, None) == -1
        msg = L.ls_amd_last_error()
        assert b"unknown path %d" % path in msg and b"LS_AMD_CROSS_BLOCK_AUTO, LS_AMD_CROSS_BLOCK_COLUMNS or LS_AMD_CROSS_BLOCK_KERNEL" in msg
        assert L.ls_amd_cross_block_kernel_name_path(None, path, 1) is None
        assert b"unknown path %d" % path in L.ls_amd_last_error()
    for path in (0, 1, 2):
        for K in (0, 65, -3):
            assert L.ls_amd_cross_apply_block_path(None, path, K, None, 1, 0, None, 1, 0, None) == -1
            assert b"K = %d is outside [1, 64]" % K in L.ls_amd_last_error()
            assert L.ls_amd_cross_block_kernel_name_path(None, path, K) is None
            assert b"K = %d is outside [1, 64]" % K in L.ls_amd_last_error()
        assert L.ls_amd_cross_apply_block_path(None, path, 64, None, 1, 0, None, 1, 0, None) == -1
        assert b"NULL plan" in L.ls_amd_last_error()
        assert L.ls_amd_cross_block_kernel_name_path(None, path, 1) is None
        assert b"NULL plan" in L.ls_amd_last_error()


def test_a_bad_method_is_refused_before_any_device_work():
    plan = D.CrossSectorPlan.__new__(D.CrossSectorPlan)  # no handle, no device: the method is looked at first
    for bad in ("rows", "Kernel", "", 2, True, b"kernel"):
        with pytest.raises(ValueError, match="none of None .*'columns', 'kernel'"):
            plan.apply_block(None, None, method=bad)
        with pytest.raises(ValueError, match="none of None .*'columns', 'kernel'"):
            plan.block_kernel(8, bad)


def test_thermal_correlation_refuses_a_bad_block_method_before_any_device_work():
    src, dst = X.ring(8, 4, 0), X.ring(8, 4, 3)
    bonds = [[i, (i + 1) % 8] for i in range(8)]
    cfg = {"basis": src["basis"], "observables": [G.sz_site(0)], "hamiltonian": {"name": "H", "terms": [
        {"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}
    for bad in ("rows", "auto", 1, False):
        with pytest.raises(ValueError, match="block_method = .* is none of None, 'columns', 'kernel'"):
            thermal_correlation(cfg, 0, 0.5, [0.0, 1.0], target=dst, groups="project", block_method=bad)
