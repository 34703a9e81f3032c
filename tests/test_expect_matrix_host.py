"""Matrix elements between blocks of sector states, the parts that need no device (ls_amd_expect_matrix_elements,
ExpectationPlan.matrix_elements, expectation.matrix_elements, expectation.eigenstate_matrix_elements): the ABI and the build, the
compiler's resource report against the table of DESIGN.md section 6j, the polarisation identity on dense matrices, and the arguments
refused before a device is asked for."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import expectation
from distributed_matvec_amd.expectation import eigenstate_matrix_elements, matrix_elements  # noqa: F401  (the feature under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")


def test_abi_makefile_and_python_names():
    from distributed_matvec_amd import _lib

    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib.load()
    for name in ("ls_amd_expect_matrix_elements", "ls_amd_expect_matrix_kernel_name"):
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
        assert name in open(os.path.join(ROOT, "distributed-matvec_amd", "_lib.py"), encoding="utf-8").read()
    make = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_expect_mat.hip" in ksrc and "k_expect_mat_fermi.hip" in ksrc
    assert re.search(r"^k_expect_mat\.o k_expect_mat_fermi\.o k_expect_mat_ablate\.o k_expect_mat_fermi_ablate\.o: "
                     r"k_expect_mat_t\.hpp k_expect_blk_t\.hpp k_expect_t\.hpp k_corr_t\.hpp k_cross_t\.hpp lsk_fermi\.hpp$", make, re.M)
    # the rule of the block form is what it was
    assert re.search(r"^k_expect_blk\.o k_expect_blk_fermi\.o k_expect_blk_ablate\.o k_expect_blk_fermi_ablate\.o: "
                     r"k_expect_blk_t\.hpp k_expect_t\.hpp k_corr_t\.hpp k_cross_t\.hpp lsk_fermi\.hpp$", make, re.M)
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_expect" not in isa
    for name in ("matrix_elements", "matrix_kernel"):
        assert hasattr(D.ExpectationPlan, name), name
    for name in ("matrix_elements", "eigenstate_matrix_elements"):
        assert name in expectation.__all__ and name in D.__all__ and getattr(D, name) is getattr(expectation, name), name


def test_the_matrix_kernel_reuses_the_block_stages_without_floating_point_atomics():
    def code_of(header):
        src = open(os.path.join(CSRC, header), encoding="utf-8").read()
        return "\n".join(line.split("//")[0] for line in src.splitlines())

    code = code_of("k_expect_mat_t.hpp")
    assert '#include "k_expect_blk_t.hpp"' in code
    # ... and the headers it takes its stages and constants from
    for header in ("k_expect_mat_t.hpp", "k_expect_t.hpp", "k_corr_t.hpp"):
        assert "atomicAdd" not in code_of(header) and "unsafeAtomicAdd" not in code_of(header), header
    assert "expect_blk_fold<NC>(" in code and "corr_grid(n)" in code and "lsk_corr_sum(" in code and "kExpKC" in code
    assert re.search(r"constexpr int kExpMatKA = [48];", code)
    for unit, fermi in (("k_expect_mat.hip", False), ("k_expect_mat_fermi.hip", True)):
        text = open(os.path.join(CSRC, unit), encoding="utf-8").read()
        assert ("expect_mat_launch<true>" in text) == fermi and ("expect_mat_launch<false>" in text) == (not fermi)
        assert ('"k_expect_mat_fermi"' in text) == fermi


def test_null_plan_is_refused_by_the_library():
    """the entry points answer a NULL plan with a message (no device is touched)"""
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert L.ls_amd_expect_matrix_elements(None, 1, 2, None, 2, 1, 2, None, 2, 1, None, None) == -1
    assert b"ls_amd_expect_matrix_elements: NULL plan" in L.ls_amd_last_error()
    assert L.ls_amd_expect_matrix_kernel_name(None, 1, 1) is None
    assert b"ls_amd_expect_matrix_kernel_name: NULL plan" in L.ls_amd_last_error()


def test_polarisation_identity_on_dense_matrices():
    """<phi|O|psi> = (E(phi + psi) - E(phi - psi) - i E(phi + i psi) + i E(phi - i psi)) / 4, E(chi) = <chi|O|chi>, for a matrix that is
    not Hermitian: the identity behind method="polarisation", with the combination ExpectationPlan._matrix_polarisation uses"""
    rs = np.random.RandomState(5)
    for n in (1, 2, 7, 40):
        O = rs.randn(n, n) + 1j * rs.randn(n, n)
        phi, psi = rs.randn(n, 3) + 1j * rs.randn(n, 3), rs.randn(n, 4) + 1j * rs.randn(n, 4)
        E = lambda chi: np.einsum("ia,ij,ja->a", chi.conj(), O, chi)  # noqa: E731
        want = phi.conj().T @ O @ psi
        for a in range(3):
            for b in range(4):
                p, q = phi[:, a:a + 1], psi[:, b:b + 1]
                got = 0.25 * (E(p + q) - E(p - q) - 1j * E(p + 1j * q) + 1j * E(p - 1j * q))[0]
                assert abs(got - want[a, b]) <= 1e-12 * max(1.0, abs(want[a, b])) * n
        assert np.abs(O - O.conj().T).max() > 0.1  # (the matrix is not Hermitian: conj(<psi|O|phi>) is another number)


def _heisenberg(basis_cfg, L, hermitian=True):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    terms = [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]
    if not hermitian:
        terms = [{"expression": "σ⁺₀ σ⁻₁", "sites": bonds}]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "H", "terms": terms}}


def test_eigenstate_matrix_elements_refuses_before_any_device_work():
    """this machine may have no device at all: every refusal below is raised before one is asked for"""
    cfg = _heisenberg(X.ring(8, 4, 0), 8)
    plain = _heisenberg(X.ring(8, 4), 8)
    zz = {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[0, 1]]}]}
    with pytest.raises(ValueError, match="no operators"):
        eigenstate_matrix_elements(cfg, [])
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_bytes"):
            eigenstate_matrix_elements(cfg, [zz], max_bytes=bad)
    for bad in ("all", [0.5, 1.5], [[0, 1]]):
        with pytest.raises(ValueError, match="states must be None, a slice or a 1-D array of integer indices"):
            eigenstate_matrix_elements(cfg, [zz], states=bad)
    # the result in bytes, by name: 16 x operators x m x m -- an index array and a bounded slice of a projected sector ...
    with pytest.raises(ValueError, match=r"eigenstate_matrix_elements: 2 operators between 5 states are 800 bytes; max_bytes is 799"):
        eigenstate_matrix_elements(cfg, [zz, zz], states=[0, 1, 2, 3, 4], max_bytes=799)
    with pytest.raises(ValueError, match=r"1 operators between 3 states are 144 bytes; max_bytes is 100"):
        eigenstate_matrix_elements(cfg, zz, states=slice(1, 7, 2), max_bytes=100)
    # ... and everything of a sector without symmetries, whose dimension follows from its quantum numbers: C(8, 4) = 70
    with pytest.raises(ValueError, match=r"1 operators between 70 states are 78400 bytes; max_bytes is 78399"):
        eigenstate_matrix_elements(plain, [zz], max_bytes=78399)
    with pytest.raises(ValueError, match=r"between 2 states are 64 bytes"):
        eigenstate_matrix_elements(plain, [zz], states=slice(-2, None), max_bytes=63)
    # what full_spectrum refuses
    with pytest.raises(ValueError, match="max_dim is 69"):
        eigenstate_matrix_elements(plain, [zz], max_dim=69)
    with pytest.raises(ValueError, match="not Hermitian"):
        eigenstate_matrix_elements(_heisenberg(X.ring(8, 4), 8, hermitian=False), [zz])


def test_matrix_elements_refuses_before_any_device_work():
    import torch

    basis = D.loadConfigFromDict(X.ring(8, 4, 0))
    zz = {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[0, 1]]}]}
    reps = torch.zeros(10, dtype=torch.int64)
    block = torch.zeros((10, 2), dtype=torch.float64)
    with pytest.raises(D.LsAmdError, match="one partition"):
        matrix_elements(basis, [reps, reps], block, block, [zz])
    with pytest.raises(D.LsAmdError, match="contiguous 1-D int64"):
        matrix_elements(basis, reps.to(torch.int32), block, block, [zz])
    with pytest.raises(D.LsAmdError, match="no operators"):
        matrix_elements(basis, reps, block, block, [])
    with pytest.raises(D.LsAmdError, match="neither an Operator"):
        matrix_elements(basis, reps, block, block, ["σᶻ₀ σᶻ₁"])


def _stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    stats = {}
    for unit in ("k_expect_mat.hip", "k_expect_mat_fermi.hip"):
        stats.update(kernel_resources.resources(source=unit))
    return stats


def test_design_lists_the_resources_of_every_instantiation():
    """the table of DESIGN.md section 6j names every instantiation of k_expect_mat with the compiler's report: scratch 0 in every
    row, static LDS within 64 KB"""
    stats = _stats()
    names = subprocess.run(["c++filt"], input="\n".join(stats), capture_output=True, text=True).stdout.split("\n")
    have = {}
    for (_, v), dn in zip(stats.items(), names):
        short = re.sub(r"^void ", "", dn.split("(")[0])
        if short.startswith("k_expect_mat<"):
            have[short] = v
    # {32, 64-bit words} x {f64 | c128 x {+-1, complex characters}} x FERMI
    assert len(have) == 12, sorted(have)
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = design.split("## 6j.")[1].split("\n## ")[0]
    rows = re.findall(r"^\| `(k_expect_mat<[^`]*>)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|$", section, re.M)
    listed = {r[0]: tuple(int(q) for q in r[1:]) for r in rows}
    assert sorted(listed) == sorted(have), sorted(set(have) ^ set(listed))
    for name, v in have.items():
        assert listed[name] == (v["sgpr"], v["vgpr"], v["occ"], v["scratch"], v["lds"]), (name, listed[name], v)
        assert v["scratch"] == 0 and v["lds"] <= 64 * 1024, (name, v)
