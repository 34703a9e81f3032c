"""The CSR export of cross-sector plans and full_spectrum, as far as no device is needed: the entry points of the C ABI and their
NULL refusals, CsrMatrix on hand-made CPU tensors, the refusals of full_spectrum that come before anything is enumerated, and the
compiler's resource report of the new kernels."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import CsrMatrix  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import diagonalize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")
NAMES = ("ls_amd_cross_csr_bytes", "ls_amd_cross_csr", "ls_amd_csr_free")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int64_t\s+ls_amd_cross_csr_bytes\s*\(\s*ls_amd_cross\s+const\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"int\s+ls_amd_cross_csr\s*\(\s*ls_amd_cross\s*\*\s*\w+\s*,\s*int64_t\s+max_bytes\s*,\s*ls_amd_csr\s*\*\s*\w+\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"void\s+ls_amd_csr_free\s*\(\s*ls_amd_csr\s*\*\s*\w+\s*\)\s*;", header)
    struct = re.search(r"typedef\s+struct\s+ls_amd_csr\s*\{(.*?)\}\s*ls_amd_csr\s*;", header, flags=re.S)
    assert struct
    for field in ("rows", "cols", "nnz", "dtype", "d_row_ptr", "d_col", "d_val"):
        assert re.search(r"\b" + field + r"\b", struct.group(1)), field
    L = _lib().load()
    for name in NAMES:
        assert hasattr(L, name), name
    # the ctypes mirror has the layout of the C struct: three int64, an enum, three pointers
    assert [f[0] for f in _lib().LsAmdCsr._fields_] == ["rows", "cols", "nnz", "dtype", "d_row_ptr", "d_col", "d_val"]
    assert C.sizeof(_lib().LsAmdCsr) == 56
    assert callable(D.CrossSectorPlan.to_csr) and callable(D.Operator.to_csr) and callable(D.Operator.to_dense)
    assert callable(diagonalize.full_spectrum) and "CsrMatrix" in D.__all__
    assert set(diagonalize.SpectrumResult.__dataclass_fields__) >= {"eigenvalues", "eigenvectors", "representatives", "dimension", "seconds"}


def test_null_arguments_are_refused_without_a_device():
    lib = _lib()
    L = lib.load()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    assert L.ls_amd_cross_csr_bytes(None) == -1 and "NULL plan" in err()
    out = lib.LsAmdCsr(rows=3, cols=4, nnz=5)
    assert L.ls_amd_cross_csr(None, 1 << 30, C.byref(out), None) == -1 and "NULL plan" in err()
    assert (out.rows, out.cols, out.nnz, out.d_row_ptr, out.d_col, out.d_val) == (0, 0, 0, None, None, None)  # cleared
    fake = C.c_void_p(8)  # never dereferenced: the output is looked at first
    assert L.ls_amd_cross_csr(fake, 1 << 30, None, None) == -1 and "NULL output" in err()
    L.ls_amd_csr_free(None)
    L.ls_amd_csr_free(C.byref(out))  # a cleared struct


def test_csr_matrix_to_dense_on_cpu_tensors():
    import torch

    # 4 x 3, rectangular, row 1 empty, the last row too
    m = CsrMatrix((4, 3), torch.tensor([0, 2, 2, 3, 3]), torch.tensor([0, 2, 1]), torch.tensor([1.5, -2.0, 4.0], dtype=torch.float64))
    want = np.array([[1.5, 0, -2.0], [0, 0, 0], [0, 4.0, 0], [0, 0, 0]])
    assert m.nnz == 3 and m.dtype == torch.float64
    assert np.array_equal(m.row_indices().numpy(), [0, 0, 2])
    assert np.array_equal(m.to_dense().numpy(), want)
    # complex, wider than tall
    z = CsrMatrix((2, 5), torch.tensor([0, 1, 3]), torch.tensor([4, 0, 3]), torch.tensor([1j, 2.0, 3 - 1j], dtype=torch.complex128))
    wz = np.zeros((2, 5), dtype=complex)
    wz[0, 4], wz[1, 0], wz[1, 3] = 1j, 2.0, 3 - 1j
    assert np.array_equal(z.to_dense().numpy(), wz)
    # no entries at all
    e = CsrMatrix((2, 2), torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64))
    assert e.nnz == 0 and np.array_equal(e.to_dense().numpy(), np.zeros((2, 2)))
    # the guard names both numbers
    with pytest.raises(D.LsAmdError, match=r"4 x 3 matrix needs 96 bytes, max_bytes is 95"):
        m.to_dense(max_bytes=95)
    t = m.to_torch()
    assert t.layout == torch.sparse_csr and tuple(t.shape) == (4, 3)
    assert torch.equal(t.crow_indices(), m.crow_indices) and torch.equal(t.col_indices(), m.col_indices) and torch.equal(t.values(), m.values)


def _chain(L, weight, expression):
    return {"basis": {"number_spins": L, "hamming_weight": weight},
            "hamiltonian": {"terms": [{"expression": expression, "sites": [[i, (i + 1) % L] for i in range(L)]}]}}


def test_full_spectrum_refusals_come_before_a_device(monkeypatch):
    def no_device():
        raise AssertionError("full_spectrum asked for a device before refusing")

    monkeypatch.setattr(_lib(), "require_device", no_device)
    with pytest.raises(ValueError, match="not Hermitian"):
        diagonalize.full_spectrum(_chain(10, 5, "σ⁺₀ σ⁻₁"))
    hermitian = _chain(10, 5, "σˣ₀ σˣ₁")
    hermitian["hamiltonian"]["terms"].append({"expression": "σʸ₀ σʸ₁", "sites": hermitian["hamiltonian"]["terms"][0]["sites"]})
    # C(10, 5) = 252 states, 252^2 doubles
    with pytest.raises(ValueError, match=rf"252 states.*{252 * 252 * 8} bytes.*max_dim is 1\b"):
        diagonalize.full_spectrum(hermitian, max_dim=1)
    with pytest.raises(ValueError, match=rf"252 states.*{252 * 252 * 16} bytes.*max_dim is 251\b"):
        diagonalize.full_spectrum(hermitian, dtype="c128", max_dim=251)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_dim"):
            diagonalize.full_spectrum(hermitian, max_dim=bad)


def test_unprojected_dimensions_from_the_quantum_numbers():
    dim = diagonalize._unprojected_dimension
    assert dim(D.loadConfigFromDict({"basis": {"number_spins": 12, "hamming_weight": 6}})) == 924
    assert dim(D.loadConfigFromDict({"basis": {"number_spins": 10}})) == 1024
    assert dim(D.loadConfigFromDict({"basis": {"particle": "spinless-fermion", "number_sites": 12, "number_particles": 5}})) == 792
    assert dim(D.loadConfigFromDict({"basis": {"particle": "spinful-fermion", "number_sites": 6, "number_particles": 6, "number_up": 3}})) == 400
    assert dim(D.loadConfigFromDict({"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 3}})) == 56
    ring = {"basis": {"number_spins": 8, "hamming_weight": 4, "symmetries": [{"permutation": [(i + 1) % 8 for i in range(8)], "sector": 0}]}}
    assert dim(D.loadConfigFromDict(ring)) is None  # known once the representatives are enumerated


# ---- the kernels in the compiler's resource report --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    return kernel_resources.resources(source="k_csr.hip")


def test_the_unit_holds_the_twenty_emitting_kinds_and_the_row_passes(stats):
    """k_csr.hip: k_cross_pull<cross_emit_w<W>, PM1, CPLX, REAL, FERMI> for the 10 kinds of either family, k_csr_merge and
    k_csr_write for f64 and c128; nothing spills, the row passes are one wave wide on less than 2 KiB of LDS"""
    emit = {}
    for name, v in stats.items():
        m = re.match(r"_Z12k_cross_pullI12cross_emit_wI([jm])ELb([01])ELb([01])ELb([01])ELb([01])EE", name)
        if m:
            emit[(m.group(1), *(int(g) for g in m.groups()[1:]))] = v
    kinds = {(w, *k, f) for w in "jm" for k in ((1, 0, 1), (1, 1, 1), (1, 1, 0), (0, 1, 1), (0, 1, 0)) for f in (0, 1)}
    assert set(emit) == kinds
    rows = {n: v for n, v in stats.items() if n.startswith(("_Z11k_csr_merge", "_Z11k_csr_write"))}
    assert len(rows) == 4 and len(stats) == 24, sorted(stats)
    for name, v in sorted(stats.items()):
        print(name[:70], v)
        assert v["scratch"] == 0, (name, v)
    for v in emit.values():
        assert v["lds"] <= 32 * 1024 and v["occ"] >= 4, v  # five blocks of 256 threads per CU at the least
    for v in rows.values():
        assert v["lds"] <= 2048 and v["occ"] == 8, v


def test_the_apply_units_keep_their_kernels():
    """the emitting mode is instantiated in k_csr.hip alone, which the Makefile builds with the template's header dependencies"""
    for unit in ("k_cross.hip", "k_cross_fermi.hip"):
        assert "cross_emit_w" not in open(os.path.join(CSRC, unit)).read()
    assert "cross_emit_w<W>" in open(os.path.join(CSRC, "k_csr.hip")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^KSRC :=.*\bk_csr\.hip\b", mk, flags=re.M)
    assert re.search(r"^k_cross\.o k_cross_fermi\.o k_csr\.o.*: k_cross_t\.hpp lsk_fermi\.hpp$", mk, flags=re.M)
