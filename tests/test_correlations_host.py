"""Correlation matrices without a device: the C ABI, the Makefile entry and the Python names are there; the group average of the
raw matrices (ls_amd_test_corr_symmetrize) equals a numpy average over the images ls_amd_basis_apply_group_element gives of the
one-hot states -- a ring with translations, reflection and spin inversion, a torus, a spinful basis with the up <-> down flip --
on random raw matrices; and the refusals that need no device come back by name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_symm as F
from distributed_matvec_amd import CorrelationPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from helpers import approx_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_corr_create", "ls_amd_corr_modes", "ls_amd_corr_densities", "ls_amd_corr_hoppings", "ls_amd_corr_kernel_name",
         "ls_amd_corr_destroy", "ls_amd_test_corr_symmetrize")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _f64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_abi_makefile_and_python_names():
    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert "typedef struct ls_amd_corr ls_amd_corr;" in header
    make = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_corr.hip" in ksrc and "k_corr_fermi.hip" in ksrc
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_corr" not in isa
    for name in ("CorrelationPlan", "spin_correlations", "fermion_correlations", "structure_factor", "SpinCorrelations", "FermionCorrelations"):
        assert name in D.__all__ and hasattr(D, name), name
    assert callable(D.correlations.correlations)


def _torus_spin_config():
    tx, ty = F.torus(4, 3, point_group=False)
    return {"basis": {"number_spins": 12, "hamming_weight": 6, "symmetries": [{"permutation": tx, "sector": 0}, {"permutation": ty, "sector": 0}]}}


BASES = {
    "ring12_translation_reflection_inversion": lambda: E.ring(12, 6, 0, inv=1, reflect=0),
    "ring12_k6_reflection_inversion_minus": lambda: E.ring(12, 6, 6, inv=-1, reflect=1),
    "torus_4x3": _torus_spin_config,
    "spinful6_spin_flip": lambda: {"basis": R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1).basis_config()},
    "ring10_unprojected": lambda: E.ring(10, 5, None),
}


def _images(basis):
    """img[g][i] = the position of the bit of g(1 << i), for every permutation element of the group"""
    L = _lib()
    M, order = basis.numberBits(), int(L.ls_amd_basis_group_order(basis.payload))
    img = np.zeros((order, M), dtype=np.int64)
    for g in range(order):
        for i in range(M):
            t = int(L.ls_amd_basis_apply_group_element(basis.payload, g, C.c_uint64(1 << i)))
            assert bin(t).count("1") == 1
            img[g, i] = t.bit_length() - 1
        assert sorted(img[g]) == list(range(M))
    return img


@pytest.mark.parametrize("name", sorted(BASES))
def test_symmetrize_is_the_average_over_the_group(name):
    L = _lib()
    basis = D.loadConfigFromDict(BASES[name]())
    M = basis.numberBits()
    img = _images(basis)
    inv = basis.spinInversion() != 0
    expect = {"ring12_translation_reflection_inversion": (24, True), "ring12_k6_reflection_inversion_minus": (24, True), "torus_4x3": (12, False),
              "spinful6_spin_flip": (12, False), "ring10_unprojected": (1, False)}[name]
    assert (len(img), inv) == expect and M == (12 if name != "ring10_unprojected" else 10)
    rs = np.random.RandomState(len(name))
    # densities: the one-point row, then D
    d, Dm = rs.rand(M), rs.rand(M, M)
    raw = np.concatenate([d, Dm.ravel()])
    out = np.zeros_like(raw)
    assert L.ls_amd_test_corr_symmetrize(basis.payload, 0, _f64p(raw), _f64p(out)) == 0
    want_d, want_D = np.zeros(M), np.zeros((M, M))
    for p in img:
        want_d += d[p]
        want_D += Dm[np.ix_(p, p)]
        if inv:  # the same element with the global flip: bit b -> 1 - b
            want_d += 1.0 - d[p]
            want_D += 1.0 - d[p][:, None] - d[p][None, :] + Dm[np.ix_(p, p)]
    order = len(img) * (2 if inv else 1)
    assert approx_equal(out[:M], want_d / order).all() and approx_equal(out[M:].reshape(M, M), want_D / order).all()
    # hoppings
    G = rs.rand(M, M) + 1j * rs.rand(M, M)
    out = np.zeros((M, M), dtype=np.complex128)
    assert L.ls_amd_test_corr_symmetrize(basis.payload, 1, _f64p(G.view(np.float64)), _f64p(out.view(np.float64))) == 0
    want = np.zeros((M, M), dtype=np.complex128)
    for p in img:
        want += G[np.ix_(p, p)]
        if inv:  # B+_i B_j -> B_i B+_j = B+_j B_i off the diagonal, the density -> 1 - density on it
            flipped = G[np.ix_(p, p)].T.copy()
            np.fill_diagonal(flipped, 1.0 - np.diag(G)[p])
            want += flipped
    want /= order
    assert approx_equal(out.real, want.real).all() and approx_equal(out.imag, want.imag).all()
    # the average is a projection: applying it twice changes nothing beyond rounding
    again = np.zeros_like(out)
    assert L.ls_amd_test_corr_symmetrize(basis.payload, 1, _f64p(out.view(np.float64)), _f64p(again.view(np.float64))) == 0
    assert np.abs(again - out).max() < 1e-14


def test_refusals_that_need_no_device():
    L = _lib()
    from distributed_matvec_amd._lib import LsAmdError, LsHsBasis

    def message():
        return L.ls_amd_last_error().decode()

    basis = D.loadConfigFromDict(E.ring(8, 4, 0))
    h = C.c_void_p()
    one = (C.c_uint64 * 1)(15)
    assert L.ls_amd_corr_create(C.byref(h), None, one, 1, None) == -1 and "ls_amd_corr_create: NULL basis" in message()
    assert L.ls_amd_corr_create(None, basis.payload, one, 1, None) == -1 and "NULL handle" in message()
    foreign = LsHsBasis()
    assert L.ls_amd_corr_create(C.byref(h), C.byref(foreign), one, 1, None) == -1 and "not built by this library" in message()
    assert L.ls_amd_corr_create(C.byref(h), basis.payload, one, 0, None) == -1 and "no rows" in message()
    assert L.ls_amd_corr_create(C.byref(h), basis.payload, None, 5, None) == -1 and "NULL representatives" in message()
    assert not h.value
    wide = D.loadConfigFromDict({"basis": R.Case(62, 2, gens=F.translations(62), secs=[0]).basis_config()})
    assert L.ls_amd_corr_create(C.byref(h), wide.payload, one, 1, None) == -1
    assert "ls_amd_corr_create: projected fermionic bases of more than 60 modes" in message()
    raw = np.zeros(8 + 64)
    assert L.ls_amd_test_corr_symmetrize(None, 0, _f64p(raw), _f64p(raw)) == -1 and "NULL basis" in message()
    assert L.ls_amd_test_corr_symmetrize(basis.payload, 2, _f64p(raw), _f64p(raw)) == -1 and "kind 2" in message()
    assert L.ls_amd_test_corr_symmetrize(basis.payload, 0, None, _f64p(raw)) == -1 and "NULL raw matrix" in message()
    assert L.ls_amd_corr_modes(None) == -1 and "NULL plan" in message()
    assert L.ls_amd_corr_kernel_name(None, 0) is None and "NULL plan" in message()
    assert L.ls_amd_corr_densities(None, 0, None, None, None, 1, None) == -1 and "ls_amd_corr_densities: NULL plan" in message()
    assert L.ls_amd_corr_hoppings(None, 0, None, None, 1, None) == -1 and "ls_amd_corr_hoppings: NULL plan" in message()
    L.ls_amd_corr_destroy(None)
    # the Python entry points name the other family
    fermi = D.loadConfigFromDict({"basis": R.Case(6, 3).basis_config()})
    with pytest.raises(LsAmdError, match="fermion_correlations"):
        D.spin_correlations(fermi, None, None)
    with pytest.raises(LsAmdError, match="spin_correlations"):
        D.fermion_correlations(basis, None, None)
    with pytest.raises(LsAmdError, match="one partition"):
        D.CorrelationPlan(basis, [None, None])
    with pytest.raises(LsAmdError, match="contiguous 1-D int64"):
        D.CorrelationPlan(basis, np.arange(3))


def test_structure_factor_is_the_fourier_sum():
    rs = np.random.RandomState(3)
    N = 6
    Cm = rs.rand(N, N) + 1j * rs.rand(N, N)
    Cm = Cm + Cm.conj().T
    pos = np.arange(N, dtype=float)
    q = 2 * np.pi * np.arange(N) / N
    got = D.structure_factor(Cm, pos, q)
    want = np.array([sum(np.exp(1j * qq * (pos[i] - pos[j])) * Cm[i, j] for i in range(N) for j in range(N)) / N for qq in q])
    assert np.abs(got - want).max() < 1e-13 and np.abs(got.imag).max() < 1e-13
    # two dimensions
    pos2 = np.array([[x, y] for y in range(2) for x in range(3)], dtype=float)
    q2 = np.array([[0.0, 0.0], [2 * np.pi / 3, np.pi]])
    got = D.structure_factor(Cm, pos2, q2)
    want = np.array([sum(np.exp(1j * qq @ (pos2[i] - pos2[j])) * Cm[i, j] for i in range(N) for j in range(N)) / N for qq in q2])
    assert np.abs(got - want).max() < 1e-13
    with pytest.raises(ValueError):
        D.structure_factor(Cm, pos[:4], q)
