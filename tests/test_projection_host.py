"""Projection into symmetry sectors, the parts that need no device (SectorProjection, project, product_state; ls_amd_project): the
ABI and the build, the size of the full basis and its refusals, product_state -- values, weights and errors -- against the projector
columns of tests/entanglement_reference.py and tests/fermion_entanglement_reference.py (row s of B, conjugated: <r~|s>), and the
refusals of the Python layer that are raised before a device is asked for."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_symm as F
from distributed_matvec_amd import SectorProjection  # noqa: F401  (the feature under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_project_create", "ls_amd_project_full_size", "ls_amd_project_apply", "ls_amd_project_check", "ls_amd_project_kernel_name",
         "ls_amd_project_destroy", "ls_amd_test_project_full_size", "ls_amd_test_project_state_index")
NEEL = 0b010101010101


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _free_ring(L, k):
    """an L-site ring without a fixed weight, translation sector k"""
    return {"basis": {"number_spins": L, "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]}}


def _reps(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy())


def test_abi_makefile_and_python_names():
    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert "typedef struct ls_amd_project ls_amd_project;" in header
    make = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_project.hip" in ksrc and "k_project_fermi.hip" in ksrc
    assert re.search(r"^k_project\.o k_project_fermi\.o.*: k_project_t\.hpp lsk_fermi\.hpp$", make, re.M)
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_project" not in isa
    for name in ("SectorProjection", "project", "product_state"):
        assert name in D.__all__ and getattr(D, name) is getattr(D.projection, name), name


SIZES = {
    "ring12_weight6": (lambda: E.ring(12, 6, 3), math.comb(12, 6)),
    "ring12_weight6_inversion": (lambda: E.ring(12, 6, 0, inv=1), 924),
    "ring10_every_weight": (lambda: _free_ring(10, 1), 1 << 10),
    "spinful6_3_3": (lambda: {"basis": R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1).basis_config()}, 400),
    "spinless34_two_particles": (lambda: {"basis": R.Case(34, 2, gens=F.translations(34), secs=[5]).basis_config()}, math.comb(34, 2)),
    "spinless10_every_number": (lambda: {"basis": R.Case(10, None).basis_config()}, 1 << 10),
}


@pytest.mark.parametrize("name", sorted(SIZES))
def test_full_size(name):
    make, want = SIZES[name]
    basis = D.loadConfigFromDict(make())
    assert _lib().ls_amd_test_project_full_size(basis.payload) == want
    pj = D.SectorProjection(basis, _reps(np.zeros(0, dtype=np.uint64)))
    assert pj.full_size == want and pj.h is None  # on the host, before any device is needed


def test_full_size_refusals():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    big = D.loadConfigFromDict({"basis": {"number_spins": 41, "symmetries": []}})
    assert L.ls_amd_test_project_full_size(big.payload) == -1 and "41 sites without a fixed" in err()
    with pytest.raises(D.LsAmdError, match="41 sites without a fixed"):
        D.SectorProjection(big, _reps(np.zeros(0, dtype=np.uint64)))
    with pytest.raises(D.LsAmdError, match="41 sites without a fixed"):
        D.product_state(big, _reps(np.zeros(1, dtype=np.uint64)), 0)
    modes = D.loadConfigFromDict({"basis": {"particle": "spinless-fermion", "number_sites": 42}})
    assert L.ls_amd_test_project_full_size(modes.payload) == -1 and "42 modes without a fixed" in err()
    assert L.ls_amd_test_project_full_size(None) == -1 and "NULL" in err()
    # the C entry points refuse NULL arguments and bad arguments by name, before any device work
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    spin = D.loadConfigFromDict(E.ring(8, 4, 0))
    assert L.ls_amd_project_create(None, spin.payload, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_project_create(C.byref(h), None, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_project_create(C.byref(h), spin.payload, None, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_project_create(C.byref(h), big.payload, reps, 4, None) == -1 and "41 sites" in err()
    assert h.value is None
    assert L.ls_amd_project_apply(None, 0, 1, reps, 1, 0, reps, 1, 0, None) == -1 and "NULL" in err()
    assert L.ls_amd_project_check(None, None) == -1 and L.ls_amd_project_full_size(None) == -1
    assert L.ls_amd_project_kernel_name(None) is None
    L.ls_amd_project_destroy(None)


def test_state_index_is_the_position_in_the_plain_basis():
    L = _lib()
    spin = D.loadConfigFromDict(E.ring(12, 6, 3))
    full = E.tables(E.ring(12, 6, 3))[1]
    assert [L.ls_amd_test_project_state_index(spin.payload, C.c_uint64(int(s))) for s in full] == list(range(924))
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2], flip=0)
    fb = D.loadConfigFromDict({"basis": case.basis_config()})
    assert [L.ls_amd_test_project_state_index(fb.payload, C.c_uint64(int(s))) for s in case.states] == list(range(400))
    free = D.loadConfigFromDict(_free_ring(10, 1))
    assert L.ls_amd_test_project_state_index(free.payload, C.c_uint64(777)) == 777


def _check_product_state(basis, reps, states, B, s, want_weight=None):
    """product_state(s) sqrt(weight) is row s of B, conjugated; -> (psi, weight)"""
    psi, weight = D.product_state(basis, _reps(reps), int(s))
    want = np.conj(B[int(np.searchsorted(states, np.uint64(s)))])
    got = psi.numpy() * math.sqrt(weight)
    assert got.shape == want.shape and np.count_nonzero(psi.numpy()) == 1
    assert np.abs(got - want).max() <= 1e-14, np.abs(got - want).max()
    assert abs(np.linalg.norm(psi.numpy()) - 1.0) <= 1e-15 and abs(weight - np.linalg.norm(want) ** 2) <= 1e-14
    if want_weight is not None:
        assert abs(weight - want_weight) <= 1e-14
    return psi, weight


def test_neel_state_lives_in_two_sectors_of_the_ring():
    import torch

    total = 0.0
    for k in range(12):
        for inv in (1, -1):
            cfg = E.ring(12, 6, k, inv=inv)
            basis = D.loadConfigFromDict(cfg)
            _model, full, reps, _idx, _coef, _live = E.tables(cfg)
            if (k, inv) in ((0, 1), (6, -1)):
                _, B = E.projector_columns(cfg)
                psi, w = _check_product_state(basis, reps, full, B, NEEL, 0.5)
                assert psi.dtype == torch.float64  # a real entry, +-1 characters
                psi_c, _ = D.product_state(basis, _reps(reps), NEEL, dtype=torch.complex128)
                assert psi_c.dtype == torch.complex128 and np.array_equal(psi_c.numpy(), psi.numpy().astype(complex))
                total += w
            else:
                with pytest.raises(D.LsAmdError, match="zero weight") as e:
                    D.product_state(basis, _reps(reps), NEEL)
                assert "0b010101010101" in str(e.value) and f"[{k}]" in str(e.value) and f"spin inversion {inv:+d}" in str(e.value)
    assert abs(total - 1.0) <= 1e-14


def test_product_states_of_a_complex_sector_and_a_stabilised_orbit():
    import torch

    cfg = E.ring(12, 6, 3)
    basis = D.loadConfigFromDict(cfg)
    _model, full, reps, _idx, _coef, live = E.tables(cfg)
    _, B = E.projector_columns(cfg)
    seen_complex = False
    for s in full[live][::37]:
        psi, _ = _check_product_state(basis, reps, full, B, s)
        assert psi.dtype == torch.complex128  # complex characters
        seen_complex = seen_complex or abs(psi.numpy().imag).max() > 0.5
    assert seen_complex
    with pytest.raises(D.LsAmdError, match="float64 cannot hold"):
        D.product_state(basis, _reps(reps), int(full[live][1]), dtype=torch.float64)
    dead = full[~live]
    assert len(dead)  # k = 3 kills the orbits of period 2 and 6
    with pytest.raises(D.LsAmdError, match="zero weight"):
        D.product_state(basis, _reps(reps), int(dead[0]))


FERMI = {
    "spinless8_k0": lambda: R.Case(8, 4, gens=F.translations(8), secs=[0]),
    "spinful6_k0_flip_plus": lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1),
    "spinful6_k1_flip_minus": lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[1], flip=-1),
    "spinless10_dihedral": lambda: R.Case(10, 5, gens=F.dihedral(10), secs=[0, 1]),
}


@pytest.mark.parametrize("name", sorted(FERMI))
def test_fermionic_product_states_carry_the_orbit_sign(name):
    case = FERMI[name]()
    basis = D.loadConfigFromDict({"basis": case.basis_config()})
    B = case.columns.toarray()
    live = np.flatnonzero(case.live)
    assert len(live) > 40
    negative = 0
    for i in live[::max(1, len(live) // 40)]:
        _check_product_state(basis, case.reps, case.states, B, case.states[i])
    if name.endswith("k0") or name.endswith("flip_plus"):
        # every character is +1: a negative entry is the orbit sign alone, and without it the value would be wrong
        rows = [i for i in live if B[i].real.min() < -1e-9]
        assert rows
        for i in rows[:5]:
            psi, _ = _check_product_state(basis, case.reps, case.states, B, case.states[i])
            negative += int(psi.numpy().real.min() == -1.0)
        assert negative == len(rows[:5])
    dead = np.flatnonzero(~case.live)
    if len(dead):
        with pytest.raises(D.LsAmdError, match="zero weight"):
            D.product_state(basis, _reps(case.reps), int(case.states[dead[0]]))


def test_states_outside_the_basis_are_refused_by_name():
    ring = D.loadConfigFromDict(E.ring(12, 6, 0, inv=1))
    reps = _reps(E.tables(E.ring(12, 6, 0, inv=1))[2])
    with pytest.raises(D.LsAmdError, match="bits above the 12 sites"):
        D.product_state(ring, reps, 1 << 12 | NEEL)
    with pytest.raises(D.LsAmdError, match="Hamming weight 5, the basis 6"):
        D.product_state(ring, reps, 0b11111)
    with pytest.raises(D.LsAmdError, match="int word"):
        D.product_state(ring, reps, 1.0)
    with pytest.raises(D.LsAmdError, match="64-bit"):
        D.product_state(ring, reps, -1)
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.product_state(ring, [reps, reps], NEEL)
    with pytest.raises(D.LsAmdError, match="not among reps"):
        D.product_state(ring, reps[1:], int(reps[0]))
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1)
    fb = D.loadConfigFromDict({"basis": case.basis_config()})
    with pytest.raises(D.LsAmdError, match=r"\(2 up, 4 down\), the basis \(3 up, 3 down\)"):
        D.product_state(fb, _reps(case.reps), 0b001111_000011)
    with pytest.raises(D.LsAmdError, match="bits above the 12 modes"):
        D.product_state(fb, _reps(case.reps), 1 << 12)
    spinless = R.Case(8, 4, gens=F.translations(8), secs=[1])
    sb = D.loadConfigFromDict({"basis": spinless.basis_config()})
    with pytest.raises(D.LsAmdError, match="particle number 3, the basis 4"):
        D.product_state(sb, _reps(spinless.reps), 0b111)


def test_python_refusals_that_need_no_device():
    import torch

    cfg = E.ring(12, 6, 3)
    basis = D.loadConfigFromDict(cfg)
    reps = _reps(E.tables(cfg)[2])
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.SectorProjection(basis, [reps, reps])
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.project(basis, [reps, reps], torch.zeros(924, dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match="int64"):
        D.SectorProjection(basis, reps.double())
    pj = D.SectorProjection(basis, [reps])
    assert pj.full_size == 924 and pj.complex_characters
    with pytest.raises(D.LsAmdError, match="923 rows, the basis without symmetries has 924 states"):
        pj.project(torch.zeros(923, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="923 rows"):
        pj.project(torch.zeros(923, 2, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="vector of 924 elements or an"):
        pj.project(torch.zeros(924, 2, 2, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=r"K = 65 columns, outside \[1, 64\]"):
        pj.project(torch.zeros(924, 65, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match=r"K = 0 columns"):
        pj.project(torch.zeros(924, 0, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="neither float64 nor complex128"):
        pj.project(torch.zeros(924, dtype=torch.float32))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        pj.project(torch.zeros(924, dtype=torch.complex128))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        pj.project(np.zeros(924))
    assert pj.h is None  # nothing above asked for a device
    pj.destroy()
