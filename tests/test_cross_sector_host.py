"""Cross-sector operators without a device: the C ABI (ls_amd_operator_adjoint, ls_amd_operator_maps_sector, ls_amd_cross_*) is
declared and exported and refuses NULL arguments; the adjoint of the term tables is the conjugate transpose on every state; the
covariance check accepts the operators the numpy projectors say map one sector into another -- however they are written -- and
refuses the neighbouring wrong sectors by naming the generator; the push formula used as the reference at L = 16 agrees with
explicit projectors; and the kernels of csrc/k_cross.hip are in the compiler's resource report within the budget."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import CrossSectorPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from fermion_jw import yaml_terms
from helpers import apply_terms_python, product_terms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_operator_adjoint", "ls_amd_operator_maps_sector", "ls_amd_cross_create", "ls_amd_cross_apply", "ls_amd_cross_check",
         "ls_amd_cross_kernel_name", "ls_amd_cross_nnz", "ls_amd_cross_destroy")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _operator(basis_cfg, op_cfg):
    """(Basis, Operator) of an operator section on a basis config"""
    basis = D.loadConfigFromDict(basis_cfg)
    return basis, D.Operator.fromSpec(basis, config.parse_operator(op_cfg, basis.spec))


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"ls_hs_operator\s*\*\s*ls_amd_operator_adjoint\s*\(\s*ls_hs_operator\s+const\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"int\s+ls_amd_operator_maps_sector\s*\(\s*ls_hs_operator\s+const\s*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"int\s+ls_amd_cross_create\s*\(\s*ls_amd_cross\s*\*\*\s*\w+\s*,\s*ls_hs_operator\s+const\s*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*"
                     r"\s*\w+\s*,\s*ls_amd_dtype\s+\w+\s*,\s*uint64_t\s+const\s*\*\s*d_src_reps\s*,\s*int64_t\s+n_src\s*,\s*uint64_t\s+const\s*\*"
                     r"\s*d_dst_reps\s*,\s*int64_t\s+n_dst\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    for name in NAMES[3:]:
        assert re.search(r"\b" + name + r"\s*\(", header), name
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    from distributed_matvec_amd import kpm

    assert callable(D.CrossSectorPlan) and callable(D.Operator.adjoint) and callable(D.Operator.mapsSector)
    assert "target" in kpm.spectral_function.__code__.co_varnames and "target_state" in kpm.KpmResult.__dataclass_fields__


def test_null_arguments_are_refused_without_a_device():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    assert not L.ls_amd_operator_adjoint(None) and "NULL" in err()
    basis, op = _operator(X.ring(8, 4, 0), X.sz_q(8, 3))
    assert L.ls_amd_operator_maps_sector(None, basis.payload) == -1 and "NULL" in err()
    assert L.ls_amd_operator_maps_sector(op.payload, None) == -1 and "NULL" in err()
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    assert L.ls_amd_cross_create(None, op.payload, basis.payload, 1, reps, 4, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_create(C.byref(h), None, basis.payload, 1, reps, 4, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_create(C.byref(h), op.payload, None, 1, reps, 4, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_create(C.byref(h), op.payload, basis.payload, 1, None, 4, reps, 4, None) == -1 and "NULL" in err()
    assert h.value is None
    assert L.ls_amd_cross_apply(None, reps, reps, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_check(None, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_kernel_name(None) is None and "NULL" in err()
    assert L.ls_amd_cross_nnz(None) == -1 and "NULL" in err()
    L.ls_amd_cross_destroy(None)


# ---- the adjoint -----------------------------------------------------------------------------------------------------------------
def _dense(op, nbits):
    """<b|A|a> of an Operator over all 2^nbits states, from its term tables"""
    diag, off = product_terms(op)
    out = np.zeros((1 << nbits, 1 << nbits), dtype=complex)
    for a in range(1 << nbits):
        for b, v in apply_terms_python(diag + off, a).items():
            out[b, a] += v
    return out


def _random_spin_operator(basis, rng, n_terms=14, L=6):
    terms = []
    for _ in range(n_terms):
        m = int(rng.integers(0, 1 << L))
        r = int(rng.integers(0, 1 << L)) & m
        x = int(rng.integers(0, 1 << L))
        s = int(rng.integers(0, 1 << L))
        terms.append((complex(rng.normal(), rng.normal()), m, r, x, s))
    terms.append((complex(rng.normal(), rng.normal()), 0b000101, 0b000100, 0, 0b110000))  # diagonal, with projector and sign
    terms.append((complex(rng.normal(), rng.normal()), 0b011000, 0b001000, 0b011001, 0b001010))  # flip and sign overlap (x & s != 0)
    return D.Operator.fromSpec(basis, config.OperatorSpec(terms))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_adjoint_is_the_conjugate_transpose_on_every_state(seed):
    basis = D.loadConfigFromDict({"basis": {"number_spins": 6, "symmetries": []}})
    A = _random_spin_operator(basis, np.random.default_rng(seed))
    dA = _dense(A, 6)
    assert np.count_nonzero(dA) > 100 and np.abs(dA - dA.conj().T).max() > 0.1  # generic: dense and far from Hermitian
    used = [t for part in product_terms(A) for t in part]
    assert any(t[1] for t in used) and any(t[3] for t in used) and any(t[4] for t in used) and any(t[3] & t[4] for t in used)
    Ad = A.adjoint()
    assert np.abs(_dense(Ad, 6) - dA.conj().T).max() <= 1e-14 * np.abs(dA).max()
    assert np.abs(_dense(Ad.adjoint(), 6) - dA).max() <= 1e-14 * np.abs(dA).max()
    assert not A.isHermitian and Ad.isReal == A.isReal


def test_adjoint_of_a_fermionic_hop():
    cfg = {"basis": {"particle": "spinless-fermion", "number_sites": 6}}
    model = [((0.7 + 0.4j), [("+", 0, 0), ("-", 3, 0)]), (-1.3, [("+", 5, 0), ("-", 2, 0)]), (0.25, [("+", 1, 0), ("-", 2, 0), ("n", 4, 0)])]
    basis, A = _operator(cfg, {"terms": yaml_terms(model, False)})
    dA = _dense(A, 6)
    assert np.count_nonzero(dA) > 0 and (dA.real < 0).any() and (dA.real > 0).any()  # the Jordan-Wigner signs are in the tables
    Ad = A.adjoint()
    assert np.abs(_dense(Ad, 6) - dA.conj().T).max() <= 1e-15
    assert np.abs(_dense(Ad.adjoint(), 6) - dA).max() <= 1e-15


# ---- the covariance check -----------------------------------------------------------------------------------------------------
def _maps(src_cfg, dst_cfg, op_cfg):
    """(bool, message)"""
    _, op = _operator(src_cfg, op_cfg)
    target = D.loadConfigFromDict(dst_cfg)
    ok = op.mapsSector(target)
    msg = ""
    if not ok:
        with pytest.raises(D.LsAmdError) as e:
            op.mapsSector(target, explain=True)
        msg = str(e.value)
    return ok, msg


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_maps_sector_accepts_the_covariant_cases(name):
    src, dst, op, _ = X.CASES[name]
    ok, msg = _maps(src, dst, op)
    assert ok, msg
    # ... and numpy agrees that nothing leaves the target sector
    assert X.projector_matrix(src, dst, op)[3] <= 1e-12


def test_maps_sector_does_not_depend_on_how_the_operator_is_written():
    src, dst = X.ring(8, 4, 0), X.ring(8, 4, 3)
    _, a = _operator(src, X.sz_q(8, 3))
    _, b = _operator(src, X.sz_q_projectors(8, 3))
    ta, tb = product_terms(a)[0], product_terms(b)[0]
    assert all(t[1] == 0 and t[4] != 0 for t in ta) and all(t[1] != 0 and t[4] == 0 for t in tb)  # sign masks | projector terms
    assert np.abs(_dense(a, 8) - _dense(b, 8)).max() <= 1e-15  # the same operator
    assert _maps(src, dst, X.sz_q(8, 3))[0] and _maps(src, dst, X.sz_q_projectors(8, 3))[0]
    assert not _maps(src, dst, X.sz_q_projectors(8, 2))[0]


def test_maps_sector_refuses_the_neighbouring_sectors_and_names_the_generator():
    # dk = 2 used for k 0 -> 3: by the projectors 2.8 of the image leaves the target sector -- no rounding effect
    src, dst = X.ring(8, 4, 0), X.ring(8, 4, 3)
    leak = X.projector_matrix(src, dst, X.sz_q(8, 2))[3]
    assert leak > 1.0
    ok, msg = _maps(src, dst, X.sz_q(8, 2))
    assert not ok and "generator 0" in msg, msg
    ok, msg = _maps(X.ring(8, 4, 0), X.ring(8, 3, 3), X.splus_q(8, 2))
    assert not ok and "generator 0" in msg, msg
    # the staggered field: reflection sector 0 instead of 1, inversion +1 instead of -1
    s = X.ring(8, 4, 0, 0, 1)
    ok, msg = _maps(s, X.ring(8, 4, 4, 0, -1), X.staggered_z(8))
    assert not ok and "generator 1" in msg and "generator 0" not in msg, msg
    ok, msg = _maps(s, X.ring(8, 4, 4, 1, 1), X.staggered_z(8))
    assert not ok and "spin inversion" in msg and "generator" not in msg, msg
    ok, msg = _maps(s, X.ring(8, 4, 0, 1, -1), X.staggered_z(8))  # ... and translation sector 0 instead of 4
    assert not ok and "generator 0" in msg, msg


def test_maps_sector_preconditions_have_their_own_messages():
    src = X.ring(8, 4, 0)
    op = X.sz_q(8, 0)
    other = {"basis": {"number_spins": 8, "hamming_weight": 4, "symmetries": [{"permutation": [(i + 2) % 8 for i in range(8)], "sector": 0}]}}
    ok, msg = _maps(src, other, op)
    assert not ok and "different generators" in msg
    ok, msg = _maps(src, X.ring(8, 4, 0, 0), op)  # one generator more
    assert not ok and "different generators" in msg
    ok, msg = _maps(src, X.ring(10, 5, 0), op)
    assert not ok and "different number_sites" in msg
    ok, msg = _maps(src, X.ring(8, 4, 0, inversion=1), op)
    assert not ok and "one basis only" in msg
    ok, msg = _maps(src, {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 4}}, op)
    assert not ok and "particle types" in msg
    fermi = {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 4,
                       "symmetries": [{"permutation": [(i + 1) % 8 for i in range(8)], "sector": 0}]}}
    hop = {"terms": yaml_terms([(1.0, [("+", j, 0), ("-", (j + 1) % 8, 0)]) for j in range(8)], False)}
    ok, msg = _maps(fermi, fermi, hop)
    assert not ok and "projected fermionic" in msg
    # no group at all: nothing to check (Hamming weights are a run-time matter)
    plain = {"basis": {"number_spins": 8, "hamming_weight": 4, "symmetries": []}}
    assert _maps(plain, plain, {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}]})[0]
    free = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2}}
    to = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 5, "number_up": 3}}
    assert _maps(free, to, {"terms": yaml_terms([(1.0, [("+", 2, 0)])], True)})[0]


# ---- the reference of the GPU tests ----------------------------------------------------------------------------------------------
EXPECTED = {"L8_sz_k0_k3": (10, 8, 2), "L8_dihedral_staggered": (7, 4, 3)}  # source rows, target rows, images dropped for zero norm


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_formula_matrix_is_the_projector_matrix(name):
    src, dst, op, _ = X.CASES[name]
    r1, r2, want, leak = X.projector_matrix(src, dst, op)
    got = X.case_formula(name)
    assert np.array_equal(got["src"], r1) and np.array_equal(got["dst"], r2)
    assert leak <= 1e-12 and np.abs(want).max() > 0.1 and got["images"] > 0
    assert np.abs(got["matrix"] - want).max() <= 1e-12
    if name in EXPECTED:
        assert (len(r1), len(r2), got["dropped"]) == EXPECTED[name]


def test_formula_matrix_is_the_projector_matrix_at_12_sites():
    src, dst, op = X.ring(12, 6, 0), X.ring(12, 6, 5), X.sz_q(12, 5)
    r1, r2, want, leak = X.projector_matrix(src, dst, op)
    got = X.formula_matrix(src, dst, op)
    assert np.array_equal(got["src"], r1) and np.array_equal(got["dst"], r2) and leak <= 1e-12
    assert np.abs(got["matrix"] - want).max() <= 1e-12 and np.abs(want).max() > 0.1


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
def test_cross_kernels_in_the_resource_report():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    stats = kernel_resources.resources(source="k_cross.hip")
    cross = {k: v for k, v in stats.items() if k.startswith("_Z12k_cross_pullI")}
    # {32-, 64-bit words} x {f64 | c128 x {+-1, complex source characters} x {real, complex terms}}
    assert len(cross) == 10, sorted(cross)
    assert len(stats) == 10, sorted(stats)  # nothing else in the unit
    for name, v in stats.items():
        assert v["scratch"] == 0, (name, v)
        # the admitted-blocks rule of test_hot_kernel_register_budget: the SGPR file must not admit fewer blocks than LDS and VGPRs
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (name, v)
