"""Expectation values of arbitrary operators without a device: the C ABI, the Makefile entries and the Python names are there; the
group average the host compiles (ls_amd_test_expect_average: the merged terms of |G|^-1 sum_g U_g O U_g^-1) equals, entry by entry
over all 2^M product states, a numpy average with U_g built from the images ls_amd_basis_apply_group_element gives, the permutation
sign of tests/fermion_symm.py (counted pair by pair) and the global spin inversion -- for random 3- and 4-site monomials with sigma^y
and overlapping sites on the spin bases, with n factors and four-point c+ c+ c c on the fermionic ones; and the refusals that need no
device come back by name.

An operator is kept as {flip mask x: c_x[a]} with O|a> = sum_x c_x[a] |a ^ x>, a vector over all words per flip mask: the matrix
itself (4096^2 entries) is never formed, and nothing is left out of the comparison.  Then
    (U_g O U_g^+) = {g.x: c'[g.a] = sign(g, a) sign(g, a ^ x) c_x[a]},   (F O F) = {x: c'[~a] = c_x[a]}."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_spinful_symm as FS
import fermion_symm as F
from distributed_matvec_amd import ExpectationPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from distributed_matvec_amd.api import Operator
from test_correlations_host import BASES as CORR_BASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_expect_create", "ls_amd_expect_values", "ls_amd_expect_num_terms", "ls_amd_expect_num_groups",
         "ls_amd_expect_kernel_name", "ls_amd_expect_destroy", "ls_amd_test_expect_average")
ONE = np.uint64(1)

BASES = dict(CORR_BASES)
BASES["spinless12_dihedral_reflection_odd"] = lambda: {"basis": R.Case(12, 6, gens=F.dihedral(12), secs=[0, 1]).basis_config()}
BASES["spinless10_k3"] = lambda: {"basis": R.Case(10, 4, gens=F.translations(10), secs=[3]).basis_config()}


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _message():
    return _lib().ls_amd_last_error().decode()


def test_abi_makefile_and_python_names():
    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert "typedef struct ls_amd_expect ls_amd_expect;" in header
    make = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile"), encoding="utf-8").read()
    ksrc = re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    assert "k_expect.hip" in ksrc and "k_expect_fermi.hip" in ksrc
    assert re.search(r"^k_expect\.o k_expect_fermi\.o.*: .*k_expect_t\.hpp.*k_corr_t\.hpp", make, re.M)
    # the new units are not fingerprinted: the fingerprints of the existing kernels stay what they were
    isa = open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert "k_expect" not in isa
    for name in ("ExpectationPlan", "expectation_values", "dimer_correlations", "pair_correlations"):
        assert name in D.__all__ and hasattr(D, name), name
    assert callable(D.expectation.expectation)


# ---- the group average ------------------------------------------------------------------------------------------------------------
def _permutations(basis):
    """p[g] with (g.a)[i] = a[p[g][i]], from the images of the one-hot words"""
    L = _lib()
    M, order = basis.numberBits(), int(L.ls_amd_basis_group_order(basis.payload))
    out = []
    for g in range(order):
        p = [None] * M
        for s in range(M):
            t = int(L.ls_amd_basis_apply_group_element(basis.payload, g, C.c_uint64(1 << s)))
            assert bin(t).count("1") == 1
            p[t.bit_length() - 1] = s
        assert sorted(p) == list(range(M))
        out.append(p)
    return out


def _as_maps(terms, M):
    """{x: c_x[a]} of terms (v, m, r, x, s): A|a> = v [a & m == r] (-1)^popcount(a & s) |a ^ x>"""
    words = np.arange(1 << M, dtype=np.uint64)
    out = {}
    for v, m, r, x, s in terms:
        c = np.where((words & np.uint64(m)) == np.uint64(r), complex(v), 0.0) * np.where(np.bitwise_count(words & np.uint64(s)) & 1, -1.0, 1.0)
        out[int(x)] = out.get(int(x), 0.0) + c
    return out


def _reference_average(maps, perms, M, fermi, inv):
    words = np.arange(1 << M, dtype=np.uint64)
    full = np.uint64((1 << M) - 1)
    acc = {}
    for p in perms:
        ga = FS.apply_v(p, words)
        sg = FS.sign_v(p, words) if fermi else np.ones(len(words))
        for x, c in maps.items():
            gx = int(FS.apply_v(p, np.array([x], dtype=np.uint64))[0])
            moved = np.zeros(len(words), dtype=np.complex128)
            moved[ga] = c * sg * sg[words ^ np.uint64(x)]
            acc[gx] = acc.get(gx, 0.0) + moved
            if inv:
                flipped = np.zeros_like(moved)
                flipped[words ^ full] = moved
                acc[gx] = acc[gx] + flipped
    order = len(perms) * (2 if inv else 1)
    return {x: c / order for x, c in acc.items()}


def _average_hook(basis, op):
    L = _lib()
    n = int(L.ls_amd_test_expect_average(basis.payload, op.payload, 0, None, None, None, None, None))
    assert n >= 0, _message()
    v = np.zeros(2 * max(n, 1))
    m, r, x, s = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(4))
    u64p = C.POINTER(C.c_uint64)
    got = int(L.ls_amd_test_expect_average(basis.payload, op.payload, n, v.ctypes.data_as(C.POINTER(C.c_double)), m.ctypes.data_as(u64p),
                                           r.ctypes.data_as(u64p), x.ctypes.data_as(u64p), s.ctypes.data_as(u64p)))
    assert got == n
    terms = [(complex(v[2 * i], v[2 * i + 1]), int(m[i]), int(r[i]), int(x[i]), int(s[i])) for i in range(n)]
    for _, mm, rr, _, ss in terms:  # the canonical form
        assert rr & ~mm == 0 and ss & mm == 0
    return terms


_SUBS = "₀₁₂₃"


def _random_sections(rs, spec, count):
    """random 3- and 4-site monomials with a random complex coefficient in the language of the basis"""
    L = spec.number_sites
    out = []
    for _ in range(count):
        k = int(rs.choice([3, 4]))
        sites = [int(q) for q in rs.choice(L, size=k, replace=False)]
        coef = complex(rs.randn(), rs.randn())
        if spec.particle == "spin-1/2":
            kinds = ["σʸ"] + [str(rs.choice(["σˣ", "σʸ", "σᶻ", "σ⁺", "σ⁻"])) for _ in range(k + 1)]  # k + 2 factors: sites overlap
            local = list(range(k)) + [int(q) for q in rs.choice(k, size=2)]
            rs.shuffle(local)
            expr = " ".join(f"{a}{_SUBS[i]}" for a, i in zip(kinds, local))
        elif spec.particle == "spinless-fermion":
            shape = [["c†", "c†", "c", "c"], ["n", "c†", "c", "n"], ["c†", "n", "c"], ["c†", "c", "n"], ["n", "n", "n"]][int(rs.randint(5))]
            k = len(shape)
            sites = [int(q) for q in rs.choice(L, size=k, replace=False)]
            expr = " ".join(f"{a}{_SUBS[i]}" for i, a in enumerate(shape))
        else:
            shape = [["c†", "c†", "c", "c"], ["n", "c†", "c", "n"], ["c†", "n", "c"], ["n", "n", "c†", "c"]][int(rs.randint(4))]
            k = len(shape)
            sites = [int(q) for q in rs.choice(L, size=k, replace=False)]
            expr = " ".join(f"{a}{_SUBS[i]}{rs.choice(['↑', '↓'])}" for i, a in enumerate(shape))
        out.append({"terms": [{"expression": f"({coef.real:.17g}{coef.imag:+.17g}j) × {expr}", "sites": [sites]}]})
    return out


@pytest.mark.parametrize("name", sorted(BASES))
def test_average_is_the_average_over_the_group(name):
    basis = D.loadConfigFromDict(BASES[name]())
    spec = basis.spec
    M = basis.numberBits()
    assert M <= 12
    perms = _permutations(basis)
    inv = basis.spinInversion() != 0
    fermi = spec.particle != "spin-1/2"
    assert (len(perms), inv) == {"ring12_translation_reflection_inversion": (24, True), "ring12_k6_reflection_inversion_minus": (24, True),
                                 "torus_4x3": (12, False), "spinful6_spin_flip": (12, False), "ring10_unprojected": (1, False),
                                 "spinless12_dihedral_reflection_odd": (24, False), "spinless10_k3": (10, False)}[name]
    assert fermi == basis.hasFermionSigns()
    rs = np.random.RandomState(len(name))
    sections = _random_sections(rs, spec, 8)
    if fermi and spec.particle == "spinless-fermion":  # the four-point function, always
        sections.append({"terms": [{"expression": "c†₀ c†₁ c₂ c₃", "sites": [[7, 2, 5, 0]]}]})
    if not fermi:  # sigma^y on overlapping sites, always
        sections.append({"terms": [{"expression": "σʸ₀ σˣ₁ σʸ₁ σᶻ₂ σʸ₂", "sites": [[4, 1, 8]]}]})
    nonzero = 0
    for sec in sections:
        op_spec = config.parse_operator(sec, spec)
        if not op_spec.terms:
            continue  # (a monomial that vanishes identically, e.g. sigma^+ sigma^+ on one site)
        op = Operator.fromSpec(basis, op_spec)
        vmax = max(abs(t[0]) for t in op_spec.terms)
        got = _as_maps(_average_hook(basis, op), M)
        want = _reference_average(_as_maps(op_spec.terms, M), perms, M, fermi, inv)
        worst = 0.0
        for x in set(got) | set(want):
            diff = np.asarray(got.get(x, 0.0)) - np.asarray(want.get(x, 0.0))
            worst = max(worst, float(np.abs(diff).max()))
        assert worst <= 1e-12 * vmax, (name, sec, worst)
        nonzero += any(np.abs(c).max() > 1e-3 * vmax for c in want.values())
    assert nonzero >= 4  # (the averages do not all vanish)


def test_average_of_an_invariant_operator_is_the_operator():
    """the Heisenberg ring commutes with its translations, its reflection and the inversion: the average gives it back"""
    cfg = E.ring(12, 6, 0, inv=1, reflect=0)
    basis = D.loadConfigFromDict(cfg)
    bonds = [[i, (i + 1) % 12] for i in range(12)]
    sec = {"terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}
    spec = config.parse_operator(sec, basis.spec)
    got = _as_maps(_average_hook(basis, Operator.fromSpec(basis, spec)), 12)
    want = _as_maps(spec.terms, 12)
    assert set(x for x, c in got.items() if np.abs(c).max() > 0) == set(x for x, c in want.items() if np.abs(c).max() > 0)
    for x in want:
        assert np.abs(got[x] - want[x]).max() <= 1e-12


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_that_need_no_device():
    L = _lib()
    from distributed_matvec_amd._lib import LsAmdError, LsHsBasis, LsHsOperator

    basis = D.loadConfigFromDict(E.ring(8, 4, 0))
    other = D.loadConfigFromDict(E.ring(8, 4, 1))
    sec = {"terms": [{"expression": "σˣ₀ σᶻ₁ σˣ₂", "sites": [[0, 3, 5]]}]}
    op = Operator.fromSpec(basis, config.parse_operator(sec, basis.spec))
    foreign_op = Operator.fromSpec(other, config.parse_operator(sec, other.spec))
    opp = C.POINTER(LsHsOperator)
    h = C.c_void_p()
    one = (C.c_uint64 * 1)(15)
    ops = (opp * 1)(op.payload)
    assert L.ls_amd_expect_create(C.byref(h), None, ops, 1, one, 1, None) == -1 and "ls_amd_expect_create: NULL basis" in _message()
    assert L.ls_amd_expect_create(None, basis.payload, ops, 1, one, 1, None) == -1 and "NULL handle" in _message()
    foreign = LsHsBasis()
    assert L.ls_amd_expect_create(C.byref(h), C.byref(foreign), ops, 1, one, 1, None) == -1 and "not built by this library" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, ops, 0, one, 1, None) == -1 and "no operators (n_ops = 0" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, None, 1, one, 1, None) == -1 and "no operators" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, (opp * 1)(), 1, one, 1, None) == -1 and "operator 0 is NULL" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, (opp * 1)(foreign_op.payload), 1, one, 1, None) == -1
    assert "operator 0 is an operator of another basis" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, ops, 1, one, 0, None) == -1 and "no rows" in _message()
    assert L.ls_amd_expect_create(C.byref(h), basis.payload, ops, 1, None, 5, None) == -1 and "NULL representatives" in _message()
    assert not h.value
    wide = D.loadConfigFromDict({"basis": R.Case(62, 2, gens=F.translations(62), secs=[0]).basis_config()})
    wide_op = Operator.fromSpec(wide, config.parse_operator({"terms": [{"expression": "n₀", "sites": [[3]]}]}, wide.spec))
    assert L.ls_amd_expect_create(C.byref(h), wide.payload, (opp * 1)(wide_op.payload), 1, one, 1, None) == -1
    assert "ls_amd_expect_create: projected fermionic bases of more than 60 modes" in _message()
    # a projected fermionic basis: a term that flips a mode outside its projector mask is no fermionic operator
    fermi = D.loadConfigFromDict({"basis": R.Case(8, 4, gens=F.translations(8), secs=[0]).basis_config()})
    bad = Operator.fromSpec(fermi, config.OperatorSpec([(1.0 + 0j, 0b0001, 0b0001, 0b0011, 0)]))
    assert L.ls_amd_expect_create(C.byref(h), fermi.payload, (opp * 1)(bad.payload), 1, one, 1, None) == -1
    assert "a term flips modes outside its projector mask" in _message() and "not a product of creation and annihilation operators" in _message()
    assert L.ls_amd_test_expect_average(fermi.payload, bad.payload, 0, None, None, None, None, None) == -1
    assert "ls_amd_test_expect_average: a term flips modes outside its projector mask" in _message()
    assert L.ls_amd_test_expect_average(None, op.payload, 0, None, None, None, None, None) == -1 and "NULL basis" in _message()
    assert L.ls_amd_test_expect_average(basis.payload, None, 0, None, None, None, None, None) == -1 and "operator 0 is NULL" in _message()
    assert L.ls_amd_test_expect_average(basis.payload, foreign_op.payload, 0, None, None, None, None, None) == -1 and "another basis" in _message()
    assert L.ls_amd_test_expect_average(basis.payload, op.payload, 4, None, None, None, None, None) == -1 and "NULL output" in _message()
    assert L.ls_amd_expect_num_terms(None) == -1 and "ls_amd_expect_num_terms: NULL plan" in _message()
    assert L.ls_amd_expect_num_groups(None) == -1 and "NULL plan" in _message()
    assert L.ls_amd_expect_kernel_name(None) is None and "NULL plan" in _message()
    assert L.ls_amd_expect_values(None, 0, None, None, None) == -1 and "ls_amd_expect_values: NULL plan" in _message()
    L.ls_amd_expect_destroy(None)
    # the Python entry points
    spinful = D.loadConfigFromDict({"basis": R.Case(4, up=(2, 2)).basis_config()})
    spinless = D.loadConfigFromDict({"basis": R.Case(6, 3).basis_config()})
    with pytest.raises(LsAmdError, match="pair_correlations"):
        D.dimer_correlations(spinful, None, None, [(0, 1)])
    with pytest.raises(LsAmdError, match="dimer_correlations"):
        D.pair_correlations(basis, None, None)
    with pytest.raises(LsAmdError, match="spinful-fermion basis, not a spinless one"):
        D.pair_correlations(spinless, None, None)
    with pytest.raises(LsAmdError, match="one partition"):
        D.ExpectationPlan(basis, [None, None], [sec])
    with pytest.raises(LsAmdError, match="contiguous 1-D int64"):
        D.ExpectationPlan(basis, np.arange(3), [sec])


def test_operator_sections_of_the_drivers():
    """the sections dimer_correlations and pair_correlations hand to the plan, as dense matrices on tiny systems"""
    from distributed_matvec_amd.expectation import dimer_section, pair_section

    def dense(spec_terms, M):
        A = np.zeros((1 << M, 1 << M), dtype=np.complex128)
        for x, c in _as_maps(spec_terms, M).items():
            a = np.arange(1 << M)
            A[a ^ x, a] += c
        return A

    sx, sy, sz = np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]])

    def site(op, q, M):  # site q <-> bit q: the factor of bit M - 1 comes first in the Kronecker product
        out = np.eye(1)
        for b in reversed(range(M)):
            out = np.kron(out, op if b == q else np.eye(2))
        return out

    def ss(i, j, M):
        return sum(site(o, i, M) @ site(o, j, M) for o in (sx, sy, sz)) / 4

    M = 5
    for a, b in (((0, 1), (2, 3)), ((0, 1), (1, 2)), ((3, 1), (3, 1)), ((2, 4), (4, 0)), ((1, 2), (2, 1))):
        got = dense(config.parse_operator(dimer_section(a, b)).terms, M)
        assert np.abs(got - ss(*a, M) @ ss(*b, M)).max() <= 1e-14, (a, b)
    # pairs: Delta+_i Delta_j on 2 sites (modes: up 0, 1; down 2, 3), against Jordan-Wigner matrices in the bit order
    import fermion_jw as JW

    spec = config.BasisSpec(number_sites=2, particle="spinful-fermion")
    c = [JW.annihilator(k, 4).toarray() for k in range(4)]
    for i in range(2):
        for j in range(2):
            delta_i, delta_j = c[i + 2] @ c[i], c[j + 2] @ c[j]
            got = dense(config.parse_operator(pair_section(i, j), spec).terms, 4)
            assert np.abs(got - delta_i.conj().T @ delta_j).max() <= 1e-14, (i, j)
