"""Cross-sector operators on projected fermionic bases without a device: the signed covariance rule
(ls_amd_operator_maps_sector_signed, Operator.mapsSector(..., signs=True)) accepts the cases that the signed projectors of
tests/fermion_cross_reference.py say map one sector into another and refuses the neighbouring momentum by naming the generator; it
agrees with dense U_g A U_g^+ on 6 modes for a translation, a reflection and a lifted flip at every dk; the plain rule keeps its
refusal and the signed entry gives the plain rule's answer for spins; tables that are no fermionic operators are refused by
name."""
import os
import re

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_jw as J
import fermion_symm as F
from distributed_matvec_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operator(basis_cfg, op_cfg):
    basis = D.loadConfigFromDict(basis_cfg)
    return basis, D.Operator.fromSpec(basis, config.parse_operator(op_cfg, basis.spec))


def _maps(src_cfg, dst_cfg, op_cfg, signs=True):
    """(bool, message)"""
    _, op = _operator(src_cfg, op_cfg)
    target = D.loadConfigFromDict(dst_cfg)
    ok = op.mapsSector(target, signs=signs)
    msg = ""
    if not ok:
        with pytest.raises(D.LsAmdError) as e:
            op.mapsSector(target, explain=True, signs=signs)
        msg = str(e.value)
    return ok, msg


def _case(name, model=None):
    src, dst, m, _, _, _ = R.CASES[name]
    return R.basis_config(src), R.basis_config(dst), R.operator_section(model or m, R.is_spinful(name))


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_operator_maps_sector_signed\s*\(\s*ls_hs_operator\s+const\s*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*\s*\w+\s*\)\s*;", header)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert hasattr(L, "ls_amd_operator_maps_sector_signed")
    basis, op = _operator(*_case("L8_cdag_q3")[0::2])
    assert L.ls_amd_operator_maps_sector_signed(None, basis.payload) == -1 and "NULL" in L.ls_amd_last_error().decode()
    assert L.ls_amd_operator_maps_sector_signed(op.payload, None) == -1 and "NULL" in L.ls_amd_last_error().decode()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_signed_rule_accepts_the_covariant_cases(name):
    ok, msg = _maps(*_case(name))
    assert ok, msg
    # ... and the signed projectors agree: nothing leaves the target sector, and the sizes are those of the table
    ref = R.case_reference(name)
    n_src, n_dst, zero = R.CASES[name][5]
    assert ref["leak"] <= 4e-14 and ref["norm"] > 1.0
    assert (len(ref["src"]), len(ref["dst"])) == (n_src, n_dst)
    if zero == "> 0":
        assert ref["pull_dropped"] > 0
    elif zero is not None:
        assert ref["pull_dropped"] == zero
    assert ref["images"] > 0


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_signed_rule_refuses_a_wrong_dk_and_names_the_generator(name):
    src, dst, model, dk, _, _ = R.CASES[name]
    wrong = R.wrong_dk_model(name)
    ok, msg = _maps(*_case(name, wrong))
    L = src["L"]
    assert not ok and "generator 0" in msg and f"exp(-2 pi i {dst['secs'][0] - src['secs'][0]} / {L})" in msg, msg
    # by the projectors the image leaves the target sector altogether -- no rounding effect
    ref = R.reference(src, dst, wrong)
    assert ref["leak"] > 0.5 * ref["norm"] > 0.5


def test_signed_rule_refuses_the_other_reflection_sector():
    src, dst, model, _, _, _ = R.CASES["L8_dihedral_cdag_q0"]
    odd = dict(dst, secs=[0, 1])
    ok, msg = _maps(R.basis_config(src), R.basis_config(odd), R.operator_section(model, False))
    assert not ok and "generator 1" in msg and "generator 0" not in msg, msg
    ref = R.reference(src, odd, model)
    assert ref["leak"] > 0.5 * ref["norm"] > 0.5


# ---- brute force on 6 modes ------------------------------------------------------------------------------------------------------
def _dense_u(p):
    """U_g on the 2^M Fock space: U_g|a> = sign(g, a)|g.a>"""
    M = len(p)
    U = np.zeros((1 << M, 1 << M))
    for a in range(1 << M):
        U[F.apply(p, a), a] = F.sign(p, a)
    return U


def _six_mode_operators(q):
    """c+_q, c_q, n_q, a ring hop, a pair operator and a four-operator monomial on a 6-site spinless ring"""
    L = 6
    ph = lambda j: R.phase(L, q, j)  # noqa: E731
    return {
        "cdag_q": [(ph(j), [("+", j, 0)]) for j in range(L)],
        "c_q": [(ph(j), [("-", j, 0)]) for j in range(L)],
        "n_q": [(ph(j), [("n", j, 0)]) for j in range(L)],
        "hop": [(ph(j), [("+", j, 0), ("-", (j + 1) % L, 0)]) for j in range(L)],
        "pair": [(ph(j), [("+", j, 0), ("+", (j + 2) % L, 0)]) for j in range(L)],
        "four": [(ph(j), [("+", j, 0), ("+", (j + 1) % L, 0), ("-", (j + 3) % L, 0), ("n", (j + 4) % L, 0)]) for j in range(L)],
    }


GENERATORS = {"translation": [1, 2, 3, 4, 5, 0], "reflection": [5, 4, 3, 2, 1, 0], "lifted_flip": [3, 4, 5, 0, 1, 2]}


@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_signed_rule_is_the_dense_conjugation_on_six_modes(gen):
    """max |U_g A U_g^+ - f A| on the 64 x 64 matrices is zero exactly when the rule accepts, f = exp(-2 pi i dk / order)"""
    p = GENERATORS[gen]
    order = 6 if gen == "translation" else 2
    U = _dense_u(p)
    assert np.abs(U @ U.T - np.eye(64)).max() == 0 and (U < 0).any()  # a signed permutation matrix
    accepted = refused = 0
    for q in (0, 1, 3):
        for name, model in _six_mode_operators(q).items():
            A = J.dense(model, 6, False).toarray()
            UAU = U @ A @ U.T
            for dk in range(order):
                defect = np.abs(UAU - np.exp(-2j * np.pi * dk / order) * A).max()
                assert defect <= 1e-14 or defect >= 0.1, (gen, name, q, dk, defect)  # nothing in between
                src = {"basis": {"particle": "spinless-fermion", "number_sites": 6, "number_particles": 3, "symmetries": [{"permutation": p, "sector": 0}]}}
                dst = {"basis": {"particle": "spinless-fermion", "number_sites": 6, "number_particles": 3, "symmetries": [{"permutation": p, "sector": dk}]}}
                ok, msg = _maps(src, dst, R.operator_section(model, False))
                assert ok == (defect <= 1e-14), (gen, name, q, dk, defect, msg)
                if not ok:
                    assert "generator 0" in msg, msg
                accepted += ok
                refused += not ok
    assert accepted >= 6 and refused >= 6, (accepted, refused)


# ---- what stays as it was --------------------------------------------------------------------------------------------------------
def test_plain_rule_still_refuses_projected_fermionic_bases():
    for name in ("L8_cdag_q3", "spinful_L6_sz_q2"):
        ok, msg = _maps(*_case(name), signs=False)
        assert not ok and "projected fermionic" in msg, msg


@pytest.mark.parametrize("name", sorted(X.CASES))
def test_signed_entry_gives_the_plain_answer_for_spins(name):
    src, dst, op, _ = X.CASES[name]
    assert _maps(src, dst, op, signs=True) == _maps(src, dst, op, signs=False) == (True, "")


def test_signed_entry_gives_the_plain_refusals_for_spins():
    src, dst = X.ring(8, 4, 0), X.ring(8, 4, 3)
    for s, d, op in ((src, dst, X.sz_q(8, 2)), (X.ring(8, 4, 0, 0, 1), X.ring(8, 4, 4, 0, -1), X.staggered_z(8)),
                     (X.ring(8, 4, 0, 0, 1), X.ring(8, 4, 4, 1, 1), X.staggered_z(8)), (src, X.ring(10, 5, 0), X.sz_q(8, 0))):
        plain, signed = _maps(s, d, op, signs=False), _maps(s, d, op, signs=True)
        assert not plain[0] and plain == signed, (plain, signed)
    # unprojected fermions: no group, nothing to check, by either entry
    free = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2}}
    to = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 5, "number_up": 3}}
    assert _maps(free, to, {"terms": J.yaml_terms([(1.0, [("+", 2, 0)])], True)}, signs=True)[0]


def test_preconditions_of_the_signed_rule_have_their_own_messages():
    src_cfg, dst_cfg, op = _case("L8_cdag_q3")
    other = R.basis_config(R.sector(8, 4, [[(i + 2) % 8 for i in range(8)]], [0]))
    ok, msg = _maps(src_cfg, other, op)
    assert not ok and "different generators" in msg
    ok, msg = _maps(src_cfg, R.basis_config(R.sector(8, 4, F.dihedral(8), [0, 0])), op)  # one generator more
    assert not ok and "different generators" in msg
    ok, msg = _maps(src_cfg, {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 4}}, op)  # none
    assert not ok and "different generators" in msg
    ok, msg = _maps(src_cfg, R.basis_config(R.sector(10, 4, F.translations(10), [3])), op)
    assert not ok and "different number_sites" in msg
    ok, msg = _maps(src_cfg, R.basis_config(R.sector(4, 4, F.translations(4), [3], n_up=2)), op)
    assert not ok and "particle types" in msg


# ---- tables that are no fermionic operators --------------------------------------------------------------------------------------
def _raw(terms, L=40):
    sec = R.sector(L, 2, F.translations(L), [0])
    basis = D.loadConfigFromDict(R.basis_config(sec))
    return D.Operator.fromSpec(basis, config.OperatorSpec(terms)), D.loadConfigFromDict(R.basis_config(sec))


def test_a_flip_outside_the_projector_mask_is_refused_by_name():
    op, target = _raw([(1.0 + 0j, 0b0001, 0b0001, 0b0011, 0)])  # x = {0, 1}, m = {0}
    assert not op.mapsSector(target, signs=True)
    with pytest.raises(D.LsAmdError, match="flips modes outside its projector mask"):
        op.mapsSector(target, explain=True, signs=True)


def test_a_sign_mask_that_is_no_jordan_wigner_string_is_refused_by_name():
    # c+_30 WITHOUT its string: s = 0 differs from J(x) = the 30 modes below on more modes than the rule expands
    op, target = _raw([(1.0 + 0j, 1 << 30, 0, 1 << 30, 0)])
    assert not op.mapsSector(target, signs=True)
    with pytest.raises(D.LsAmdError, match="not a fermionic operator"):
        op.mapsSector(target, explain=True, signs=True)
    # ... and WITH it the same table is one entry per site: sum_j c+_j on 40 modes maps k = 0 into k = 0
    terms = [(1.0 + 0j, 1 << j, 0, 1 << j, (1 << j) - 1) for j in range(40)]
    op, target = _raw(terms)
    assert op.mapsSector(target, explain=True, signs=True)
