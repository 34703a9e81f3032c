"""Cross-sector operators between bases with DIFFERENT symmetry groups, without a device: the new C entries
(ls_amd_cross_create_groups, ls_amd_operator_maps_subgroup_sector) are declared, exported and refuse NULL; the subgroup rule of
groups="restrict" accepts exactly where dense conjugation U_g A U_g^+ = chi2(g) conj(chi1(g)) A holds on 6-8 sites -- with the
target's generator looked up among the PRODUCTS of the source's generators -- and names the generator otherwise; the signed rule
does the same for projected fermions against the signed projectors; groups="same" keeps its refusals through the new entry point;
unequal number_sites, particle types and a target group outside the source group have their own messages; and the kernels of
csrc/k_cross_project*.hip are in the compiler's resource report within the budget of the existing cross kernels."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import cross_groups_reference as G
import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_symm as F
from distributed_matvec_amd import config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _operator(basis_cfg, op_cfg):
    basis = D.loadConfigFromDict(basis_cfg)
    return basis, D.Operator.fromSpec(basis, config.parse_operator(op_cfg, basis.spec))


def _maps(src_cfg, dst_cfg, op_cfg):
    """(bool, message) of the subgroup rule"""
    _, op = _operator(src_cfg, op_cfg)
    target = D.loadConfigFromDict(dst_cfg)
    ok = op.mapsSector(target, subgroup=True)
    msg = ""
    if not ok:
        with pytest.raises(D.LsAmdError) as e:
            op.mapsSector(target, explain=True, subgroup=True)
        msg = str(e.value)
    return ok, msg


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_cross_create_groups\s*\(\s*ls_amd_cross\s*\*\*\s*\w+\s*,\s*ls_hs_operator\s+const\s*\*\s*\w+\s*,\s*ls_hs_basis\s+const"
                     r"\s*\*\s*\w+\s*,\s*ls_amd_dtype\s+\w+\s*,\s*int\s+mode\s*,", header)
    assert re.search(r"int\s+ls_amd_operator_maps_subgroup_sector\s*\(\s*ls_hs_operator\s+const\s*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*\s*\w+\s*\)\s*;", header)
    assert re.search(r"LS_AMD_CROSS_SAME\s*=\s*0\s*,\s*LS_AMD_CROSS_RESTRICT\s*=\s*1\s*,\s*LS_AMD_CROSS_PROJECT\s*=\s*2", header)
    L = _lib()
    assert hasattr(L, "ls_amd_cross_create_groups") and hasattr(L, "ls_amd_operator_maps_subgroup_sector")
    from distributed_matvec_amd import kpm

    assert D.CrossSectorPlan.GROUPS == {"same": 0, "restrict": 1, "project": 2}
    assert "groups" in kpm.spectral_function.__code__.co_varnames and "subgroup" in D.Operator.mapsSector.__code__.co_varnames


def test_null_arguments_and_unknown_modes_are_refused_without_a_device():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    basis, op = _operator(X.ring(8, 4, 0), X.sz_q(8, 3))
    assert L.ls_amd_operator_maps_subgroup_sector(None, basis.payload) == -1 and "NULL" in err()
    assert L.ls_amd_operator_maps_subgroup_sector(op.payload, None) == -1 and "NULL" in err()
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    for mode in (0, 1, 2):
        assert L.ls_amd_cross_create_groups(None, op.payload, basis.payload, 1, mode, reps, 4, reps, 4, None) == -1 and "NULL" in err()
        assert L.ls_amd_cross_create_groups(C.byref(h), None, basis.payload, 1, mode, reps, 4, reps, 4, None) == -1 and "NULL" in err()
        assert L.ls_amd_cross_create_groups(C.byref(h), op.payload, None, 1, mode, reps, 4, reps, 4, None) == -1 and "NULL" in err()
        assert L.ls_amd_cross_create_groups(C.byref(h), op.payload, basis.payload, 1, mode, None, 4, reps, 4, None) == -1 and "NULL" in err()
    assert L.ls_amd_cross_create_groups(C.byref(h), op.payload, basis.payload, 1, 3, reps, 4, reps, 4, None) == -1 and "unknown mode 3" in err()
    assert h.value is None


def _create(src_cfg, dst_cfg, op_cfg, dtype, mode):
    """the message of ls_amd_cross_create_groups for a pair it refuses before any device work (the representatives are never read)"""
    L = _lib()
    _, op = _operator(src_cfg, op_cfg)
    target = D.loadConfigFromDict(dst_cfg)
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    assert L.ls_amd_cross_create_groups(C.byref(h), op.payload, target.payload, dtype, mode, reps, 4, reps, 4, None) == -1 and h.value is None
    return L.ls_amd_last_error().decode()


def test_same_keeps_its_refusals_through_the_new_entry_point():
    src, op = X.ring(8, 4, 0), X.sz_q(8, 0)
    other = G.with_generators(8, 4, [(G.translation(8, 2), 0)])
    assert "different generators" in _create(src, other, op, 1, 0)
    assert "different generators" in _create(src, X.ring(8, 4, 0, 0), op, 1, 0)
    assert "one basis only" in _create(src, X.ring(8, 4, 0, inversion=1), op, 1, 0)
    assert "different number_sites" in _create(src, X.ring(10, 5, 0), op, 1, 0)
    assert "generator 0" in _create(src, X.ring(8, 4, 3), X.sz_q(8, 2), 1, 0)
    assert "c128" in _create(src, X.ring(8, 4, 3), X.sz_q(8, 3), 0, 0)


def test_new_modes_refuse_by_name_before_any_device_work():
    full = G.ring(8, 4, 0, 0, 1)
    fermi = {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 4}}
    for mode in (1, 2):
        assert "different number_sites (8 and 10)" in _create(full, G.ring(10, 5, 3), X.sz_q(8, 3), 1, mode)
        assert "particle types" in _create(full, fermi, X.sz_q(8, 3), 1, mode)
        # f64: a complex operator, or complex characters on the target
        assert "f64 needs a real operator and +-1 characters on both bases" in _create(full, G.ring(8, 4, 3), X.sz_q(8, 3), 0, mode)
    assert "f64 needs a real operator and +-1 characters on both bases" in _create(full, G.ring(8, 4, 3), G.sz_site(0), 0, 2)
    # restrict runs its rule at creation; project asks nothing of the operator (sigma^z_0 passes the lines above in mode 2 only)
    assert "generator 0" in _create(full, G.ring(8, 4, 3), G.sz_site(0), 1, 1)
    msg = _create(G.with_generators(8, 4, [(G.reflection(8), 0)]), G.with_generators(8, 4, [(G.translation(8, 2), 0)]), X.sz_q(8, 0), 1, 1)
    assert "generator 0" in msg and 'groups="project"' in msg


# ---- the subgroup rule against dense conjugation -------------------------------------------------------------------------------
def _spin_pairs():
    """(name, source, target, operator): sources with more symmetry than their targets, on 6 and 8 sites"""
    out = []
    for L in (6, 8):
        dihedral = G.ring(L, L // 2, 0, 0, 1)
        for dk in range(L):
            out.append((f"L{L}_sz_q{dk}_into_k2", dihedral, G.ring(L, L // 2, 2), X.sz_q(L, dk)))
        out.append((f"L{L}_staggered_into_refl1", dihedral, G.with_generators(L, L // 2, [(G.reflection(L), 1)]), X.staggered_z(L)))
        out.append((f"L{L}_staggered_into_refl0", dihedral, G.with_generators(L, L // 2, [(G.reflection(L), 0)]), X.staggered_z(L)))
        out.append((f"L{L}_staggered_into_k_half_inv-1", dihedral, G.ring(L, L // 2, L // 2, inversion=-1), X.staggered_z(L)))
        out.append((f"L{L}_staggered_into_k_half_inv+1", dihedral, G.ring(L, L // 2, L // 2, inversion=1), X.staggered_z(L)))
        out.append((f"L{L}_sz0_into_k1", dihedral, G.ring(L, L // 2, 1), G.sz_site(0)))
        # the target's generators are PRODUCTS of the source's: T R (a reflection about another axis) and T^2
        TR = G.compose(G.translation(L), G.reflection(L))
        for s in (0, 1):
            out.append((f"L{L}_sz_q0_into_TR{s}", dihedral, G.with_generators(L, L // 2, [(TR, s)]), X.sz_q(L, 0)))
            out.append((f"L{L}_staggered_into_TR{s}", dihedral, G.with_generators(L, L // 2, [(TR, s)]), X.staggered_z(L)))
        for s in range(L // 2):
            out.append((f"L{L}_sz_q1_into_T2_{s}", G.ring(L, L // 2, 1), G.with_generators(L, L // 2, [(G.translation(L, 2), s)]), X.sz_q(L, 1)))
        # a source in a non-trivial sector: chi1 enters the factor
        out.append((f"L{L}_sz_q1_from_k1_refl_none", G.ring(L, L // 2, 1), G.ring(L, L // 2, 2), X.sz_q(L, 1)))
        out.append((f"L{L}_staggered_from_refl1", G.ring(L, L // 2, L // 2, 1, -1), G.with_generators(L, L // 2, [(G.reflection(L), 0)]), X.staggered_z(L)))
    return out


SPIN_PAIRS = _spin_pairs()


@pytest.mark.parametrize("name,src,dst,op", SPIN_PAIRS, ids=[p[0] for p in SPIN_PAIRS])
def test_subgroup_rule_accepts_exactly_where_dense_conjugation_holds(name, src, dst, op):
    defects = G.subgroup_defects(src, dst, op)
    assert defects is not None, "every pair here has its target group inside the source group"
    ok, msg = _maps(src, dst, op)
    bad = [n for n, d in defects if d > 1e-12]
    assert all(d <= 1e-13 or d > 1e-3 for _, d in defects), defects  # no borderline case
    assert ok == (not bad), (defects, msg)
    if bad:
        assert bad[0] in msg, (bad, msg)  # the first generator that fails is the one named


def test_subgroup_rule_decides_both_ways():
    verdicts = [all(d <= 1e-12 for _, d in G.subgroup_defects(s, d_, o)) for _, s, d_, o in SPIN_PAIRS]
    assert sum(verdicts) >= 12 and len(verdicts) - sum(verdicts) >= 12


def test_a_target_without_symmetries_is_always_a_subgroup():
    plain = {"basis": {"number_spins": 8, "hamming_weight": 4, "symmetries": []}}
    assert _maps(G.ring(8, 4, 0, 0, 1), plain, G.sz_site(0))[0]
    assert _maps(G.ring(8, 4, 3), plain, G.hop_q_plus_sz0(8, 1))[0]


def test_a_target_group_outside_the_source_group_names_the_generator_and_points_to_project():
    refl_only = G.with_generators(8, 4, [(G.reflection(8), 0)])
    T2 = G.with_generators(8, 4, [(G.reflection(8), 0), (G.translation(8, 2), 0)])
    assert G.subgroup_defects(refl_only, T2, X.sz_q(8, 0)) is None
    ok, msg = _maps(refl_only, T2, X.sz_q(8, 0))
    assert not ok and "generator 1" in msg and "generator 0" not in msg and 'groups="project"' in msg, msg
    # upwards: a translations-only source into a dihedral target
    ok, msg = _maps(G.ring(8, 4, 0), G.ring(8, 4, 0, 0), X.sz_q(8, 0))
    assert not ok and "generator 1" in msg and 'groups="project"' in msg, msg
    # the inversion on the target only
    ok, msg = _maps(G.ring(8, 4, 0), G.ring(8, 4, 0, inversion=1), X.sz_q(8, 0))
    assert not ok and "spin inversion" in msg and 'groups="project"' in msg, msg
    # ... on the source only is fine
    assert _maps(G.ring(8, 4, 0, inversion=1), G.ring(8, 4, 3), X.sz_q(8, 3))[0]


def test_unequal_sites_and_particle_types_have_their_own_messages():
    src, op = G.ring(8, 4, 0, 0, 1), X.sz_q(8, 0)
    ok, msg = _maps(src, G.ring(10, 5, 0), op)
    assert not ok and "different number_sites (8 and 10)" in msg, msg
    ok, msg = _maps(src, {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 4}}, op)
    assert not ok and "particle types" in msg, msg


def test_same_generators_give_the_answers_of_the_existing_rule():
    """where groups="same" applies, the subgroup rule decides as ls_amd_operator_maps_sector does (chi1 from the closure is the
    generator's own character), on the cases of tests/cross_sector_reference.py and their wrong neighbours"""
    for name, (src, dst, op, _) in sorted(X.CASES.items()):
        assert _maps(src, dst, op)[0], name
    ok, msg = _maps(X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 2))
    assert not ok and "generator 0" in msg, msg
    s = X.ring(8, 4, 0, 0, 1)
    ok, msg = _maps(s, X.ring(8, 4, 4, 0, -1), X.staggered_z(8))
    assert not ok and "generator 1" in msg and "generator 0" not in msg, msg
    ok, msg = _maps(s, X.ring(8, 4, 4, 1, 1), X.staggered_z(8))
    assert not ok and "spin inversion" in msg and "generator" not in msg, msg


# ---- projected fermions: the signed rule over the target's generators ------------------------------------------------------------
def _fermi_maps(src, dst, model):
    spinful = src["n_up"] is not None
    return _maps(R.basis_config(src), R.basis_config(dst), R.operator_section(model, spinful))


FERMI_PAIRS = {
    # 10-mode dihedral (0, 0) source into translation sectors (the cases of the GPU tests), and their wrong neighbours
    "n_q3": (R.sector(10, 4, F.dihedral(10), [0, 0]), R.sector(10, 4, F.translations(10), [3]), R.n_q(10, 3), True),
    "n_q3_wrong_k": (R.sector(10, 4, F.dihedral(10), [0, 0]), R.sector(10, 4, F.translations(10), [4]), R.n_q(10, 3), False),
    "cdag_q2": (R.sector(10, 4, F.dihedral(10), [0, 0]), R.sector(10, 5, F.translations(10), [2]), R.c_dag(10, 2), True),
    "cdag_q2_wrong_k": (R.sector(10, 4, F.dihedral(10), [0, 0]), R.sector(10, 5, F.translations(10), [1]), R.c_dag(10, 2), False),
    "cdag_site0": (R.sector(10, 4, F.dihedral(10), [0, 0]), R.sector(10, 5, F.translations(10), [2]), [(1.0, [("+", 0, 0)])], False),
    # spinful: spin_flip on the source only
    "spinful_n_q1": (R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1), R.sector(4, 4, F.translations(4), [1], n_up=2), R.n_q(4, 1, True), True),
    "spinful_n_q1_wrong_k": (R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1), R.sector(4, 4, F.translations(4), [2], n_up=2), R.n_q(4, 1, True), False),
}


@pytest.mark.parametrize("name", sorted(FERMI_PAIRS))
def test_signed_subgroup_rule_agrees_with_the_signed_projectors(name):
    src, dst, model, want = FERMI_PAIRS[name]
    ok, msg = _fermi_maps(src, dst, model)
    assert ok == want, msg
    ref = R.reference(src, dst, model)
    assert ref["norm"] > 0.5
    if want:
        assert ref["leak"] <= 4e-14, ref["leak"]  # nothing leaves the target sector
    else:
        assert "generator 0" in msg and ref["leak"] > 0.1 * ref["norm"], (msg, ref["leak"], ref["norm"])


def test_spin_flip_on_the_target_only_is_no_subgroup():
    src = R.sector(4, 4, F.translations(4), [0], n_up=2)
    dst = R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1)
    ok, msg = _fermi_maps(src, dst, R.n_q(4, 0, True))
    assert not ok and "spin_flip" in msg and 'groups="project"' in msg, msg


# ---- the dense references of the GPU tests are what the issue says they are ------------------------------------------------------
def test_restricted_matrix_is_the_full_image_over_the_target_norm():
    """<r'|_2 A|psi> = (A psi^)(r') / n2(r') when the target group is a subgroup and A is covariant under it: the identity that
    groups="restrict" rests on, by the dense projectors (10-site ring, (k = 0, refl 0, inv +1) -> (k = 3), S^z_q)"""
    src, dst, op = G.ring(10, 5, 0, 0, 1), G.ring(10, 5, 3), X.sz_q(10, 3)
    ref = G.dense(src, dst, op)
    assert (len(ref["src"]), len(ref["dst"])) == (13, 25)
    assert ref["leak"] <= 1e-12 and ref["norm"] > 1.0
    rows = ref["image"][ref["dst"].astype(np.int64)] / ref["n2"][:, None]
    assert np.abs(rows - ref["matrix"]).max() <= 1e-13
    # ... and sigma^z_0 is covariant under nothing: the image leaves the sector and the shortcut is wrong
    loc = G.dense(src, G.ring(10, 5, 2), G.sz_site(0))
    assert loc["leak"] > 1.0
    short = loc["image"][loc["dst"].astype(np.int64)] / loc["n2"][:, None]
    assert np.abs(short - loc["matrix"]).max() > 0.1


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["k_cross_project.hip", "k_cross_project_fermi.hip"])
def test_project_kernels_in_the_resource_report(source):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    stats = kernel_resources.resources(source=source)
    mine = {k: v for k, v in stats.items() if k.startswith("_Z15k_cross_projectI")}
    # {32-, 64-bit words} x {f64 | c128 x {real coefficient | +-1 source characters, complex coefficient | complex source characters}}
    assert len(mine) == 8 and len(stats) == 8, sorted(stats)
    pull = kernel_resources.resources(source="k_cross.hip")
    lds_budget = max(v["lds"] for v in pull.values())
    for name, v in stats.items():
        assert v["scratch"] == 0, (name, v)
        assert v["lds"] <= lds_budget, (name, v, lds_budget)  # within the LDS of the existing cross kernels
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (name, v)
