"""Projected spinless-fermion bases without a device: the independent reference (tests/fermion_symm.py) against counting, the host
mirror of the device sign code (closed forms against the sign table, the table against inversion counting, up to bit 63), both
YAML loaders on spinless files with `symmetries:`, and the refusals that stay (spinful bases)."""
import itertools
from math import comb

import numpy as np
import pytest
import yaml

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib, config
from fermion_jw import ring, yaml_terms
from fermion_symm import closure, dihedral, representatives, sign, state_info, torus, translations, tv_model
from helpers import product_terms


def sectors_of(L, gens):
    orders = [len(closure(L, [p], [0])) for p in gens]
    for secs in itertools.product(*[range(o) for o in orders]):
        try:
            yield list(secs), closure(L, gens, list(secs))
        except ValueError:
            continue


@pytest.mark.parametrize("L,N,gens", [(6, 3, translations(6)), (7, 2, translations(7)), (8, 4, translations(8)), (9, 3, translations(9)),
                                      (6, 2, torus(3, 2)), (9, 4, torus(3, 3, point_group=False))])
def test_reference_sector_dimensions_sum_to_the_weight_space(L, N, gens):
    # abelian groups: the one-dimensional sectors are all the irreducible representations
    assert sum(len(representatives(L, N, g)[0]) for _, g in sectors_of(L, gens)) == comb(L, N)


def test_reference_vanishing_orbit_0101():
    g = closure(4, translations(4), [0])
    t2 = [2, 3, 0, 1]
    assert sign(t2, 0b0101) == -1
    rep, _, norm = state_info(g, 0b0101)
    assert rep == 0b0101 and norm == 0.0
    reps, _ = representatives(4, 2, g)
    assert list(reps) == [0b0011]  # k = 0 keeps one state: momenta 1 + 3 = 0 mod 4 is the only pair


def create(L, N, gens, secs):
    import ctypes as C

    lib = _lib.load()
    ng = len(gens)
    perms = (C.c_int * max(1, ng * L))(*[v for p in gens for v in p])
    sectors = (C.c_int * max(1, ng))(*secs)
    b = lib.ls_hs_create_spinless_fermion_basis(L, N, ng, perms, sectors)
    assert b, lib.ls_amd_last_error().decode()
    return lib, b


def permutation_of(lib, b, g, L):
    """p with (g.a)[i] = a[p_i], read off single-mode states"""
    p = [0] * L
    for src in range(L):
        out = int(lib.ls_amd_basis_apply_group_element(b, g, 1 << src))
        p[out.bit_length() - 1] = src
    return p


def random_generator(rs, L):
    """a random permutation of order <= 6: disjoint 2- and 3-cycles on shuffled modes (the closure stays small at 64 modes)"""
    idx = list(rs.permutation(L))
    p = list(range(L))
    while len(idx) >= 3:
        k = int(rs.choice([2, 3]))
        cyc, idx = idx[:k], idx[k:]
        for a, b in zip(cyc, cyc[1:] + cyc[:1]):
            p[a] = b
    return p


@pytest.mark.parametrize("L", [5, 12, 31, 32, 33, 48, 63, 64])
def test_host_sign_closed_forms_table_and_inversion_count(L):
    rs = np.random.RandomState(L)
    for gens in (dihedral(L), [random_generator(rs, L)], [random_generator(rs, L)]):  # (two random ones span a huge group)
        lib, b = create(L, -1, gens, [0] * len(gens))
        try:
            assert lib.ls_amd_basis_fermion_signs(b) == 1
            order = lib.ls_amd_basis_group_order(b)
            states = [int(v) for v in rs.randint(0, 2**62, size=24, dtype=np.uint64)]
            states = [s | (1 << 63) if L == 64 and i % 2 else s for i, s in enumerate(states)]
            mask = (1 << L) - 1
            states = [s & mask for s in states] + [mask, 1 << (L - 1), (1 << (L - 1)) | 1]
            for g in range(0, order, max(1, order // 24)):
                p = permutation_of(lib, b, g, L)
                for a in states:
                    want = sign(p, a)
                    assert lib.ls_amd_test_fermion_sign(b, g, a, 1) == want, (L, g, hex(a))
                    assert lib.ls_amd_test_fermion_sign(b, g, a, 0) == want, (L, g, hex(a))
        finally:
            lib.ls_hs_destroy_basis(b)


def test_unprojected_and_spin_bases_carry_no_signs():
    lib = _lib.load()
    basis, _ = D.loadConfigFromDict({"basis": {"particle": "spinless-fermion", "number_sites": 6, "number_particles": 3},
                                     "hamiltonian": {"terms": yaml_terms(tv_model(ring(6)), False)}}, hamiltonian=True)
    assert not basis.hasFermionSigns() and not basis.requiresProjection()
    spin, _ = D.loadConfigFromDict(config.heisenberg_chain_config(8, symm=True), hamiltonian=True)
    assert not spin.hasFermionSigns()
    assert lib.ls_amd_test_fermion_sign(spin.payload, 1, 3, 1) == 0


def spinless_symm_cfg(L, N, gens, secs, model):
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N,
                      "symmetries": [{"permutation": p, "sector": s} for p, s in zip(gens, secs)]},
            "hamiltonian": {"terms": yaml_terms(model, False)}}


LOADER_CASES = {
    "ring_10_dihedral": spinless_symm_cfg(10, 5, dihedral(10), [0, 1], tv_model(ring(10), V=0.7)),
    "ring_12_k5_phase": spinless_symm_cfg(12, 4, translations(12), [5], tv_model(ring(12), V=0.3, phase=0.2)),
    "torus_4x4": spinless_symm_cfg(16, 3, torus(4, 4), [2, 2, 0, 1], tv_model(ring(16))),
    "ring_64": spinless_symm_cfg(64, 3, translations(64), [7], tv_model(ring(64))),
}


@pytest.mark.parametrize("name", sorted(LOADER_CASES))
def test_c_and_python_loaders_agree_on_spinless_symmetries(name):
    cfg = LOADER_CASES[name]
    lib = _lib.load()
    conf = lib.ls_amd_load_yaml_config_from_string(yaml.safe_dump(cfg, allow_unicode=True).encode("utf-8"))
    assert conf, lib.ls_amd_last_error().decode()
    try:
        c = conf.contents
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        b = c.basis.contents
        assert (b.number_sites, b.number_particles, b.number_up, b.particle_type) == \
            (basis.numberSites(), basis.numberParticles(), basis.numberUp(), basis.particleType())
        assert bool(b.requires_projection) and basis.requiresProjection()
        assert lib.ls_amd_basis_fermion_signs(c.basis) == 1 and basis.hasFermionSigns()
        order = lib.ls_amd_basis_group_order(c.basis)
        assert order == lib.ls_amd_basis_group_order(basis.payload) == len(closure(cfg["basis"]["number_sites"],
                                                                                     [s["permutation"] for s in cfg["basis"]["symmetries"]],
                                                                                     [s["sector"] for s in cfg["basis"]["symmetries"]]))
        import ctypes as C

        for g in range(order):
            cr, ci, pr, pi = C.c_double(), C.c_double(), C.c_double(), C.c_double()
            lib.ls_amd_basis_group_character(c.basis, g, C.byref(cr), C.byref(ci))
            lib.ls_amd_basis_group_character(basis.payload, g, C.byref(pr), C.byref(pi))
            assert (cr.value, ci.value) == (pr.value, pi.value)
            assert lib.ls_amd_basis_apply_group_element(c.basis, g, 0b1011) == lib.ls_amd_basis_apply_group_element(basis.payload, g, 0b1011)
        assert product_terms(D.Operator(c.hamiltonian, owning=False)) == product_terms(h)
    finally:
        lib.ls_hs_destroy_yaml_config(conf)


def test_spinful_symmetries_are_still_refused():
    cfg = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 2,
                     "symmetries": [{"permutation": [1, 2, 3, 0], "sector": 0}]},
           "hamiltonian": {"terms": [{"expression": "n₀↑", "sites": [[0]]}]}}
    with pytest.raises(ValueError, match="symmetries"):
        config.parse_basis(cfg)
    lib = _lib.load()
    assert not lib.ls_amd_load_yaml_config_from_string(yaml.safe_dump(cfg, allow_unicode=True).encode("utf-8"))
    assert "symmetries" in lib.ls_amd_last_error().decode()


def test_bad_spinless_symmetries_are_refused_alike():
    for syms, what in (([{"permutation": [1, 2, 0], "sector": 0}], "symmetries[0]"),
                       ([{"permutation": [1, 1, 2, 3], "sector": 0}], "not a permutation")):
        cfg = {"basis": {"particle": "spinless-fermion", "number_sites": 4, "number_particles": 2, "symmetries": syms},
               "hamiltonian": {"terms": [{"expression": "n₀", "sites": [[0]]}]}}
        lib = _lib.load()
        assert not lib.ls_amd_load_yaml_config_from_string(yaml.safe_dump(cfg).encode("utf-8"))
        assert what in lib.ls_amd_last_error().decode()
        with pytest.raises((ValueError, D.LsAmdError), match=what.replace("[", r"\[").replace("]", r"\]")):
            D.loadConfigFromDict(cfg, hamiltonian=True)


def test_adopt_a_foreign_spinless_prefix_with_generators():
    """ls_amd_adopt_basis on a struct that is only the reference's prefix: the group, its characters and the sign tables are those
    of ls_hs_create_spinless_fermion_basis; a spinful prefix with generators keeps its error"""
    import ctypes as C

    L, N, gens, secs = 12, 5, dihedral(12), [6, 1]
    lib, own = create(L, N, gens, secs)
    fb = _lib.LsHsBasis(number_sites=L, number_particles=N, number_up=-1, particle_type=2, spin_inversion=0,
                        state_index_is_identity=False, requires_projection=True)
    bp = C.pointer(fb)
    perms = (C.c_int * (len(gens) * L))(*[v for p in gens for v in p])
    sectors = (C.c_int * len(gens))(*secs)
    try:
        assert lib.ls_amd_adopt_basis(bp, len(gens), perms, sectors) == 0, lib.ls_amd_last_error()
        assert lib.ls_amd_basis_fermion_signs(bp) == 1
        order = lib.ls_amd_basis_group_order(bp)
        assert order == lib.ls_amd_basis_group_order(own) == 24
        rs = np.random.RandomState(5)
        for g in range(order):
            cr, ci, pr, pi = C.c_double(), C.c_double(), C.c_double(), C.c_double()
            lib.ls_amd_basis_group_character(bp, g, C.byref(cr), C.byref(ci))
            lib.ls_amd_basis_group_character(own, g, C.byref(pr), C.byref(pi))
            assert (cr.value, ci.value) == (pr.value, pi.value)
            p = permutation_of(lib, bp, g, L)
            for a in rs.randint(0, 1 << L, size=16):
                assert lib.ls_amd_test_fermion_sign(bp, g, int(a), 0) == lib.ls_amd_test_fermion_sign(own, g, int(a), 0) == sign(p, int(a))
        lib.ls_amd_release(C.cast(bp, C.c_void_p))
        spinful = _lib.LsHsBasis(number_sites=4, number_particles=2, number_up=-1, particle_type=1, spin_inversion=0,
                                 state_index_is_identity=False, requires_projection=True)
        p4 = (C.c_int * 4)(1, 2, 3, 0)
        s4 = (C.c_int * 1)(0)
        assert lib.ls_amd_adopt_basis(C.pointer(spinful), 1, p4, s4) != 0
        assert "fermionic bases with symmetries are not supported" in lib.ls_amd_last_error().decode()
    finally:
        lib.ls_hs_destroy_basis(own)
