"""Projected spinful-fermion bases without a device: the lifted group of ls_hs_create_spinful_fermion_basis against the independent
reference (tests/fermion_spinful_symm.py), the host mirror of the device sign code (closed forms of the lifted ring elements against
the sign table, the table against inversion counting, past bit 32), how the elements were compiled, creation / clone / adoption,
every validation error, both YAML loaders, and the refusals that stay."""
import ctypes as C

import numpy as np
import pytest
import yaml

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib, config
from fermion_jw import hubbard_model, product_states, ring, yaml_terms
from fermion_spinful_symm import apply_v, group, lift, representatives, sign_v, state_info_v, swap
from fermion_symm import apply, dihedral, sign, state_info, torus, translations
from helpers import product_terms


def create(L, N, n_up, flip, gens, secs, expect_error=None):
    lib = _lib.load()
    ng = len(gens)
    flat = [v for p in gens for v in p]
    perms = (C.c_int * max(1, len(flat)))(*flat)
    sectors = (C.c_int * max(1, ng))(*secs)
    b = lib.ls_hs_create_spinful_fermion_basis(L, N, n_up, flip, ng, perms, sectors)
    if expect_error is not None:
        assert not b
        assert expect_error in lib.ls_amd_last_error().decode(), lib.ls_amd_last_error().decode()
        return lib, None
    assert b, lib.ls_amd_last_error().decode()
    return lib, b


def permutation_of(lib, b, g, M):
    """p with (g.a)[i] = a[p_i], read off single-mode states"""
    p = [0] * M
    for src in range(M):
        out = int(lib.ls_amd_basis_apply_group_element(b, g, 1 << src))
        p[out.bit_length() - 1] = src
    return p


def elements_of(lib, b, M):
    out = {}
    for g in range(lib.ls_amd_basis_group_order(b)):
        re, im = C.c_double(), C.c_double()
        assert lib.ls_amd_basis_group_character(b, g, C.byref(re), C.byref(im)) == 0
        out[tuple(permutation_of(lib, b, g, M))] = complex(re.value, im.value)
    return out


def assert_same_group(got, want):
    want = dict(want)
    assert set(got) == set(want)
    for p, ch in got.items():
        assert abs(ch - want[p]) < 1e-12, (p, ch, want[p])


def test_reference_array_forms_match_the_scalar_ones():
    rs = np.random.RandomState(0)
    L = 5
    grp = group(L, dihedral(L), [0, 1], flip=-1)
    states = rs.randint(0, 1 << (2 * L), size=64).astype(np.uint64)
    for p, _ in grp:
        assert [int(v) for v in apply_v(p, states)] == [apply(p, int(a)) for a in states]
        assert [int(v) for v in sign_v(p, states)] == [sign(p, int(a)) for a in states]
    best, ch0, norm = state_info_v(grp, states)
    for i, a in enumerate(states):
        r, c, n = state_info(grp, int(a))
        assert r == int(best[i]) and abs(n - norm[i]) < 1e-15 and (n == 0 or abs(c - ch0[i]) < 1e-12)


def test_reference_sectors_partition_the_product_space():
    L, nu, nd = 4, 2, 2
    total = 0
    for k in range(L):
        for f in (1, -1):
            total += len(representatives(L, nu, nd, group(L, translations(L), [k], flip=f))[0])
    assert total == len(product_states(L, nu, nd))
    assert sign(swap(3), 0b011_101) == 1 and sign(swap(3), 0b001_101) == 1 and sign(swap(3), 0b001_100) == -1  # (-1)^(N↑ N↓)
    assert lift([1, 2, 0], 3) == [1, 2, 0, 4, 5, 3]


SMALL_GROUPS = [(L, gens, flip) for L in (2, 3, 4, 5) for gens in (translations(L), dihedral(L)) for flip in (0, 1)] + \
               [(6, torus(3, 2), 0), (6, torus(3, 2), 1)]


@pytest.mark.parametrize("L,gens,flip", SMALL_GROUPS)
def test_host_signs_exhaustively_against_inversion_counting(L, gens, flip):
    """closed forms where the element is a lifted ring element == sign table == inversion counting, over every 2 L-bit word"""
    lib, b = create(L, 2, 1, flip, gens, [0] * len(gens))
    try:
        assert lib.ls_amd_basis_fermion_signs(b) == 1
        M = 2 * L
        for g in range(lib.ls_amd_basis_group_order(b)):
            p = permutation_of(lib, b, g, M)
            for a in range(1 << M):
                want = sign(p, a)
                assert lib.ls_amd_basis_apply_group_element(b, g, a) == apply(p, a)
                assert lib.ls_amd_test_fermion_sign(b, g, a, 0) == want, (g, p, bin(a))
                assert lib.ls_amd_test_fermion_sign(b, g, a, 1) == want, (g, p, bin(a))
    finally:
        lib.ls_hs_destroy_basis(b)


@pytest.mark.parametrize("L,gens", [(8, dihedral(8)), (16, dihedral(16)), (17, dihedral(17)), (24, dihedral(24)), (31, dihedral(31)),
                                    (32, dihedral(32)), (20, torus(4, 5)), (25, torus(5, 5))])
def test_host_signs_on_random_words_up_to_64_modes(L, gens):
    rs = np.random.RandomState(L)
    lib, b = create(L, 2, 1, -1, gens, [0] * len(gens))
    try:
        M = 2 * L
        order = lib.ls_amd_basis_group_order(b)
        mask = (1 << M) - 1
        states = [int(v) & mask for v in rs.randint(0, 2**63, size=20, dtype=np.uint64)]
        states = [s | (1 << (M - 1)) if i % 2 else s for i, s in enumerate(states)]  # the top mode, at or above bit 32 for L > 16
        states += [mask, ((1 << L) - 1) << L, (1 << (M - 1)) | 1, 1 << L]
        for g in range(0, order, max(1, order // 40)):
            p = permutation_of(lib, b, g, M)
            for a in states:
                want = sign(p, a)
                assert lib.ls_amd_basis_apply_group_element(b, g, a) == apply(p, a), (L, g, hex(a))
                assert lib.ls_amd_test_fermion_sign(b, g, a, 0) == want, (L, g, hex(a))
                assert lib.ls_amd_test_fermion_sign(b, g, a, 1) == want, (L, g, hex(a))
    finally:
        lib.ls_hs_destroy_basis(b)


def ring_form(p, L):
    """(is a lifted ring rotation / reflection, reversed, swapped) of a permutation of the 2 L modes, read off the permutation"""
    swapped = p[0] >= L
    s = [v - (L if swapped else 0) for v in p[:L]]
    if sorted(s) != list(range(L)) or p[L:] != [v + (0 if swapped else L) for v in s]:
        return False, False, swapped
    rot = all(s[i] == (s[0] + i) % L for i in range(L))
    rev = all(s[i] == (s[0] - i) % L for i in range(L))
    return rot or rev, rev and not rot, swapped


@pytest.mark.parametrize("L,gens,flip", [(7, translations(7), 0), (8, dihedral(8), 1), (17, dihedral(17), -1), (9, torus(3, 3), 1),
                                         (16, torus(4, 4), 0), (20, torus(4, 5), -1)])
def test_lifted_ring_elements_get_the_closed_form_kinds(L, gens, flip):
    lib, b = create(L, 2, 1, flip, gens, [0] * len(gens))
    try:
        kinds = []
        for g in range(lib.ls_amd_basis_group_order(b)):
            is_ring, rev, swapped = ring_form(permutation_of(lib, b, g, 2 * L), L)
            kind = lib.ls_amd_test_group_element_kind(b, g)
            kinds.append(kind)
            if is_ring:
                assert kind & 4 and bool(kind & 2) == swapped, (g, kind)
                if L > 2:  # (on two sites a reflection is a rotation)
                    assert bool(kind & 1) == rev, (g, kind)
            else:
                assert kind == 0, (g, kind)
        if len(gens) <= 2 and L not in (9, 16, 20):
            assert all(k >= 4 for k in kinds)  # a ring: no network left
        else:
            assert kinds.count(0) > len(kinds) // 2  # a torus: mostly networks
        assert lib.ls_amd_test_group_element_kind(b, len(kinds)) == -1
    finally:
        lib.ls_hs_destroy_basis(b)


def test_spin_and_spinless_elements_keep_their_kinds():
    lib = _lib.load()
    spin, _ = D.loadConfigFromDict(config.heisenberg_chain_config(8, symm=True), hamiltonian=True)
    assert {lib.ls_amd_test_group_element_kind(spin.payload, g) for g in range(spin.groupOrder())} <= {0, 1, 2}
    assert spin.spinFlip() == 0


CASES = [(6, 6, 3, 0, translations(6), [1]), (8, 8, 4, 1, dihedral(8), [0, 0]), (8, 8, 4, -1, dihedral(8), [4, 1]),
         (9, 4, 2, 0, torus(3, 3, point_group=False), [1, 2]), (6, 6, 3, -1, [], []), (17, 4, 2, 1, dihedral(17), [0, 1])]


@pytest.mark.parametrize("L,N,n_up,flip,gens,secs", CASES)
def test_creator_clone_and_adoption_build_the_reference_group(L, N, n_up, flip, gens, secs):
    want = group(L, gens, secs, flip)
    lib, own = create(L, N, n_up, flip, gens, secs)
    clone = lib.ls_hs_clone_basis(own)
    fb = _lib.LsHsBasis(number_sites=L, number_particles=N, number_up=n_up, particle_type=1, spin_inversion=0,
                        state_index_is_identity=False, requires_projection=True)
    bp = C.pointer(fb)
    flat = [v for p in gens for v in p]
    perms = (C.c_int * max(1, len(flat)))(*flat)
    sectors = (C.c_int * max(1, len(gens)))(*secs)
    try:
        assert clone, lib.ls_amd_last_error().decode()
        if flip:
            assert lib.ls_amd_adopt_spinful_fermion_basis(bp, flip, len(gens), perms, sectors) == 0, lib.ls_amd_last_error()
        else:
            assert lib.ls_amd_adopt_basis(bp, len(gens), perms, sectors) == 0, lib.ls_amd_last_error()
        for b in (own, clone, bp):
            c = b.contents
            assert (c.number_sites, c.number_particles, c.number_up, c.particle_type, c.spin_inversion) == (L, N, n_up, 1, 0)
            assert bool(c.requires_projection) and not bool(c.state_index_is_identity)
            assert lib.ls_amd_basis_spin_flip(b) == flip and lib.ls_amd_basis_fermion_signs(b) == 1
            assert lib.ls_amd_basis_group_order(b) == len(want)
            assert lib.ls_hs_basis_number_bits(b) == 2 * L
            assert_same_group(elements_of(lib, b, 2 * L), want)
        rs = np.random.RandomState(L)
        for g in range(len(want)):
            p = permutation_of(lib, own, g, 2 * L)
            assert p == permutation_of(lib, clone, g, 2 * L) == permutation_of(lib, bp, g, 2 * L)  # the same order of the elements
            for a in rs.randint(0, 1 << (2 * L), size=8, dtype=np.int64):
                assert lib.ls_amd_test_fermion_sign(clone, g, int(a), 0) == lib.ls_amd_test_fermion_sign(bp, g, int(a), 0) == sign(p, int(a))
        lib.ls_amd_release(C.cast(bp, C.c_void_p))
    finally:
        lib.ls_hs_destroy_basis(own)
        if clone:
            lib.ls_hs_destroy_basis(clone)


def test_without_generators_and_flip_the_basis_is_the_unprojected_one():
    lib, b = create(6, 6, 3, 0, [], [])
    try:
        assert not bool(b.contents.requires_projection) and lib.ls_amd_basis_fermion_signs(b) == 0 and lib.ls_amd_basis_group_order(b) == 1
    finally:
        lib.ls_hs_destroy_basis(b)


@pytest.mark.parametrize("args,why", [
    ((6, 5, 3, 1, translations(6), [0]), "spin_flip requires number_up == number_particles - number_up"),
    ((6, 6, 3, 2, translations(6), [0]), "spin_flip must be 0, 1 or -1"),
    ((6, 6, -1, 0, translations(6), [0]), "need a fixed number_up"),
    ((6, 6, -1, 1, [], []), "need a fixed number_up"),
    ((6, 6, 3, 0, [[1, 2, 3, 4, 5, 5]], [0]), "generator 0 is not a permutation"),
    ((6, 6, 3, 0, [[1, 2, 3, 4, 5, 6]], [0]), "generator 0 is not a permutation"),
    ((6, 6, 3, 0, dihedral(6), [1, 0]), "incompatible with the group structure"),
    ((6, 6, 7, 0, translations(6), [0]), "need 0 <= number_up <= number_sites"),
    ((33, 2, 1, 0, translations(33), [0]), "number_sites must be in [1, 32]"),
    ((0, 0, 0, 0, [], []), "number_sites must be in [1, 32]"),
])
def test_creator_validation_errors(args, why):
    create(*args, expect_error=why)


def test_the_flip_sector_must_be_compatible_with_the_group():
    # translation by one site at k = 1 on four sites is fine with either flip (the flip commutes with it and has order 2) ...
    for flip in (1, -1):
        lib, b = create(4, 4, 2, flip, translations(4), [1])
        assert lib.ls_amd_basis_group_order(b) == 8
        lib.ls_hs_destroy_basis(b)
    # ... a reflection in a momentum sector other than 0 and L / 2 is not, with or without it
    create(6, 6, 3, -1, dihedral(6), [1, 0], expect_error="incompatible with the group structure")


def test_adoption_errors():
    lib = _lib.load()
    p4, s4 = (C.c_int * 4)(1, 2, 3, 0), (C.c_int * 1)(0)
    # number_up unset: generators keep the message of the spinless pull request (pinned by tests/test_fermion_symm_host.py)
    fb = _lib.LsHsBasis(number_sites=4, number_particles=2, number_up=-1, particle_type=1, spin_inversion=0,
                        state_index_is_identity=False, requires_projection=True)
    assert lib.ls_amd_adopt_basis(C.pointer(fb), 1, p4, s4) != 0
    assert "fermionic bases with symmetries are not supported" in lib.ls_amd_last_error().decode()
    assert lib.ls_amd_adopt_spinful_fermion_basis(C.pointer(fb), 1, 0, p4, s4) != 0
    assert "fermionic bases with symmetries are not supported" in lib.ls_amd_last_error().decode()
    # a flip with N↑ != N↓, a spin prefix handed to the spinful entry, a prefix that claims no projection
    fb = _lib.LsHsBasis(number_sites=4, number_particles=3, number_up=2, particle_type=1, spin_inversion=0,
                        state_index_is_identity=False, requires_projection=True)
    assert lib.ls_amd_adopt_spinful_fermion_basis(C.pointer(fb), -1, 1, p4, s4) != 0
    assert "spin_flip requires" in lib.ls_amd_last_error().decode()
    spin = _lib.LsHsBasis(number_sites=4, number_particles=-1, number_up=2, particle_type=0, spin_inversion=0,
                          state_index_is_identity=False, requires_projection=True)
    assert lib.ls_amd_adopt_spinful_fermion_basis(C.pointer(spin), 1, 1, p4, s4) != 0
    assert "not a spinful-fermion basis" in lib.ls_amd_last_error().decode()
    fb = _lib.LsHsBasis(number_sites=4, number_particles=4, number_up=2, particle_type=1, spin_inversion=0,
                        state_index_is_identity=False, requires_projection=False)
    assert lib.ls_amd_adopt_basis(C.pointer(fb), 1, p4, s4) != 0
    assert "requires_projection differs" in lib.ls_amd_last_error().decode()


def spinful_symm_cfg(L, nu, nd, gens, secs, flip, model):
    basis = {"particle": "spinful-fermion", "number_sites": L, "number_particles": nu + nd, "number_up": nu,
             "symmetries": [{"permutation": p, "sector": s} for p, s in zip(gens, secs)]}
    if flip:
        basis["spin_flip"] = flip
    return {"basis": basis, "hamiltonian": {"terms": yaml_terms(model, True)}}


LOADER_CASES = {
    "ring_8_dihedral_flip": spinful_symm_cfg(8, 4, 4, dihedral(8), [4, 1], -1, hubbard_model(8, ring(8), U=3.0)),
    "ring_7_k2_phase": spinful_symm_cfg(7, 3, 2, translations(7), [2], 0, hubbard_model(7, ring(7), phase=0.2)),
    "torus_4x4_flip": spinful_symm_cfg(16, 2, 2, torus(4, 4), [0, 0, 0, 0], 1, hubbard_model(16, ring(16))),
    "flip_only": spinful_symm_cfg(6, 3, 3, [], [], 1, hubbard_model(6, ring(6))),
    "ring_32": spinful_symm_cfg(32, 1, 1, translations(32), [5], 0, hubbard_model(32, ring(32))),
}


@pytest.mark.parametrize("name", sorted(LOADER_CASES))
def test_c_and_python_loaders_agree_on_spinful_symmetries(name):
    cfg = LOADER_CASES[name]
    bs = cfg["basis"]
    L = bs["number_sites"]
    lib = _lib.load()
    conf = lib.ls_amd_load_yaml_config_from_string(yaml.safe_dump(cfg, allow_unicode=True).encode("utf-8"))
    assert conf, lib.ls_amd_last_error().decode()
    try:
        c = conf.contents
        spec = config.parse_basis(cfg)
        assert spec.permutations == [s["permutation"] for s in bs["symmetries"]] and spec.spin_flip == bs.get("spin_flip", 0)
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        b = c.basis.contents
        assert (b.number_sites, b.number_particles, b.number_up, b.particle_type, b.spin_inversion) == \
            (basis.numberSites(), basis.numberParticles(), basis.numberUp(), basis.particleType(), 0)
        assert bool(b.requires_projection) and basis.requiresProjection() and basis.hasFermionSigns()
        assert basis.spinFlip() == lib.ls_amd_basis_spin_flip(c.basis) == bs.get("spin_flip", 0)
        want = group(L, [s["permutation"] for s in bs["symmetries"]], [s["sector"] for s in bs["symmetries"]], bs.get("spin_flip", 0))
        assert basis.groupOrder() == lib.ls_amd_basis_group_order(c.basis) == len(want)
        assert_same_group(elements_of(lib, c.basis, 2 * L), want)
        assert_same_group(elements_of(lib, basis.payload, 2 * L), want)
        assert product_terms(D.Operator(c.hamiltonian, owning=False)) == product_terms(h)
    finally:
        lib.ls_hs_destroy_yaml_config(conf)


def both_loaders_refuse(basis, why):
    cfg = {"basis": basis, "hamiltonian": {"terms": [{"expression": "n₀↑", "sites": [[0]]}]}}
    lib = _lib.load()
    assert not lib.ls_amd_load_yaml_config_from_string(yaml.safe_dump(cfg, allow_unicode=True).encode("utf-8"))
    c_error = lib.ls_amd_last_error().decode()
    assert why in c_error, c_error
    with pytest.raises((ValueError, D.LsAmdError)) as ei:
        D.loadConfigFromDict(cfg, hamiltonian=True)
    assert why in str(ei.value), str(ei.value)
    return c_error, str(ei.value)


T4 = [{"permutation": [1, 2, 3, 0], "sector": 0}]


@pytest.mark.parametrize("basis,why", [
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 3, "number_up": 2, "spin_flip": 1},
     "spin_flip requires number_up == number_particles - number_up"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2, "spin_flip": 2}, "spin_flip must be 1 or -1"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "spin_flip": 1},
     "spin_flip is a key of spinful-fermion bases with number_up, not of particle 'spinful-fermion' without number_up"),
    ({"particle": "spinless-fermion", "number_sites": 4, "number_particles": 2, "spin_flip": 1},
     "spin_flip is a key of spinful-fermion bases with number_up, not of particle 'spinless-fermion'"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2, "symmetries": [{"permutation": [1, 2, 0], "sector": 0}]},
     "basis.symmetries[0]: expected {permutation: [4 sites], sector: int}"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2,
      "symmetries": [{"permutation": [1, 1, 2, 3], "sector": 0}]}, "generator 0 is not a permutation"),
    ({"particle": "spinful-fermion", "number_sites": 6, "number_particles": 6, "number_up": 3,
      "symmetries": [{"permutation": p, "sector": s} for p, s in zip(dihedral(6), [1, 0])]}, "incompatible with the group structure"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "symmetries": T4},
     "symmetries is not supported for particle 'spinful-fermion' without number_up"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2, "symmetries": T4, "spin_inversion": 1},
     "spin_inversion is not supported for particle 'spinful-fermion'"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2, "symmetries": T4, "hamming_weight": 2},
     "hamming_weight is not supported for particle 'spinful-fermion'"),
])
def test_both_loaders_refuse_alike(basis, why):
    both_loaders_refuse(basis, why)


def test_pinned_refusals_stay():
    """what the tests of the spinless pull request pin: number_up unset + symmetries, spin_inversion, adoption with number_up == -1"""
    cfg = {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 2, "symmetries": T4}}
    with pytest.raises(ValueError, match="symmetries"):
        config.parse_basis(cfg)
    both_loaders_refuse(cfg["basis"], "symmetries")
    with pytest.raises(ValueError, match="spin_inversion"):
        config.parse_basis({"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "spin_inversion": 1}})
    both_loaders_refuse({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "spin_inversion": 1}, "spin_inversion")


def test_hubbard_config_passes_symmetries_and_flip_through():
    plain = config.hubbard_config(6, ring(6))
    assert "symmetries" not in plain["basis"] and "spin_flip" not in plain["basis"]
    syms = [{"permutation": p, "sector": s} for p, s in zip(dihedral(6), [3, 1])]
    cfg = config.hubbard_config(6, ring(6), U=2.0, symmetries=syms, spin_flip=-1)
    assert cfg["hamiltonian"] == config.hubbard_config(6, ring(6), U=2.0)["hamiltonian"]
    basis, _ = D.loadConfigFromDict(cfg, hamiltonian=True)
    assert basis.spinFlip() == -1 and basis.groupOrder() == 24 and basis.hasFermionSigns()
    unprojected, _ = D.loadConfigFromDict(plain, hamiltonian=True)
    assert unprojected.spinFlip() == 0 and not unprojected.requiresProjection() and not unprojected.hasFermionSigns()


def test_sector_sizes_of_the_reference_cases():
    """the representative counts the GPU tests rely on (ring 6, ring 7, ring 8 dihedral with flip, 3 x 3 torus)"""
    assert len(representatives(6, 3, 3, group(6, translations(6), [1]))[0]) == 66
    assert len(representatives(7, 3, 2, group(7, translations(7), [2]))[0]) == 105
    assert len(representatives(8, 4, 4, group(8, dihedral(8), [0, 0], 1))[0]) == 181
    assert len(representatives(8, 4, 4, group(8, dihedral(8), [4, 1], -1))[0]) == 145
    assert len(representatives(9, 2, 2, group(9, torus(3, 3, point_group=False), [1, 2]))[0]) == 144
    assert len(product_states(6, 3, 3)) == 400
