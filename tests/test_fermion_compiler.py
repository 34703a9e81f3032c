"""Fermionic bases on the host side: the expression compiler's terms (config.py), applied by a tiny evaluator to the basis
states, equal an independent Jordan-Wigner Kronecker construction; the basis constructor's fields and queries."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import config
from fermion_jw import (apply_terms, dense, hubbard_model, product_states, restrict, ring, weight_states, yaml_terms)


def compiled(model, L, spinful):
    spec = config.BasisSpec(number_sites=L, particle="spinful-fermion" if spinful else "spinless-fermion")
    return config.parse_operator({"terms": yaml_terms(model, spinful)}, spec).terms


SPINLESS = {
    "hop_forward": [(-1.0, [("+", 0, 0), ("-", 3, 0)])],
    "hop_backward": [(-1.0, [("+", 5, 0), ("-", 1, 0)])],
    "hop_wrap": [(-0.7, [("+", 7, 0), ("-", 0, 0)]), (-0.7, [("+", 0, 0), ("-", 7, 0)])],
    "density": [(0.3, [("n", 2, 0)]), (1.1, [("n", 1, 0), ("n", 6, 0)])],
    "complex_hop": [(0.4 + 0.9j, [("+", 1, 0), ("-", 4, 0)]), (0.4 - 0.9j, [("+", 4, 0), ("-", 1, 0)])],
    "repeated_mode": [(1.0, [("+", 2, 0), ("-", 2, 0), ("+", 2, 0)]), (2.0, [("n", 3, 0), ("n", 3, 0)])],
    "pair_creation": [(0.5, [("+", 1, 0), ("+", 6, 0)]), (0.5, [("-", 6, 0), ("-", 1, 0)])],
    "ring_8": [(-1.0, [("+", i, 0), ("-", (i + 1) % 8, 0)]) for i in range(8)]
              + [(-1.0, [("+", (i + 1) % 8, 0), ("-", i, 0)]) for i in range(8)],
}


@pytest.mark.parametrize("name", sorted(SPINLESS))
@pytest.mark.parametrize("N", [-1, 3])
def test_spinless_terms_equal_jordan_wigner(name, N):
    L = 8
    model = SPINLESS[name]
    H = dense(model, L, False).toarray()
    states = weight_states(L, N)
    want = restrict(H, states) if N >= 0 else H
    got = apply_terms(compiled(model, L, False), states)
    assert np.abs(got - want).max() < 1e-12, name


SPINFUL = {
    "hubbard_ring_3": hubbard_model(3, ring(3), t=1.0, U=2.5),
    "hubbard_open_4_complex": hubbard_model(4, [(0, 1), (1, 2), (2, 3)], t=0.8, U=1.0, phase=0.3),
    "extended_hubbard_ring_4": hubbard_model(4, ring(4), t=1.0, U=3.0, V=0.7),
    "hop_wrap_down": [(-1.0, [("+", 3, 1), ("-", 0, 1)]), (-1.0, [("+", 0, 1), ("-", 3, 1)])],
    "pair_hopping": [(0.6, [("+", 0, 0), ("+", 0, 1), ("-", 2, 1), ("-", 2, 0)]),
                     (0.6, [("+", 2, 0), ("+", 2, 1), ("-", 0, 1), ("-", 0, 0)])],
    "spin_flip": [(0.9, [("+", 1, 0), ("-", 1, 1), ("+", 3, 1), ("-", 3, 0)]),
                  (0.9, [("+", 3, 0), ("-", 3, 1), ("+", 1, 1), ("-", 1, 0)])],
    "nn_same_site": [(1.5, [("n", 2, 0), ("n", 2, 1)]), (-0.4, [("n", 1, 1)])],
    "repeated_mode": [(1.0, [("n", 0, 0), ("+", 1, 0), ("-", 0, 0), ("n", 0, 0)])],
}


@pytest.mark.parametrize("name", sorted(SPINFUL))
def test_spinful_terms_equal_jordan_wigner(name):
    L = 4 if name != "hubbard_ring_3" else 3
    model = SPINFUL[name]
    H = dense(model, L, True).toarray()
    terms = compiled(model, L, True)
    for nu, nd in ((1, 1), (2, 1), (1, 3), (0, 2), (L, 1)):
        states = product_states(L, nu, nd)
        got = apply_terms(terms, states)
        want = restrict(H, states)
        assert np.abs(got - want).max() < 1e-12, (name, nu, nd)
    full = np.arange(2 ** (2 * L), dtype=np.uint64)
    assert np.abs(apply_terms(terms, full) - H).max() < 1e-12, name


def test_hop_sign_mask_is_the_modes_between():
    (v, m, r, x, s), = config.fermion_monomial_terms("c†₀ c₁", [1, 5], False, 8)
    assert (m, r, x, s) == (0b100010, 0b100000, 0b100010, 0b011100) and v == 1
    (v, m, r, x, s), = config.fermion_monomial_terms("c†₀↓ c₁↑", [0, 2], True, 4)  # mode (0, down) = bit 4, (2, up) = bit 2
    assert (m, r, x, s) == (0b10100, 0b00100, 0b10100, 0b01000)


def test_hubbard_config_matches_model():
    cfg = config.hubbard_config(4, ring(4), t=1.0, U=3.0, V=0.5)
    spec = config.parse_basis(cfg)
    assert (spec.particle, spec.number_sites, spec.number_particles, spec.number_up) == ("spinful-fermion", 4, 4, 2)
    terms = config.parse_operator(cfg["hamiltonian"], spec).terms
    states = product_states(4, 2, 2)
    want = restrict(dense(hubbard_model(4, ring(4), t=1.0, U=3.0, V=0.5), 4, True).toarray(), states)
    assert np.abs(apply_terms(terms, states) - want).max() < 1e-12


@pytest.mark.parametrize("basis,why", [
    ({"particle": "spinless-fermion", "number_spins": 4}, "spin-1/2"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_up": 2}, "number_particles"),
    ({"particle": "spinless-fermion", "number_sites": 4, "number_up": 2}, "number_up"),
    ({"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "symmetries": [{"permutation": [1, 2, 3, 0], "sector": 0}]}, "symmetries"),
    ({"particle": "quark", "number_sites": 4}, "unknown particle"),
])
def test_basis_schema_errors(basis, why):
    with pytest.raises(ValueError, match=why):
        config.parse_basis({"basis": basis})


def test_expression_errors():
    with pytest.raises(ValueError, match="spin index"):
        config.parse_fermion_expression("c†₀ c₁", True)
    with pytest.raises(ValueError, match="no spin index"):
        config.parse_fermion_expression("c†₀↑ c₁↑", False)
    with pytest.raises(ValueError, match="spin operator"):
        config.parse_fermion_expression("σᶻ₀ c₁", False)


def _basis(particle, L, N, Nup):
    return D.Basis.fromSpec(config.BasisSpec(number_sites=L, particle=particle, number_particles=N, number_up=Nup))


def test_spinful_product_basis_fields_and_queries():
    b = _basis("spinful-fermion", 5, 5, 3)
    assert (b.numberSites(), b.numberParticles(), b.numberUp(), b.particleType()) == (5, 5, 3, 1)
    assert b.numberBits() == 10 and b.numberWords() == 1
    assert not b.isHammingWeightFixed()  # the (N, N_up) product basis: the reference's spinful branch
    assert not b.isStateIndexIdentity() and not b.requiresProjection()
    assert not b.hasPermutationSymmetries() and not b.hasSpinInversionSymmetry()
    states = product_states(5, 3, 2)
    assert b.minStateEstimate() == int(states[0]) and b.maxStateEstimate() == int(states[-1])


def test_spinful_fixed_n_and_spinless_bases():
    b = _basis("spinful-fermion", 4, 3, -1)
    assert b.numberBits() == 8 and b.isHammingWeightFixed() and b.numberUp() == -1
    assert b.minStateEstimate() == 0b111 and b.maxStateEstimate() == 0b11100000
    s = _basis("spinless-fermion", 6, 2, -1)
    assert (s.numberBits(), s.particleType(), s.numberParticles()) == (6, 2, 2) and s.isHammingWeightFixed()
    u = _basis("spinless-fermion", 6, -1, -1)
    assert u.isStateIndexIdentity() and not u.isHammingWeightFixed()


@pytest.mark.parametrize("particle,L,N,Nup,why", [
    ("spinful-fermion", 33, 2, 1, "number_sites"),
    ("spinful-fermion", 4, 3, 4, "number_up"),
    ("spinful-fermion", 4, -1, 1, "number_particles"),
    ("spinless-fermion", 4, 5, -1, "number_particles"),
    ("spinless-fermion", 4, 2, 1, "number_up"),
])
def test_create_basis_errors(particle, L, N, Nup, why):
    with pytest.raises(D.LsAmdError, match=why):
        _basis(particle, L, N, Nup)


def test_clone_keeps_the_fermionic_kind():
    from distributed_matvec_amd import _lib

    L = _lib.load()
    b = _basis("spinful-fermion", 4, 4, 1)
    c = L.ls_hs_clone_basis(b.payload)
    try:
        assert (c.contents.number_sites, c.contents.number_particles, c.contents.number_up, c.contents.particle_type) == (4, 4, 1, 1)
        assert L.ls_hs_basis_number_bits(c) == 8 and not L.ls_hs_basis_has_fixed_hamming_weight(c)
    finally:
        L.ls_hs_destroy_basis(c)


def test_operator_terms_reach_the_high_half():
    b, h = D.loadConfigFromDict(config.hubbard_config(4, ring(4), U=2.0), hamiltonian=True)
    assert h.numberOffDiagTerms() > 0 and h.isHermitian and h.isReal
