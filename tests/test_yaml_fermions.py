"""The C YAML loader (ls_hs_load_yaml_config, csrc/yaml.c) on fermionic files: the same basis and the same term tables as the
Python mirror (config.py), and its fermionic error cases."""
import pytest
import yaml

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib, config
from fermion_jw import hubbard_model, ring, square, yaml_terms
from fermion_wide import hop, pair_hop, spinless_chain
from helpers import product_terms


def load_c(text):
    L = _lib.load()
    conf = L.ls_amd_load_yaml_config_from_string(text.encode("utf-8"))
    if not conf:
        raise D.LsAmdError(L.ls_amd_last_error().decode())
    return conf


def spinless_model(L):
    model = []
    for i, j in ring(L):
        model += [(-1.0, [("+", i, 0), ("-", j, 0)]), (-1.0, [("+", j, 0), ("-", i, 0)]), (0.7, [("n", i, 0), ("n", j, 0)])]
    model += [(0.3 + 0.4j, [("+", 0, 0), ("-", 3, 0)]), (0.3 - 0.4j, [("+", 3, 0), ("-", 0, 0)]), (0.5, [("n", 2, 0), ("+", 2, 0), ("-", 2, 0)])]
    return model


def spinful_extra(L):
    return [(0.6, [("+", 0, 0), ("+", 0, 1), ("-", 2, 1), ("-", 2, 0)]), (0.6, [("+", 2, 0), ("+", 2, 1), ("-", 0, 1), ("-", 0, 0)]),
            (0.9, [("+", 1, 0), ("-", 1, 1), ("+", 3, 1), ("-", 3, 0)]), (0.9, [("+", 3, 0), ("-", 3, 1), ("+", 1, 1), ("-", 1, 0)])]


CASES = {
    "hubbard_ring_6": config.hubbard_config(6, ring(6), t=1.0, U=4.0),
    "hubbard_2x3_peierls_V": config.hubbard_config(6, square(3, 2), t=0.8, U=2.0, V=0.5, peierls=0.3),
    "spinful_fixed_n": {"basis": {"particle": "spinful-fermion", "number_sites": 5, "number_particles": 4, "number_up": None},
                        "hamiltonian": {"terms": yaml_terms(hubbard_model(5, ring(5), U=1.0) + spinful_extra(5), True)}},
    "spinful_unrestricted": {"basis": {"particle": "spinful-fermion", "number_sites": 4},
                             "hamiltonian": {"terms": yaml_terms(spinful_extra(4), True)}},
    "spinless_ring_8": {"basis": {"particle": "spinless-fermion", "number_sites": 8, "number_particles": 3},
                        "hamiltonian": {"terms": yaml_terms(spinless_model(8), False)}},
    "spinless_unrestricted": {"basis": {"particle": "spinless-fermion", "number_sites": 7, "number_particles": None},
                              "hamiltonian": {"terms": yaml_terms(spinless_model(7), False)}},
    # wide words: the down half at bits 32..63 (a pair hop onto 31 down reaches bit 63), strings across bit 32 and up to bit 62
    "hubbard_32_peierls_pair_hop": {
        "basis": {"particle": "spinful-fermion", "number_sites": 32, "number_particles": 3, "number_up": 1},
        "hamiltonian": {"terms": yaml_terms(hubbard_model(32, ring(32) + [(0, 17), (5, 29)], t=1.0, U=2.0, V=0.3, phase=0.21)
                                            + pair_hop(0, 31, 0.5), True)}},
    "spinless_ring_64_long_hops": {
        "basis": {"particle": "spinless-fermion", "number_sites": 64, "number_particles": 2},
        "hamiltonian": {"terms": yaml_terms(spinless_chain(64, ring(64) + [(3, 60), (30, 33)], V=0.5)
                                            + hop(1, 62, 0.2 + 0.3j), False)}},
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("flow", [False, True])
def test_c_loader_equals_python_mirror_on_fermionic_files(name, flow):
    cfg = CASES[name]
    text = yaml.safe_dump(cfg, allow_unicode=True, default_flow_style=None if flow else False)
    L = _lib.load()
    conf = load_c(text)
    try:
        c = conf.contents
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        b = c.basis.contents
        assert (b.number_sites, b.number_particles, b.number_up, b.particle_type) == \
            (basis.numberSites(), basis.numberParticles(), basis.numberUp(), basis.particleType())
        assert L.ls_hs_basis_number_bits(c.basis) == basis.numberBits()
        assert bool(L.ls_hs_basis_has_fixed_hamming_weight(c.basis)) == basis.isHammingWeightFixed()
        assert int(L.ls_hs_min_state_estimate(c.basis)) == basis.minStateEstimate()
        assert int(L.ls_hs_max_state_estimate(c.basis)) == basis.maxStateEstimate()
        op_c = D.Operator(c.hamiltonian, owning=False)
        assert product_terms(op_c) == product_terms(h)
        assert op_c.isHermitian == h.isHermitian and op_c.isReal == h.isReal
        assert any(s != 0 for _, _, _, _, s in product_terms(h)[1])  # the Jordan-Wigner strings made it into the tables
    finally:
        L.ls_hs_destroy_yaml_config(conf)


def test_raw_terms_equal_the_python_compiler():
    """Before any merging: one monomial per file, so the table is exactly the compiled terms (sorted)"""
    for expr, sites, spinful in (("-1 × c†₀↑ c₁↑", [[0, 3]], True), ("0.5 × c†₀↓ c₁↑", [[3, 1]], True), ("2 × n₀↑ n₀↓", [[2]], True),
                                 ("c†₀ c₁", [[6, 1]], False), ("c†₀ c†₁ c₂ c₃", [[0, 5, 2, 7]], False), ("c₀ n₀ c†₀", [[4]], False)):
        basis = {"particle": "spinful-fermion" if spinful else "spinless-fermion", "number_sites": 8}
        cfg = {"basis": basis, "hamiltonian": {"terms": [{"expression": expr, "sites": sites}]}}
        spec = config.parse_basis(cfg)
        want = config.fermion_monomial_terms(expr, sites[0], spinful, 8)
        conf = load_c(yaml.safe_dump(cfg, allow_unicode=True))
        try:
            got = product_terms(D.Operator(conf.contents.hamiltonian, owning=False))
        finally:
            _lib.load().ls_hs_destroy_yaml_config(conf)
        _, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        assert got == product_terms(h), expr
        assert sum(len(t) for t in got) == len([t for t in want if t[0] != 0]), expr
        assert spec.particle == basis["particle"]


@pytest.mark.parametrize("text,why", [
    ("basis:\n  number_spins: 4\n  particle: spinless-fermion\n", "spin-1/2"),
    ("basis:\n  particle: quark\n  number_sites: 4\n", "unknown particle"),
    ("basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_up: 2\n", "number_particles"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\n  number_particles: 2\n  number_up: 1\n", "number_up"),
    ("basis:\n  particle: spinless-fermion\n  number_particles: 2\n", "needs number_sites"),
    ("basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_particles: 4\n  symmetries:\n    - permutation: [1, 2, 3, 0]\n      sector: 0\n",
     "symmetries"),
    ("basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_particles: 4\n  spin_inversion: 1\n", "spin_inversion"),
    ("basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_particles: 9\n", "number_particles"),
    ("basis:\n  particle: spinful-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"c†₀ c₁\"\n      sites: [[0, 1]]\n",
     "spin index"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"c†₀↑ c₁↑\"\n      sites: [[0, 1]]\n",
     "no spin index"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"σᶻ₀ c₁\"\n      sites: [[0, 1]]\n",
     "spin operator"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"c†₀ c₁\"\n      sites: [[0, 4]]\n",
     "out of range"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"c†₀ c₁\"\n      sites: [[0]]\n",
     "needs 2 sites"),
    ("basis:\n  particle: spinless-fermion\n  number_sites: 4\nhamiltonian:\n  terms:\n    - expression: \"c†x₀\"\n      sites: [[0]]\n",
     "site index"),
])
def test_c_loader_fermionic_errors(text, why):
    with pytest.raises(D.LsAmdError, match=why):
        load_c(text)


def test_python_mirror_rejects_what_the_c_loader_rejects():
    for text in ("basis:\n  number_spins: 4\n  particle: spinless-fermion\n",
                 "basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_up: 2\n",
                 "basis:\n  particle: spinful-fermion\n  number_sites: 4\n  number_particles: 4\n  spin_inversion: 1\n"):
        with pytest.raises(ValueError):
            config.parse_basis(yaml.safe_load(text))
