"""Two-point correlation matrices on the GPU (CorrelationPlan / k_corr_diag, k_corr_hop, k_corr_hop_fermi; spin_correlations,
fermion_correlations) against the CPU expansions the tests own -- tests/entanglement_reference.expand_full for spins, the projector
columns of tests/fermion_entanglement_reference for fermions -- followed by plain numpy bit arithmetic over all product states, every
one of the M^2 entries; identities at a size no dense reference reaches (the energy as a bond sum, the singlet sum rule, Tr one_body =
N, the idempotent one-body matrix of free fermions); <sigma^+_i sigma^-_j> and <c+_i c_j> through an Operator matvec + dot, which
fixes the bit and sign conventions; bitwise reproducibility; and the failures that must be loud.

Tolerance (derived, not tuned): every entry is a sum of at most n M products whose moduli sum to at most 1 for a normalised state
(Cauchy-Schwarz); each summand carries a handful of roundings, so with n <= 13 000 the worst case of recursive summation is about
n 8 2^-53 ~ 1e-11.  ATOL = 2e-11; a wrong sign, character or convention shows at 1e-2 or more."""
import ctypes as C

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_jw as JW
import fermion_symm as F
from distributed_matvec_amd import CorrelationPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd._lib import LsAmdError
from distributed_matvec_amd.config import parse_expression
from helpers import model_config

pytestmark = pytest.mark.gpu
ATOL = 2e-11
ONE = np.uint64(1)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def reference(states, vec, M, jw, species=None):
    """(d, D, G) of the full vector `vec` over the ascending product states `states`, by bit arithmetic: d[i] = <b_i>, D[i][j] =
    <b_i b_j>, G[i][j] = <B+_i B_j> = sum_s conj(vec[B+_i B_j s]) vec[s] over the s with bit j set and bit i clear, times
    (-1)^(set bits of s strictly between i and j) when jw.  species = L: pairs across the two halves are skipped (they leave the
    (N_up, N_down) basis: exactly zero)."""
    states = np.asarray(states, dtype=np.uint64)
    bits = np.stack([((states >> np.uint64(i)) & ONE).astype(np.float64) for i in range(M)], axis=1)
    w = np.abs(vec) ** 2
    d = w @ bits
    Dm = bits.T @ (w[:, None] * bits)
    G = np.zeros((M, M), dtype=np.complex128)
    for i in range(M):
        for j in range(M):
            if i == j:
                G[i, i] = d[i]
                continue
            if species is not None and (i < species) != (j < species):
                continue
            sel = (bits[:, j] == 1) & (bits[:, i] == 0)
            s = states[sel]
            t = s ^ (ONE << np.uint64(i)) ^ (ONE << np.uint64(j))
            pos = np.searchsorted(states, t)
            assert np.array_equal(states[pos], t)
            val = np.conj(vec[pos]) * vec[sel]
            if jw:
                lo, hi = min(i, j), max(i, j)
                between = np.uint64(((1 << hi) - 1) & ~((2 << lo) - 1))
                val = np.where(np.bitwise_count(s & between) & 1, -val, val)
            G[i, j] = val.sum()
    return d, Dm, G


def _random_state(torch, reps, dtype, seed=11):
    psi = D.fillRandom(reps, seed, dtype)
    return psi / torch.linalg.vector_norm(psi)


def _compare(name, got, want):
    worst = 0.0
    for label, g, w in zip(("d", "D", "G"), got, want):
        assert g.shape == w.shape and np.isfinite(g).all(), (name, label)
        err = float(np.abs(g - w).max())  # every entry, none left out
        worst = max(worst, err)
        print(f"correlations {name}: {label}{tuple(g.shape)} max error {err:.2e} (atol {ATOL:.0e})")
    assert worst <= ATOL, (name, worst)


# ---- spins -----------------------------------------------------------------------------------------------------------------------
SPIN_CASES = {
    # name: (basis config, dtype of psi, representatives): more than one 256-row tile with a ragged last one, but for the two small
    # sectors (one ragged tile)
    "ring16_unprojected_f64": (lambda: E.ring(16, 8, None), "f64", 12870),
    "ring16_k0_f64": (lambda: E.ring(16, 8, 0), "f64", 810),
    "ring16_k3_c128": (lambda: E.ring(16, 8, 3), "c128", 800),
    "ring16_k8_reflection_inversion_characters_minus": (lambda: E.ring(16, 8, 8, inv=-1, reflect=1), "f64", 230),
    "ring16_k0_reflection_inversion_plus_c128": (lambda: E.ring(16, 8, 0, inv=1, reflect=0), "c128", 257),
    "ring34_weight3_k5_64bit_words": (lambda: E.ring(34, 3, 5), "c128", 176),
    # the density kernel owns 3, 5 or 9 pairs per thread on 64-bit words: 34, 44 and 64 sites (595, 990, 2080 pairs); bit 63 in use
    "ring44_weight2_k1_five_pairs_per_thread": (lambda: E.ring(44, 2, 1), "c128", 21),
    # (unprojected: the static index table of a projected basis takes keys of up to bucket bits + 24 bits, as for its matvec plans)
    "ring64_weight2_unprojected_nine_pairs_per_thread": (lambda: E.ring(64, 2, None), "f64", 2016),
}


def _spin_setup(cfg):
    basis = D.loadConfigFromDict({"basis": cfg["basis"]})
    reps, _ = D.enumerateStates(basis, 1)
    return basis, reps[0]


@pytest.mark.parametrize("name", sorted(SPIN_CASES))
def test_spin_matrices_match_the_expansion(torch, name):
    make, dt, count = SPIN_CASES[name]
    cfg = make()
    model, full, want_reps, _idx, _coef, live = E.tables(cfg)
    basis, reps = _spin_setup(cfg)
    assert np.array_equal(_u64(reps), want_reps)
    n = len(want_reps)
    assert n == count and n % 256 != 0
    if name == "ring34_weight3_k5_64bit_words":
        assert len(full) == 5984 and int(full.max()) >> 32
    if name == "ring64_weight2_unprojected_nine_pairs_per_thread":
        assert int(full.max()) >> 63
    if name in ("ring16_k3_c128", "ring16_k8_reflection_inversion_characters_minus", "ring44_weight2_k1_five_pairs_per_thread"):
        assert (~live).any()  # zero-norm orbits
    psi = _random_state(torch, reps, torch.complex128 if dt == "c128" else torch.float64)
    vec = E.expand_full(cfg, psi.cpu().numpy())
    assert abs(np.vdot(vec, vec).real - 1.0) < 1e-12
    M = model.number_sites
    want = reference(full, vec, M, jw=False)
    pl = D.CorrelationPlan(basis, reps)
    assert pl.modes == M and pl.kernel("densities") == "k_corr_diag" and pl.kernel("hoppings") == "k_corr_hop" and pl.kernel(1) == "k_corr_hop"
    d, Dm = pl.densities(psi)
    G = pl.hoppings(psi)
    _compare(name, (d, Dm, G), want)
    assert np.array_equal(np.diag(Dm), d) or np.abs(np.diag(Dm) - d).max() <= ATOL
    # the derived quantities, against the same bit arithmetic
    sc = D.spin_correlations(basis, reps, 3.0 * psi)  # (normalised inside)
    z = 1.0 - 2.0 * want[0]
    zz = 1.0 - 2.0 * want[0][:, None] - 2.0 * want[0][None, :] + 4.0 * want[1]
    pm = want[2].T.copy()
    np.fill_diagonal(pm, 1.0 - want[0])
    ss = 0.25 * zz + 0.5 * (pm + pm.T)
    np.fill_diagonal(ss, 0.75)
    for g, w in zip(sc, (z, zz, pm, ss)):
        assert np.abs(g - w).max() <= 4 * ATOL  # (zz = 1 - 2 d - 2 d + 4 D: four times the error of an entry)
    pl.destroy()


# ---- fermions --------------------------------------------------------------------------------------------------------------------
FERMI_CASES = {
    "spinless16_k0_f64": (lambda: R.Case(16, 8, gens=F.translations(16), secs=[0]), "f64", "k_corr_hop_fermi"),
    "spinless16_k3_c128": (lambda: R.Case(16, 8, gens=F.translations(16), secs=[3]), "c128", "k_corr_hop_fermi"),
    "spinless16_dihedral_reflection_odd": (lambda: R.Case(16, 8, gens=F.dihedral(16), secs=[0, 1]), "f64", "k_corr_hop_fermi"),
    "spinless16_unprojected": (lambda: R.Case(16, 8), "c128", "k_corr_hop"),
    "spinful8_k0": (lambda: R.Case(8, up=(4, 4), gens=F.translations(8), secs=[0]), "f64", "k_corr_hop_fermi"),
    "spinful8_k0_flip_plus": (lambda: R.Case(8, up=(4, 4), gens=F.translations(8), secs=[0], flip=1), "f64", "k_corr_hop_fermi"),
    "spinful8_k1_flip_minus": (lambda: R.Case(8, up=(4, 4), gens=F.translations(8), secs=[1], flip=-1), "c128", "k_corr_hop_fermi"),
    "spinful8_unprojected_product": (lambda: R.Case(8, up=(4, 4)), "f64", "k_corr_hop"),
    "spinless64_two_particles_unprojected": (lambda: R.Case(64, 2), "c128", "k_corr_hop"),  # Jordan-Wigner masks up to mode 63
}


def _fermi_setup(case, model=None):
    cfg = case.config(model)
    if model is None:
        basis, h = D.loadConfigFromDict(cfg), None
    else:
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    return basis, h, reps


@pytest.mark.parametrize("name", sorted(FERMI_CASES))
def test_fermion_matrices_match_the_expansion(torch, name):
    make, dt, kernel = FERMI_CASES[name]
    case = make()
    basis, _, reps = _fermi_setup(case)
    assert np.array_equal(_u64(reps[0]), case.reps)
    n = len(case.reps)
    assert n > 256 and n % 256 != 0
    if name == "spinless16_k0_f64":
        assert (~case.live).any()  # fermions: k = 0 is the sector with vanishing orbits
    psi = _random_state(torch, reps[0], torch.complex128 if dt == "c128" else torch.float64)
    vec = case.full_vector(psi.cpu().numpy())
    assert abs(np.vdot(vec, vec).real - 1.0) < 1e-12
    want = reference(case.states, vec, case.M, jw=True, species=case.L if case.spinful else None)
    # the sign convention of the bit arithmetic is the one of the references' own c+_i c_j (three pairs, with modes in between)
    for i, j in ((0, 3), (5, 1), (case.M - 1, case.M - 4)):
        assert abs(R.one_body(case, vec, i, j) - want[2][i, j]) <= 1e-13
    pl = D.CorrelationPlan(basis, reps[0])
    assert pl.modes == case.M and pl.kernel(0) == "k_corr_diag" and pl.kernel(1) == kernel
    d, Dm = pl.densities(psi)
    G = pl.hoppings(psi)
    _compare(name, (d, Dm, G), want)
    if case.spinful:
        L = case.L
        assert (G[:L, L:] == 0).all() and (G[L:, :L] == 0).all()  # across the species: exactly zero, and no error flag
    fc = D.fermion_correlations(basis, reps[0], psi)
    # (fermion_correlations normalises psi once more: equal up to that rounding)
    assert max(np.abs(fc.n - d).max(), np.abs(fc.nn - Dm).max(), np.abs(fc.one_body - G).max()) <= 1e-14
    if case.spinful:
        assert np.array_equal(fc.double_occupancy, np.array([fc.nn[i, i + case.L] for i in range(case.L)]))
    else:
        assert fc.double_occupancy is None
    pl.destroy()


def test_spinful_basis_with_number_up_unset_is_spinless_over_its_modes(torch):
    """L = 6, N = 6, N_up free: 924 states over 12 modes; every pair of modes is evaluated, the pairs across the species included"""
    basis = D.loadConfigFromDict({"basis": {"particle": "spinful-fermion", "number_sites": 6, "number_particles": 6}})
    reps, _ = D.enumerateStates(basis, 1)
    case = R.Case(12, 6)  # the same words
    assert np.array_equal(_u64(reps[0]), case.states) and len(case.states) == 924
    psi = _random_state(torch, reps[0], torch.complex128)
    want = reference(case.states, psi.cpu().numpy(), 12, jw=True)
    pl = D.CorrelationPlan(basis, reps[0])
    assert pl.modes == 12 and pl.kernel(1) == "k_corr_hop"
    _compare("spinful6_number_up_unset", pl.densities(psi) + (pl.hoppings(psi),), want)
    assert np.abs(want[2][:6, 6:]).max() > 1e-3  # (they are not zero here)
    fc = D.fermion_correlations(basis, reps[0], psi)
    assert fc.double_occupancy.shape == (6,) and np.abs(fc.double_occupancy - np.array([want[1][i, i + 6] for i in range(6)])).max() <= ATOL
    pl.destroy()


@pytest.mark.parametrize("name", ["ring16_unprojected_f64", "ring16_k3_c128", "spinless16_k3_c128", "spinful8_k0_flip_plus"])
def test_several_tiles_per_block(torch, name, monkeypatch):
    """The sectors above have fewer tiles than the launch has blocks, so every block sees one tile.  LS_AMD_CORR_BLOCKS=3 makes three
    blocks walk them all -- 51, 4, 4 and 2 tiles: several per block, unevenly, or a block fewer -- through the accumulation of the
    block's partial sums from tile to tile, which is the path of every large sector."""
    monkeypatch.setenv("LS_AMD_CORR_BLOCKS", "3")
    if name in SPIN_CASES:
        make, dt, _ = SPIN_CASES[name]
        cfg = make()
        model, full = E.tables(cfg)[0], E.tables(cfg)[1]
        basis, reps = _spin_setup(cfg)
        psi = _random_state(torch, reps, torch.complex128 if dt == "c128" else torch.float64)
        want = reference(full, E.expand_full(cfg, psi.cpu().numpy()), model.number_sites, jw=False)
    else:
        make, dt, _ = FERMI_CASES[name]
        case = make()
        basis, _, reps = _fermi_setup(case)
        reps = reps[0]
        psi = _random_state(torch, reps, torch.complex128 if dt == "c128" else torch.float64)
        want = reference(case.states, case.full_vector(psi.cpu().numpy()), case.M, jw=True, species=case.L if case.spinful else None)
    pl = D.CorrelationPlan(basis, reps)
    got = pl.densities(psi) + (pl.hoppings(psi),)
    _compare(name + " (3 blocks)", got, want)
    assert pl.hoppings(psi).tobytes() == got[2].tobytes()
    pl.destroy()


# ---- ground states ---------------------------------------------------------------------------------------------------------------
def test_ground_states_against_the_expansion(torch):
    """the ground state of diagonalize() instead of a random vector: a Heisenberg ring in a momentum sector, a t-V ring"""
    from distributed_matvec_amd.diagonalize import diagonalize

    cfg = E.ring(16, 8, 0)
    cfg["hamiltonian"] = config_heisenberg_terms(16)
    r = diagonalize(cfg, num_evals=1, eps=1e-10)
    psi = r.eigenvectors[0] / torch.linalg.vector_norm(r.eigenvectors[0])
    basis, reps = _spin_setup(cfg)
    model, full = E.tables(cfg)[0], E.tables(cfg)[1]
    want = reference(full, E.expand_full(cfg, psi.cpu().numpy()), 16, jw=False)
    pl = D.CorrelationPlan(basis, reps)
    _compare("heisenberg_ring16_ground_state", pl.densities(psi) + (pl.hoppings(psi),), want)
    pl.destroy()
    case, tv = R.Case(16, 8, gens=F.translations(16), secs=[0]), F.tv_model(JW.ring(16), V=1.3)
    r = diagonalize(case.config(tv), num_evals=1, eps=1e-10)
    psi = r.eigenvectors[0] / torch.linalg.vector_norm(r.eigenvectors[0])
    basis, _, reps = _fermi_setup(case)
    want = reference(case.states, case.full_vector(psi.cpu().numpy()), 16, jw=True)
    pl = D.CorrelationPlan(basis, reps[0])
    _compare("tv_ring16_ground_state", pl.densities(psi) + (pl.hoppings(psi),), want)
    pl.destroy()


def config_heisenberg_terms(L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"name": "Heisenberg", "terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}


def test_heisenberg_chain_24_symm_identities(torch):
    """No dense reference reaches this size.  E0 = sum over the bonds of J (zz_ij + 2 pm_ij + 2 pm_ji) to the eigensolver's eps (the
    residual bounds the error of the Rayleigh quotient far below it); sum_ij <S_i.S_j> = S (S + 1) = 0 in the singlet; G = G+;
    sum_i d_i = the weight."""
    from distributed_matvec_amd.diagonalize import diagonalize

    eps = 1e-10
    cfg = model_config("heisenberg_chain_24_symm")
    r = diagonalize(cfg, num_evals=1, eps=eps)
    e0, psi = float(r.eigenvalues[0]), r.eigenvectors[0]
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    sc = D.spin_correlations(basis, reps[0], psi)
    bonds = 0.0
    scale = 0.0
    for term in cfg["hamiltonian"]["terms"]:
        if "σᶻ" not in term["expression"]:
            continue  # (the three components of every bond carry the same J: take the bonds once, from the zz term)
        J = parse_expression(term["expression"])[0].real
        for i, j in term["sites"]:
            bonds += J * (sc.zz[i, j] + 2.0 * sc.pm[i, j] + 2.0 * sc.pm[j, i]).real
            scale += 3.0 * abs(J)
    print(f"heisenberg_chain_24_symm: E0 = {e0:.12f}, bond sum = {bonds:.12f}, difference {abs(e0 - bonds):.2e} (eps {eps:.0e} x {scale:g})")
    assert abs(e0 - bonds) <= eps * scale
    # total spin 0: S^2 commutes with H, so an admixture delta of other multiplets enters <S^2> at delta^2; what is left is the rounding
    # of the 576 entries
    assert abs(sc.ss.sum()) <= 24 * 24 * ATOL
    pl = D.CorrelationPlan(basis, reps[0])
    psi = psi / torch.linalg.vector_norm(psi)
    d, _ = pl.densities(psi)
    G = pl.hoppings(psi)
    assert np.abs(G - G.conj().T).max() <= ATOL
    assert abs(d.sum() - 12.0) <= 24 * ATOL
    pl.destroy()


@pytest.mark.parametrize("U", [0.0, 4.0])
def test_hubbard_ring_identities(torch, U):
    """8 sites, translations (+ flip at U = 4): E = -t sum <c+c + h.c.> + U sum double_occupancy; Tr one_body = N; U = 0: the one-body
    matrix of a Slater determinant is a projector (eigenvalues 0 or 1 to 1e-10)"""
    from distributed_matvec_amd.diagonalize import diagonalize

    eps = 1e-10
    # U = 0: (4, 4) on 8 sites is an open shell (the level k = +-pi/2 half filled); (3, 3) is closed -- k = 0, +-pi/4 per species, total
    # momentum 0 -- and its ground state one Slater determinant
    up = (3, 3) if U == 0.0 else (4, 4)
    case = R.Case(8, up=up, gens=F.translations(8), secs=[0], flip=0 if U == 0.0 else 1)
    model = JW.hubbard_model(8, JW.ring(8), U=U)
    r = diagonalize(case.config(model), num_evals=1, eps=eps)
    e0, psi = float(r.eigenvalues[0]), r.eigenvectors[0]
    basis, _, reps = _fermi_setup(case)
    fc = D.fermion_correlations(basis, reps[0], psi)
    hop = sum((fc.one_body[i + s, j + s] + fc.one_body[j + s, i + s]).real for i, j in JW.ring(8) for s in (0, 8))
    energy = -1.0 * hop + U * fc.double_occupancy.sum()
    scale = 8 * (4.0 + U)
    print(f"hubbard U={U}: E0 = {e0:.12f}, from the correlations {energy:.12f}, difference {abs(e0 - energy):.2e}")
    assert abs(e0 - energy) <= eps * scale
    assert abs(np.trace(fc.one_body).real - sum(up)) <= 16 * ATOL and abs(np.trace(fc.one_body).imag) <= 16 * ATOL
    assert np.abs(fc.one_body - fc.one_body.conj().T).max() <= ATOL
    if U == 0.0:
        w = np.linalg.eigvalsh(fc.one_body)
        assert np.minimum(np.abs(w), np.abs(w - 1.0)).max() <= 1e-10, w


# ---- against Operator: the bit and sign conventions --------------------------------------------------------------------------------
def _expectation(torch, cfg_basis, term, reps, psi):
    basis, h = D.loadConfigFromDict({"basis": cfg_basis, "hamiltonian": {"name": "pair", "terms": [term]}}, hamiltonian=True)
    out = torch.zeros_like(psi)
    D.MatvecPlan(h, reps, psi.dtype).matvec([psi], [out])
    return complex(torch.vdot(psi, out))


def test_spin_pm_is_the_operators_sigma_plus_sigma_minus(torch):
    cfg = E.ring(12, 6, None)
    basis, reps = _spin_setup(cfg)
    psi = _random_state(torch, reps, torch.complex128)
    sc = D.spin_correlations(basis, reps, psi)
    worst = 0.0
    for i in range(12):
        for j in range(12):
            if i == j:
                continue
            want = _expectation(torch, cfg["basis"], {"expression": "σ⁺₀ σ⁻₁", "sites": [[i, j]]}, [reps], psi)
            worst = max(worst, abs(sc.pm[i, j] - want))
    print(f"<sigma+_i sigma-_j> against Operator, 132 pairs: max difference {worst:.2e}")
    assert worst <= ATOL


def test_one_body_is_the_operators_c_dagger_c(torch):
    case = R.Case(12, 6)
    basis, _, reps = _fermi_setup(case)
    psi = _random_state(torch, reps[0], torch.complex128)
    fc = D.fermion_correlations(basis, reps[0], psi)
    worst = 0.0
    for i in range(12):
        for j in range(12):
            if i == j:
                continue
            want = _expectation(torch, case.basis_config(), {"expression": "c†₀ c₁", "sites": [[i, j]]}, reps, psi)
            worst = max(worst, abs(fc.one_body[i, j] - want))
    print(f"<c+_i c_j> against Operator, 132 pairs: max difference {worst:.2e}")
    assert worst <= ATOL


# ---- reproducibility, the raw matrices, the failures -------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_and_raw_plus_hook_is_symmetrize(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    for cfg_or_case, dt in ((E.ring(16, 8, 3), torch.complex128), (R.Case(16, 8, gens=F.dihedral(16), secs=[0, 1]), torch.float64),
                            (E.ring(16, 8, 8, inv=-1, reflect=1), torch.float64)):
        if isinstance(cfg_or_case, dict):
            basis, reps = _spin_setup(cfg_or_case)
        else:
            basis, _, reps = _fermi_setup(cfg_or_case)
            reps = reps[0]
        psi = _random_state(torch, reps, dt, seed=5)
        pl = D.CorrelationPlan(basis, reps)
        a, b = pl.hoppings(psi), pl.hoppings(psi)
        assert a.tobytes() == b.tobytes()
        (d1, D1), (d2, D2) = pl.densities(psi), pl.densities(psi)
        assert d1.tobytes() == d2.tobytes() and D1.tobytes() == D2.tobytes()
        # a second plan over the same array: the same bytes again
        pl2 = D.CorrelationPlan(basis, reps)
        assert pl2.hoppings(psi).tobytes() == a.tobytes()
        pl2.destroy()
        raw = pl.hoppings(psi, symmetrize=False)
        out = np.zeros_like(raw)
        f64p = C.POINTER(C.c_double)
        assert L.ls_amd_test_corr_symmetrize(basis.payload, 1, raw.view(np.float64).ctypes.data_as(f64p), out.view(np.float64).ctypes.data_as(f64p)) == 0
        assert out.tobytes() == a.tobytes()
        assert np.abs(raw - a).max() > 1e-6  # (the raw sums over the representatives are not the averaged matrix)
        rd, rD = pl.densities(psi, symmetrize=False)
        rawd = np.concatenate([rd, rD.ravel()])
        outd = np.zeros_like(rawd)
        assert L.ls_amd_test_corr_symmetrize(basis.payload, 0, rawd.ctypes.data_as(f64p), outd.ctypes.data_as(f64p)) == 0
        M = pl.modes
        assert outd[:M].tobytes() == d1.tobytes() and outd[M:].tobytes() == D1.tobytes()
        pl.destroy()


def test_representatives_that_are_not_the_sector_raise_the_error_flag(torch):
    """A hand-made list on a 12-site weight-6 basis: 300 of its states and 300 states of the weight-5 sector.  The hoppings leave the
    list (and the weight-5 rows are on the wrong sector altogether): "not in the basis", never a wrong matrix, never a fault.  The
    plan stays usable: the flag is cleared, and the densities -- which look nothing up -- still come back."""
    cfg = E.ring(12, 6, None)
    basis, reps = _spin_setup(cfg)
    w6 = _u64(reps)[:300]
    w5 = JW.weight_states(12, 5)[:300]
    mixed = np.sort(np.concatenate([w6, w5]))
    bad = torch.from_numpy(mixed.view(np.int64)).cuda()
    psi = _random_state(torch, bad, torch.float64)
    pl = D.CorrelationPlan(basis, bad)
    for _ in range(2):
        with pytest.raises(LsAmdError, match="not in the basis"):
            pl.hoppings(psi)
    d, _ = pl.densities(psi)
    assert abs(d.sum() - float((psi.cpu().numpy() ** 2 * np.bitwise_count(mixed)).sum())) <= ATOL
    pl.destroy()
    # the same through a projected basis (static index table): a truncated list of representatives
    cfg = E.ring(12, 6, 0)
    basis, reps = _spin_setup(cfg)
    cut = reps[: reps.numel() // 2].contiguous()
    pl = D.CorrelationPlan(basis, cut)
    with pytest.raises(LsAmdError, match="not in the basis"):
        pl.hoppings(_random_state(torch, cut, torch.float64))
    pl.destroy()


def test_refusals_come_back_by_name(torch):
    basis, reps = _spin_setup(E.ring(12, 6, 5))  # complex characters
    pl = D.CorrelationPlan(basis, reps)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    psi = _random_state(torch, reps, torch.float64)
    out = np.zeros(12 * 12 * 2)
    f64p = C.POINTER(C.c_double)
    assert L.ls_amd_corr_hoppings(pl.h, 0, C.c_void_p(psi.data_ptr()), out.ctypes.data_as(f64p), 1, None) == -1
    assert "ls_amd_corr_hoppings: f64 needs +-1 characters" in L.ls_amd_last_error().decode()
    assert L.ls_amd_corr_densities(pl.h, 0, C.c_void_p(psi.data_ptr()), None, None, 1, None) == -1
    assert "ls_amd_corr_densities: f64 needs +-1 characters" in L.ls_amd_last_error().decode()
    assert L.ls_amd_corr_densities(pl.h, 7, C.c_void_p(psi.data_ptr()), None, None, 1, None) == -1 and "unknown dtype 7" in L.ls_amd_last_error().decode()
    assert L.ls_amd_corr_hoppings(pl.h, 1, C.c_void_p(psi.data_ptr()), None, 1, None) == -1 and "NULL output" in L.ls_amd_last_error().decode()
    assert L.ls_amd_corr_kernel_name(pl.h, 2) is None and "kernel 2" in L.ls_amd_last_error().decode()
    G = pl.hoppings(psi)  # float64 is promoted where the characters are complex
    assert G.dtype == np.complex128
    with pytest.raises(LsAmdError, match="ONE vector of"):
        pl.hoppings(psi[:-1])
    with pytest.raises(LsAmdError, match="neither float64 nor complex128"):
        pl.densities(psi.to(torch.float32))
    with pytest.raises(LsAmdError, match="device tensor"):
        pl.densities(psi.cpu())
    pl.destroy()
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.densities(psi)
    with pytest.raises(LsAmdError, match="fermion_correlations"):
        D.spin_correlations(D.loadConfigFromDict({"basis": R.Case(6, 3).basis_config()}), reps, psi)
    with pytest.raises(LsAmdError, match="spin_correlations"):
        D.fermion_correlations(basis, reps, psi)


def test_correlations_of_a_config_dispatch_on_the_particle_type(torch):
    cfg = E.ring(12, 6, 0)
    cfg["hamiltonian"] = config_heisenberg_terms(12)
    sc = D.correlations.correlations(cfg)
    assert isinstance(sc, D.SpinCorrelations) and sc.ss.shape == (12, 12)
    assert abs(sc.ss.sum()) <= 1e-8 and np.abs(sc.z).max() <= ATOL
    # translation invariance of the averaged matrix, and the structure factor at q = pi against the direct sum
    assert np.abs(sc.ss - np.roll(np.roll(sc.ss, 1, 0), 1, 1)).max() <= ATOL
    sq = D.structure_factor(sc.ss, np.arange(12), [np.pi, 0.0])
    assert abs(sq[0] - sum((-1) ** (i - j) * sc.ss[i, j] for i in range(12) for j in range(12)) / 12) <= 1e-12 and abs(sq[1]) <= 1e-8
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0])
    fc = D.correlations.correlations(case.config(JW.hubbard_model(6, JW.ring(6), U=4.0)))
    assert isinstance(fc, D.FermionCorrelations) and fc.one_body.shape == (12, 12) and fc.double_occupancy.shape == (6,)
    assert abs(np.trace(fc.one_body).real - 6.0) <= 12 * ATOL
