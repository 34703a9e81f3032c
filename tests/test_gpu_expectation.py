"""Expectation values of arbitrary operators on the GPU (ExpectationPlan / k_expect, k_expect_fermi; expectation_values,
dimer_correlations, pair_correlations) against the CPU expansions the tests own -- tests/entanglement_reference.expand_full for
spins, the projector columns of tests/fermion_entanglement_reference for fermions -- followed by plain numpy bit arithmetic with the
RAW terms of every operator over all product states; the 64-bit word path against unproject + a MatvecPlan of the same operator on
the symmetry-free basis + vdot (GPU code of earlier changes, independent of the new kernel); the conventions against
spin_correlations / fermion_correlations; identities at sizes no dense reference reaches (the dimer sum rule of a Heisenberg ground
state, Wick's theorem on Slater determinants); bitwise reproducibility; and the failures that must be loud.

Tolerance (the derivation of tests/test_gpu_correlations.py, not a tuned number): the value of operator k is a sum of at most
n |G| T products whose moduli sum to at most sum_t |v_t| for a normalised state (Cauchy-Schwarz per raw term); each summand carries
a handful of roundings, so with n <= 13 000 the worst case of recursive summation is about n 8 2^-53 ~ 1e-11 per unit of sum |v|:
ATOL_k = 2e-11 max(1, sum_t |v_t|).  A wrong sign, character or convention shows at 1e-2 or more."""
import ctypes as C

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_jw as JW
import fermion_symm as F
from distributed_matvec_amd import ExpectationPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from distributed_matvec_amd._lib import LsAmdError
from distributed_matvec_amd.api import Operator
from helpers import model_config

pytestmark = pytest.mark.gpu
ATOL = 2e-11
ONE = np.uint64(1)
SUBS = "₀₁₂₃"


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _random_state(torch, reps, dtype, seed=11):
    psi = D.fillRandom(reps, seed, dtype)
    return psi / torch.linalg.vector_norm(psi)


def raw_expectation(states, vec, terms):
    """<vec|O|vec> over the ascending product states `states`, O given by its raw terms (v, m, r, x, s):
    O|a> = v [a & m == r] (-1)^popcount(a & s) |a ^ x>; an image outside `states` is orthogonal to vec."""
    states = np.asarray(states, dtype=np.uint64)
    total = 0j
    for v, m, r, x, s in terms:
        sel = (states & np.uint64(m)) == np.uint64(r)
        a = states[sel]
        b = a ^ np.uint64(x)
        pos = np.minimum(np.searchsorted(states, b), len(states) - 1)
        hit = states[pos] == b
        sign = np.where(np.bitwise_count(a & np.uint64(s)) & 1, -1.0, 1.0)
        total += complex(v) * np.sum(np.conj(vec[pos[hit]]) * sign[hit] * vec[sel][hit])
    return total


def _atol(terms):
    return ATOL * max(1.0, sum(abs(t[0]) for t in terms))


def _coef(rs):
    z = complex(rs.randn(), rs.randn())
    return f"({z.real:.17g}{z.imag:+.17g}j)"


SPIN_SHAPES = (["σ⁺", "σ⁻", "σᶻ"], ["σˣ", "σˣ", "σᶻ"], ["σʸ", "σʸ", "σᶻ"], ["σˣ", "σʸ", "σᶻ"], ["σʸ", "σ⁺", "σ⁻"],
               ["σ⁺", "σ⁺", "σ⁻", "σ⁻"], ["σ⁺", "σ⁻", "σᶻ", "σᶻ"], ["σˣ", "σˣ", "σʸ", "σʸ"], ["σˣ", "σʸ", "σ⁺", "σ⁻"], ["σʸ", "σʸ", "σᶻ", "σᶻ"],
               ["σ⁺", "σ⁻", "σˣ", "σˣ"], ["σʸ", "σᶻ", "σˣ", "σᶻ"])


def spin_sections(rs, L, count, monomials=1):
    """operators of `monomials` random 3- and 4-site monomials each with a random complex coefficient: a shape above in a random order
    of its sites (most keep a part that conserves the weight; sigma^y sigma^+ sigma^- does not and vanishes on a fixed-weight basis),
    and one factor more on one of the sites, so that the site carries a composed operator"""
    out = []
    for _ in range(count):
        terms = []
        for _ in range(monomials):
            kinds = list(SPIN_SHAPES[int(rs.randint(len(SPIN_SHAPES)))])
            k = len(kinds)
            rs.shuffle(kinds)
            sites = [int(q) for q in rs.choice(L, size=k, replace=False)]
            kinds.append(str(rs.choice(["σᶻ", "σᶻ", "σᶻ", "σˣ", "σʸ"])))
            local = list(range(k)) + [int(rs.randint(k))]
            expr = " ".join(f"{a}{SUBS[i]}" for a, i in zip(kinds, local))
            terms.append({"expression": f"{_coef(rs)} × {expr}", "sites": [sites]})
        out.append({"terms": terms})
    return out


FERMI_SHAPES = (["c†", "c†", "c", "c"], ["n", "c†", "c", "n"], ["c†", "n", "c"], ["c†", "c", "n", "n"], ["n", "n", "n"], ["c†", "c", "c†", "c"])


def fermi_sections(rs, L, count, spinful):
    """random number-conserving 3- and 4-site monomials of c+, c, n (spinful: a random species per factor, so some change N_up and
    vanish exactly on the (N, N_up) basis)"""
    out = []
    for _ in range(count):
        shape = FERMI_SHAPES[int(rs.randint(len(FERMI_SHAPES)))]
        sites = [int(q) for q in rs.choice(L, size=len(shape), replace=False)]
        if spinful:
            arrows = [str(rs.choice(["↑", "↓"])) for _ in shape]
            if rs.rand() < 0.6:  # keep N_up: the species of the c+ are those of the c
                up = [a for a, k in zip(arrows, shape) if k == "c†"]
                it = iter(up)
                arrows = [next(it) if k == "c" else a for a, k in zip(arrows, shape)]
            expr = " ".join(f"{a}{SUBS[i]}{w}" for i, (a, w) in enumerate(zip(shape, arrows)))
        else:
            expr = " ".join(f"{a}{SUBS[i]}" for i, a in enumerate(shape))
        out.append({"terms": [{"expression": f"{_coef(rs)} × {expr}", "sites": [sites]}]})
    return out


def _torus_spin_config():
    tx, ty = F.torus(4, 3, point_group=False)
    return {"basis": {"number_spins": 12, "hamming_weight": 6, "symmetries": [{"permutation": tx, "sector": 0}, {"permutation": ty, "sector": 0}]}}


# name: (spin config or fermionic Case, dtype of psi, operators in the batch, monomials per operator)
CASES = {
    "ring16_k3_c128": (lambda: E.ring(16, 8, 3), "c128", 16, 1),
    "ring16_k3_c128_more_than_4096_terms": (lambda: E.ring(16, 8, 3), "c128", 20, 18),
    "ring16_k8_reflection_inversion_minus_f64": (lambda: E.ring(16, 8, 8, inv=-1, reflect=1), "f64", 20, 1),
    "torus_4x3_f64": (_torus_spin_config, "f64", 14, 1),
    "ring10_unprojected_c128": (lambda: E.ring(10, 5, None), "c128", 20, 1),
    "spinless12_dihedral_reflection_odd_f64": (lambda: R.Case(12, 6, gens=F.dihedral(12), secs=[0, 1]), "f64", 16, 1),
    "spinful6_k0_flip_plus_f64": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1), "f64", 18, 1),
    "spinful6_unprojected_product_c128": (lambda: R.Case(6, up=(3, 3)), "c128", 18, 1),
}


def _setup(torch, name):
    """(basis, reps, psi, states, full vector, sections): the references are computed once per case and shared, read-only"""
    make, dt, count, monomials = CASES[name]
    what = make()
    rs = np.random.RandomState(len(name))
    dtype = torch.complex128 if dt == "c128" else torch.float64
    if isinstance(what, dict):
        basis = D.loadConfigFromDict({"basis": what["basis"]})
        reps = D.enumerateStates(basis, 1)[0][0]
        model, full, want_reps = E.tables(what)[:3]
        assert np.array_equal(_u64(reps), want_reps)
        psi = _random_state(torch, reps, dtype)
        vec = E.expand_full(what, psi.cpu().numpy())
        sections = spin_sections(rs, model.number_sites, count, monomials)
        states = full
    else:
        basis = D.loadConfigFromDict(what.config())
        reps = D.enumerateStates(basis, 1)[0][0]
        assert np.array_equal(_u64(reps), what.reps)
        psi = _random_state(torch, reps, dtype)
        vec = what.full_vector(psi.cpu().numpy())
        sections = fermi_sections(rs, what.L, count, what.spinful)
        states = what.states
    assert abs(np.vdot(vec, vec).real - 1.0) < 1e-12
    return basis, reps, psi, states, vec, sections


@pytest.mark.parametrize("blocks", [None, 2])
@pytest.mark.parametrize("name", sorted(CASES))
def test_batches_match_the_expansion(torch, name, blocks, monkeypatch):
    """every operator of a random batch, with the default grid and with LS_AMD_CORR_BLOCKS=2 (two blocks walk all tiles: several tiles
    per block where the sector has more than 512 rows, through the accumulation of the block's partial sums from tile to tile)"""
    if blocks:
        monkeypatch.setenv("LS_AMD_CORR_BLOCKS", str(blocks))
    basis, reps, psi, states, vec, sections = _setup(torch, name)
    spec = basis.spec
    specs = [config.parse_operator(sec, spec) for sec in sections]
    keep = [k for k, s in enumerate(specs) if s.terms]  # (a monomial that vanishes identically has no terms)
    assert len(keep) >= 10
    want = np.array([raw_expectation(states, vec, specs[k].terms) for k in keep])
    pl = D.ExpectationPlan(basis, reps, [specs[k] for k in keep])
    fermi_kernel = not isinstance(CASES[name][0](), dict) and basis.hasFermionSigns()
    assert pl.kernel() == ("k_expect_fermi" if fermi_kernel else "k_expect")
    assert pl.num_terms > 0 and pl.num_groups > 0
    if name == "ring16_k3_c128":
        assert pl.num_groups > 8  # more flip-mask groups than one pass takes
        assert int(reps.numel()) == 800  # four tiles: two per block under LS_AMD_CORR_BLOCKS=2
    if name == "ring16_k3_c128_more_than_4096_terms":
        assert pl.num_terms > 4096  # more unique device terms than one launch takes
    got = pl.values(psi)
    assert got.shape == (len(keep),) and got.dtype == np.complex128 and np.isfinite(got).all()
    worst = 0.0
    for k, g, w in zip(keep, got, want):
        err, tol = abs(g - w), _atol(specs[k].terms)
        worst = max(worst, err / tol)
        assert err <= tol, (name, blocks, sections[k], g, w, err, tol)
    print(f"expectation {name} (blocks {blocks}): {len(keep)} operators, {pl.num_terms} device terms in {pl.num_groups} groups, "
          f"worst error / tolerance {worst:.2e}")
    assert (np.abs(want) > 1e-3).sum() >= 3  # (the batch does not vanish)
    assert pl.values(psi).tobytes() == got.tobytes()
    pl.destroy()


# ---- the 64-bit word path ----------------------------------------------------------------------------------------------------------
def test_64_bit_words_against_unproject_and_matvec(torch):
    """36 sites at weight 3, translations in sector k = 5 (complex characters): a few hundred representatives whose images reach above 2^32.  Reference: unproject +
    MatvecPlan of the same operator on the basis without symmetries + vdot.  The operators keep the weight, as the matvec needs."""
    cfg = E.ring(36, 3, 5)
    basis = D.loadConfigFromDict(cfg)
    reps = D.enumerateStates(basis, 1)[0][0]
    assert basis.numberBits() == 36 and reps.numel() < 256  # (orbit minima are small words: their images are not)
    plain = D.loadConfigFromDict(E.ring(36, 3, None))
    plain_reps, _ = D.enumerateStates(plain, 1)
    assert plain_reps[0].numel() == 7140 and int(_u64(plain_reps[0]).max()) >> 32
    psi = _random_state(torch, reps, torch.complex128)
    full = D.unproject(basis, reps, psi)
    assert full.numel() == 7140 and abs(float(torch.linalg.vector_norm(full)) - 1.0) < 1e-12
    rs = np.random.RandomState(36)
    sections = []
    for expr, k in (("σ⁺₀ σ⁻₁ σᶻ₂", 3), ("σ⁺₀ σ⁺₁ σ⁻₂ σ⁻₃", 4), ("σᶻ₀ σᶻ₁ σᶻ₂", 3), ("σ⁻₀ σᶻ₁ σ⁺₂ σᶻ₃", 4), ("σ⁺₀ σ⁻₀ σ⁺₁ σ⁻₂", 3),
                    ("σᶻ₀ σ⁺₁ σᶻ₁ σ⁻₂", 3)):
        for _ in range(2):
            near = int(rs.randint(36))
            sites = [(near + int(d)) % 36 for d in rs.choice(6, size=k, replace=False)]  # close together: weight 3 can reach them
            sections.append({"terms": [{"expression": f"{_coef(rs)} × {expr}", "sites": [sites]}]})
    sections.append({"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": [[35, 33]]}, {"expression": "0.5 × σᶻ₀ σᶻ₁", "sites": [[34, 35], [31, 32]]}]})
    assert any(max(s["terms"][0]["sites"][0]) >= 32 for s in sections)
    specs = [config.parse_operator(sec, basis.spec) for sec in sections]
    got = D.ExpectationPlan(basis, reps, specs).values(psi)
    worst = 0.0
    for sec, spec, g in zip(sections, specs, got):
        op = Operator.fromSpec(plain, spec)
        out = torch.zeros_like(full)
        D.MatvecPlan(op, plain_reps, full.dtype).matvec([full], [out])
        want = complex(torch.vdot(full, out))
        worst = max(worst, abs(g - want))
        assert abs(g - want) <= _atol(spec.terms), (sec, g, want)
    print(f"expectation ring36 weight 3 k = 5 (64-bit words): {len(sections)} operators, worst error {worst:.2e}")


# ---- conventions -------------------------------------------------------------------------------------------------------------------
def test_spin_and_fermion_conventions_are_those_of_the_two_point_functions(torch):
    """sigma^+_i sigma^-_j and c+_i c_j through ExpectationPlan equal spin_correlations.pm / fermion_correlations.one_body entry by
    entry (both sides are within ATOL of the exact value: 2 ATOL between them), the diagonal included"""
    cfg = E.ring(12, 6, 1)
    basis = D.loadConfigFromDict(cfg)
    reps = D.enumerateStates(basis, 1)[0][0]
    psi = _random_state(torch, reps, torch.complex128)
    sc = D.spin_correlations(basis, reps, psi)
    secs = [{"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": [[i, j]]}]} if i != j else {"terms": [{"expression": "σ⁺₀ σ⁻₀", "sites": [[i]]}]}
            for i in range(12) for j in range(12)]
    got = D.expectation_values(basis, reps, psi, secs).reshape(12, 12)
    print(f"<sigma+_i sigma-_j>: ExpectationPlan against spin_correlations.pm, max difference {np.abs(got - sc.pm).max():.2e}")
    assert np.abs(got - sc.pm).max() <= 2 * ATOL and np.abs(sc.pm).max() > 1e-2
    for case in (R.Case(12, 6, gens=F.translations(12), secs=[1]), R.Case(4, up=(2, 2), gens=F.translations(4), secs=[0], flip=-1)):
        basis = D.loadConfigFromDict(case.config())
        reps = D.enumerateStates(basis, 1)[0][0]
        psi = _random_state(torch, reps, torch.complex128)
        fc = D.fermion_correlations(basis, reps, psi)
        M, L = case.M, case.L
        arrow = (lambda q: "↑↓"[q // L]) if case.spinful else (lambda q: "")
        secs = [{"terms": [{"expression": f"c†₀{arrow(i)} c₁{arrow(j)}", "sites": [[i % L, j % L]]}]} if i % L != j % L else
                {"terms": [{"expression": f"c†₀{arrow(i)} c₀{arrow(j)}", "sites": [[i % L]]}]} for i in range(M) for j in range(M)]
        got = D.expectation_values(basis, reps, psi, secs).reshape(M, M)
        print(f"<c+_i c_j> ({M} modes): ExpectationPlan against fermion_correlations.one_body, max difference {np.abs(got - fc.one_body).max():.2e}")
        assert np.abs(got - fc.one_body).max() <= 2 * ATOL and np.abs(fc.one_body).max() > 1e-2


def test_images_outside_the_conserved_numbers_are_exactly_zero(torch):
    for cfg in (E.ring(12, 6, 0), E.ring(12, 6, None)):
        basis = D.loadConfigFromDict(cfg)
        reps = D.enumerateStates(basis, 1)[0][0]
        psi = _random_state(torch, reps, torch.float64)
        got = D.expectation_values(basis, reps, psi, [{"terms": [{"expression": "σˣ₀", "sites": [[0]]}]},
                                                      {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[0, 1]]}]}])
        assert got[0] == 0 and abs(got[1]) > 1e-3
    for case in (R.Case(10, 5, gens=F.translations(10), secs=[0]), R.Case(10, 5), R.Case(5, up=(2, 2)), R.Case(4, up=(2, 2), gens=F.translations(4), secs=[0])):
        basis = D.loadConfigFromDict(case.config())
        reps = D.enumerateStates(basis, 1)[0][0]
        psi = _random_state(torch, reps, torch.float64)
        a = "↑" if case.spinful else ""
        ops = [{"terms": [{"expression": f"c†₀{a}", "sites": [[0]]}]}, {"terms": [{"expression": f"n₀{a}", "sites": [[0]]}]}]
        if case.spinful:  # keeps N, changes N_up
            ops.append({"terms": [{"expression": "c†₀↑ c₁↓", "sites": [[0, 1]]}]})
        got = D.expectation_values(basis, reps, psi, ops)
        assert got[0] == 0 and abs(got[1]) > 1e-3 and (not case.spinful or got[2] == 0)


# ---- physics at sizes no dense reference reaches -------------------------------------------------------------------------------------
def test_dimer_sum_rule_of_heisenberg_chain_24_symm(torch):
    """H = sum_b sigma.sigma over the N_b bonds, D_b = S.S = sigma.sigma / 4: sum_b' <D_b D_b'> = <D_b H> / 4 = E0 <D_b> / 4 =
    E0^2 / (16 N_b) for every b (all bonds are equivalent under the sector's group).  |<D_b (H - E0)>| <= |D_b| |(H - E0) psi| gives
    the tolerance 0.75 eps |H| + N_b ATOL, |H| <= 3 N_b, eps the eigensolver's own bound."""
    from distributed_matvec_amd.diagonalize import diagonalize

    eps = 1e-10
    cfg = model_config("heisenberg_chain_24_symm")
    bonds = None
    for term in cfg["hamiltonian"]["terms"]:
        assert config.parse_expression(term["expression"])[0] == 1.0
        bonds = [tuple(b) for b in term["sites"]]
    nb = len(bonds)
    assert nb == 24
    r = diagonalize(cfg, num_evals=1, eps=eps)
    e0, psi = float(r.eigenvalues[0]), r.eigenvectors[0]
    basis = D.loadConfigFromDict(cfg)
    reps, _ = D.enumerateStates(basis, 1)
    Cm = D.dimer_correlations(basis, reps[0], psi, bonds)
    assert Cm.shape == (nb, nb) and np.array_equal(Cm, Cm.T)
    want = e0 * e0 / (16.0 * nb)
    tol = 0.75 * eps * 3 * nb + nb * ATOL
    rows = Cm.sum(axis=1)
    print(f"heisenberg_chain_24_symm: E0 = {e0:.12f}, E0^2 / (16 N_b) = {want:.12f}, row sums within {np.abs(rows - want).max():.2e} (tolerance {tol:.2e})")
    assert np.abs(rows - want).max() <= tol
    # <(S.S)^2> = 3 / 16 - <S.S> / 2 on the diagonal
    assert np.abs(np.diag(Cm) - (3.0 / 16.0 - 0.5 * e0 / (4.0 * nb))).max() <= 0.75 * eps * 3 * nb + ATOL


def _local(sites):
    """distinct sites in order of appearance, and the local index of every entry"""
    distinct = []
    for q in sites:
        if q not in distinct:
            distinct.append(q)
    return distinct, [distinct.index(q) for q in sites]


def test_wick_theorem_on_the_spinless_ring(torch):
    """12 modes, N = 5, V = 0, k = 0: a closed shell (momenta 0, +-1, +-2), the ground state one Slater determinant, so
    <c+_i c+_j c_k c_l> = G_il G_jk - G_ik G_jl for all (j, k, l) at i = 0.  The quadruples with j = i or k = l vanish identically on
    both sides (no operator is built for them).  Tolerance 1e-9: the eigenvector comes at eps = 1e-10; a dropped sign shows at 1e-2."""
    from distributed_matvec_amd.diagonalize import diagonalize

    case = R.Case(12, 5, gens=F.translations(12), secs=[0])
    r = diagonalize(case.config(F.tv_model(JW.ring(12), V=0.0)), num_evals=1, eps=1e-10)
    psi = r.eigenvectors[0]
    assert abs(float(r.eigenvalues[0]) - F.free_ring_energy(12, 5, 0)) <= 1e-9
    basis = D.loadConfigFromDict(case.config())
    reps = D.enumerateStates(basis, 1)[0][0]
    G = D.fermion_correlations(basis, reps, psi).one_body
    i = 0
    quads, secs = [], []
    for j in range(12):
        for k in range(12):
            for l in range(12):
                if j == i or k == l:
                    assert G[i, l] * G[j, k] - G[i, k] * G[j, l] == 0
                    continue
                distinct, loc = _local([i, j, k, l])
                quads.append((j, k, l))
                secs.append({"terms": [{"expression": f"c†{SUBS[loc[0]]} c†{SUBS[loc[1]]} c{SUBS[loc[2]]} c{SUBS[loc[3]]}", "sites": [distinct]}]})
    assert len(secs) == 11 * 132
    got = D.expectation_values(basis, reps, psi, secs)
    want = np.array([G[i, l] * G[j, k] - G[i, k] * G[j, l] for j, k, l in quads])
    print(f"Wick, spinless ring 12 at N = 5: {len(secs)} four-point functions, max difference {np.abs(got - want).max():.2e}; largest {np.abs(want).max():.3f}")
    assert np.abs(got - want).max() <= 1e-9 and np.abs(want).max() > 1e-2


def test_wick_theorem_for_the_pairs_of_the_free_hubbard_ring(torch):
    """U = 0, 8 sites, (3, 3), k = 0: the product of two closed-shell determinants, so P[i][j] = <c+_i up c_j up> <c+_i down c_j down>"""
    from distributed_matvec_amd.diagonalize import diagonalize

    case = R.Case(8, up=(3, 3), gens=F.translations(8), secs=[0])
    r = diagonalize(case.config(JW.hubbard_model(8, JW.ring(8), U=0.0)), num_evals=1, eps=1e-10)
    psi = r.eigenvectors[0]
    basis = D.loadConfigFromDict(case.config())
    reps = D.enumerateStates(basis, 1)[0][0]
    G = D.fermion_correlations(basis, reps, psi).one_body
    P = D.pair_correlations(basis, reps, psi)
    want = G[:8, :8] * G[8:, 8:]
    print(f"pairs of the free Hubbard ring: max difference {np.abs(P - want).max():.2e}; largest {np.abs(want).max():.3f}")
    assert P.shape == (8, 8) and np.abs(P - want).max() <= 1e-9 and np.abs(want).max() > 1e-2
    sub = D.pair_correlations(basis, reps, psi, sites=[5, 2])
    assert np.abs(sub - P[np.ix_([5, 2], [5, 2])]).max() <= 2 * ATOL


def test_expectation_of_a_config_finds_the_ground_state(torch):
    cfg = E.ring(12, 6, 0)
    bonds = [[i, (i + 1) % 12] for i in range(12)]
    cfg["hamiltonian"] = {"name": "Heisenberg", "terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}
    from distributed_matvec_amd.diagonalize import diagonalize

    e0 = float(diagonalize(cfg, num_evals=1, eps=1e-10).eigenvalues[0])
    got = D.expectation.expectation(cfg, [cfg["hamiltonian"], {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[3, 4]]}]}])
    assert abs(got[0] - e0) <= 1e-10 * 36 and abs(got[1] - e0 / 36) <= 1e-10 * 36


# ---- reproducibility and the failures ----------------------------------------------------------------------------------------------
def test_two_calls_and_two_plans_are_bitwise_equal(torch):
    for name in ("ring16_k3_c128", "spinless12_dihedral_reflection_odd_f64", "ring16_k8_reflection_inversion_minus_f64"):
        basis, reps, psi, _states, _vec, sections = _setup(torch, name)
        specs = [s for s in (config.parse_operator(sec, basis.spec) for sec in sections) if s.terms]
        pl = D.ExpectationPlan(basis, reps, specs)
        a, b = pl.values(psi), pl.values(psi)
        assert a.tobytes() == b.tobytes()
        pl2 = D.ExpectationPlan(basis, reps, specs)
        assert pl2.values(psi).tobytes() == a.tobytes()
        pl2.destroy()
        pl.destroy()


def test_representatives_that_are_not_the_sector_raise_the_error_flag(torch):
    """the lower half of the representatives: on the unprojected basis these are the 462 words with bit 11 clear, and sigma^+_11 sends
    each of them to a word with bit 11 set -- inside the weight sector, not in the array"""
    sec = {"terms": [{"expression": "σ⁻₀ σ⁺₁ σᶻ₂", "sites": [[0, 11, 7]]}]}
    for cfg in (E.ring(12, 6, 0), E.ring(12, 6, None)):  # the static index table, and the searched index of an incomplete array
        basis = D.loadConfigFromDict(cfg)
        reps = D.enumerateStates(basis, 1)[0][0]
        cut = reps[: reps.numel() // 2].contiguous()
        pl = D.ExpectationPlan(basis, cut, [sec])
        psi = _random_state(torch, cut, torch.float64)
        for _ in range(2):  # (the flag is cleared: the plan stays usable and keeps refusing)
            with pytest.raises(LsAmdError, match="not in the basis"):
                pl.values(psi)
        pl.destroy()


def test_refusals_come_back_by_name(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    basis = D.loadConfigFromDict(E.ring(12, 6, 5))  # complex characters
    reps = D.enumerateStates(basis, 1)[0][0]
    sec = {"terms": [{"expression": "σ⁺₀ σ⁻₁ σᶻ₂", "sites": [[0, 5, 7]]}]}
    pl = D.ExpectationPlan(basis, reps, [sec, config.parse_operator(sec, basis.spec), Operator.fromSpec(basis, config.parse_operator(sec, basis.spec))])
    psi = _random_state(torch, reps, torch.float64)
    out = np.zeros(6)
    f64p = C.POINTER(C.c_double)
    assert L.ls_amd_expect_values(pl.h, 0, C.c_void_p(psi.data_ptr()), out.ctypes.data_as(f64p), None) == -1
    assert "ls_amd_expect_values: f64 needs +-1 characters" in L.ls_amd_last_error().decode()
    assert L.ls_amd_expect_values(pl.h, 7, C.c_void_p(psi.data_ptr()), out.ctypes.data_as(f64p), None) == -1 and "unknown dtype 7" in L.ls_amd_last_error().decode()
    assert L.ls_amd_expect_values(pl.h, 1, C.c_void_p(psi.data_ptr()), None, None) == -1 and "NULL output" in L.ls_amd_last_error().decode()
    got = pl.values(psi)  # float64 is promoted where the characters are complex
    assert got.shape == (3,) and got[0] == got[1] == got[2]  # a section, an OperatorSpec and an Operator are the same operator
    with pytest.raises(LsAmdError, match="ONE vector of"):
        pl.values(psi[:-1])
    with pytest.raises(LsAmdError, match="neither float64 nor complex128"):
        pl.values(psi.to(torch.float32))
    with pytest.raises(LsAmdError, match="device tensor"):
        pl.values(psi.cpu())
    pl.destroy()
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.values(psi)
    other = D.loadConfigFromDict(E.ring(12, 6, 0))
    with pytest.raises(LsAmdError, match="an operator of another basis"):
        D.ExpectationPlan(basis, reps, [Operator.fromSpec(other, config.parse_operator(sec, other.spec))])
    with pytest.raises(LsAmdError, match="neither an Operator"):
        D.ExpectationPlan(basis, reps, ["σˣ₀"])
    with pytest.raises(LsAmdError, match="no operators"):
        D.ExpectationPlan(basis, reps, [])
    with pytest.raises(LsAmdError, match="pair_correlations"):
        D.dimer_correlations(D.loadConfigFromDict({"basis": R.Case(6, 3).basis_config()}), reps, psi, [(0, 1)])
    with pytest.raises(LsAmdError, match="dimer_correlations"):
        D.pair_correlations(basis, reps, psi)
