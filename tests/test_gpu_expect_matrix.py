"""Matrix elements of arbitrary operators between blocks of sector states on the GPU (ExpectationPlan.matrix_elements / k_expect_mat,
k_expect_mat_fermi; matrix_elements, eigenstate_matrix_elements) against the CPU expansion of every column followed by numpy bit
arithmetic with the raw terms (raw_matrix_element, next to raw_expectation of tests/test_gpu_expectation.py), against the kernel
itself one pair of columns at a time (the chunks of 8 x 8 columns and their tails), against values_block on the diagonal, against
the adjoint operators, against the polarisation identity over the unchanged values_block, against unproject + MatvecPlan + vdot on
64-bit words, and against H itself where only the sum of the operators is invariant.

Tolerance: that of tests/test_gpu_expectation.py per operator and per pair of normalised columns, ATOL_k = 2e-11 max(1, sum_t |v_t|):
the summands of <phi|O|psi> are those of <psi|O|psi> with one factor from another unit vector, and Cauchy-Schwarz bounds their moduli
by sum_t |v_t| |phi| |psi| in the same way.  Two device results that are each within ATOL_k of the exact value differ by 2 ATOL_k."""
import ctypes as C
import functools

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
from distributed_matvec_amd import config, eigenstate_matrix_elements, matrix_elements  # noqa: F401  (the feature under test)
from distributed_matvec_amd._lib import LsAmdError
from distributed_matvec_amd.api import Operator
from test_gpu_expectation import CASES, _atol, _coef, _setup, _u64

pytestmark = pytest.mark.gpu
BIG = "ring16_k3_c128_more_than_4096_terms"
BRA_SEEDS, KET_SEEDS = (21, 22, 23), (31, 32, 33, 34, 35)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    assert hasattr(D.ExpectationPlan, "matrix_elements") and hasattr(D.ExpectationPlan, "matrix_kernel")
    return t


def raw_matrix_element(states, bra_vec, ket_vec, terms):
    """<bra|O|ket> over the ascending product states `states`, O given by its raw terms (v, m, r, x, s):
    O|a> = v [a & m == r] (-1)^popcount(a & s) |a ^ x>; an image outside `states` is orthogonal to bra.  bra_vec and ket_vec may be
    blocks (len(states), K): the result is then (Ka, Kb)."""
    states = np.asarray(states, dtype=np.uint64)
    B, K = np.asarray(bra_vec), np.asarray(ket_vec)
    B2, K2 = B.reshape(len(states), -1), K.reshape(len(states), -1)
    total = np.zeros((B2.shape[1], K2.shape[1]), dtype=np.complex128)
    for v, m, r, x, s in terms:
        sel = (states & np.uint64(m)) == np.uint64(r)
        a = states[sel]
        b = a ^ np.uint64(x)
        pos = np.minimum(np.searchsorted(states, b), len(states) - 1)
        hit = states[pos] == b
        sign = np.where(np.bitwise_count(a & np.uint64(s)) & 1, -1.0, 1.0)
        total += complex(v) * (np.conj(B2[pos[hit]]).T @ (sign[hit, None] * K2[sel][hit]))
    return total if B.ndim == 2 or K.ndim == 2 else total[0, 0]


def _columns(torch, reps, dtype, seeds, normalise=True):
    cols = [D.fillRandom(reps, s, dtype) for s in seeds]
    if normalise:
        cols = [c / torch.linalg.vector_norm(c) for c in cols]
    return torch.stack(cols, dim=1).contiguous()


def _family(name, basis):
    fermi = not isinstance(CASES[name][0](), dict) and basis.hasFermionSigns()
    return "k_expect_mat_fermi" if fermi else "k_expect_mat"


def _full(what, block):
    cols = block.cpu().numpy()
    full = [E.expand_full(what, cols[:, c]) if isinstance(what, dict) else what.full_vector(cols[:, c]) for c in range(cols.shape[1])]
    return np.stack(full, axis=1)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(basis, reps, bra (n, 3), ket (n, 5), specs, sections, dense matrix elements (n_ops, 3, 5)): once per case, read-only"""
    import torch

    basis, reps, psi, states, _vec, sections = _setup(torch, name)
    what = CASES[name][0]()
    specs = [config.parse_operator(sec, basis.spec) for sec in sections]
    keep = [k for k, s in enumerate(specs) if s.terms]  # (a monomial that vanishes identically has no terms)
    bra, ket = _columns(torch, reps, psi.dtype, BRA_SEEDS), _columns(torch, reps, psi.dtype, KET_SEEDS)
    fb, fk = _full(what, bra), _full(what, ket)
    assert np.abs(np.sum(np.abs(fb) ** 2, axis=0) - 1.0).max() < 1e-12 and np.abs(np.sum(np.abs(fk) ** 2, axis=0) - 1.0).max() < 1e-12
    want = np.array([raw_matrix_element(states, fb, fk, specs[k].terms) for k in keep])
    return basis, reps, bra, ket, [specs[k] for k in keep], [sections[k] for k in keep], want


def _tols(specs):
    return np.array([_atol(s.terms) for s in specs])[:, None, None]


# ---- 1: entry by entry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [None, 2])
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != BIG))
def test_every_entry_matches_the_expansion(torch, name, blocks, monkeypatch):
    """Ka = 3 independent bra and Kb = 5 independent ket columns of every case, random non-Hermitian operators with complex
    coefficients (a transposed or mis-conjugated result is off by the size of the entries), with the default grid and with
    LS_AMD_CORR_BLOCKS=2 (ring16_k3_c128 has 800 rows, four tiles: a block accumulates its partial sums across two)"""
    if blocks:
        monkeypatch.setenv("LS_AMD_CORR_BLOCKS", str(blocks))
    basis, reps, bra, ket, specs, sections, want = _case(name)
    assert len(specs) >= 10 and want.shape == (len(specs), 3, 5)
    tol = _tols(specs)
    # the test cannot pass on zeros: a quarter of the reference's entries off the diagonal a == b are far above the tolerance
    off = ~np.eye(3, 5, dtype=bool)
    big = (np.abs(want) > 100 * tol)[:, off]
    print(f"matrix_elements {name}: {big.mean():.2f} of the reference's entries with a != b exceed 100 tolerances")
    assert big.mean() >= 0.25, (name, big.mean())
    pl = D.ExpectationPlan(basis, reps, specs)
    assert pl.matrix_kernel(3, 5) == _family(name, basis)
    if name == "ring16_k3_c128":
        assert pl.num_groups > 8 and int(reps.numel()) == 800
    got = pl.matrix_elements(bra, ket)
    assert got.shape == (len(specs), 3, 5) and got.dtype == np.complex128 and np.isfinite(got).all()
    ratio = np.abs(got - want) / tol
    print(f"matrix_elements {name} (blocks {blocks}): {len(specs)} operators x 3 x 5 columns, {pl.num_terms} device terms in "
          f"{pl.num_groups} groups, worst error / tolerance {ratio.max():.2e}")
    assert ratio.max() <= 1.0, (name, blocks, np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())
    pl.destroy()


# ---- 2: chunks and tails -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring16_k3_c128", "spinful6_k0_flip_plus_f64"])
def test_chunks_of_columns_and_their_tails(torch, name):
    """(Ka, Kb) = (1, 1), (1, 9), (9, 1), (8, 8), (9, 17) against the same entries computed one pair at a time with Ka = Kb = 1"""
    basis, reps, bra3, _ket, specs, _sections, _want = _case(name)
    pl = D.ExpectationPlan(basis, reps, specs)
    A, B = _columns(torch, reps, bra3.dtype, range(100, 109)), _columns(torch, reps, bra3.dtype, range(200, 217))
    single = np.zeros((len(specs), 9, 17), dtype=np.complex128)
    for a in range(9):
        for b in range(17):
            single[:, a, b] = pl.matrix_elements(A[:, a], B[:, b])[:, 0, 0]
    tol = 2 * _tols(specs)
    for Ka, Kb in ((1, 1), (1, 9), (9, 1), (8, 8), (9, 17)):
        assert pl.matrix_kernel(Ka, Kb) == _family(name, basis)
        got = pl.matrix_elements(A[:, :Ka], B[:, :Kb])
        assert got.shape == (len(specs), Ka, Kb)
        ratio = np.abs(got - single[:, :Ka, :Kb]) / tol
        print(f"matrix_elements {name} Ka = {Ka}, Kb = {Kb}: worst difference / tolerance against single pairs {ratio.max():.2e}")
        assert ratio.max() <= 1.0, (name, Ka, Kb, np.unravel_index(ratio.argmax(), ratio.shape))
    assert np.abs(single).max() > 1e-3
    pl.destroy()


# ---- 3: layouts ----------------------------------------------------------------------------------------------------------------------
def test_layouts_agree_and_unused_columns_do_not_leak(torch):
    basis, reps, _bra, _ket, specs, _sections, _want = _case("ring16_k3_c128")
    pl = D.ExpectationPlan(basis, reps, specs)
    n = int(reps.numel())

    def layouts(inter):
        K = inter.shape[1]
        colmajor = inter.t().contiguous().t()
        wide = torch.full((n, 2 * K), float("nan"), dtype=inter.dtype, device=inter.device)
        wide[:, 1::2] = inter
        view = wide[:, 1::2]
        assert inter.stride() == (K, 1) and colmajor.stride() == (1, n) and view.stride() == (2 * K, 2)
        return {"interleaved": inter, "colmajor": colmajor, "strided": view}

    bras, kets = layouts(_columns(torch, reps, torch.complex128, range(40, 43))), layouts(_columns(torch, reps, torch.complex128, range(50, 55)))
    ref = pl.matrix_elements(bras["interleaved"], kets["interleaved"])
    tol = 2 * _tols(specs)
    for lb, lk in (("interleaved", "colmajor"), ("colmajor", "strided"), ("strided", "interleaved"), ("strided", "strided"), ("colmajor", "colmajor")):
        got = pl.matrix_elements(bras[lb], kets[lk])
        assert not np.isnan(got).any(), (lb, lk)
        assert (np.abs(got - ref) <= tol).all(), (lb, lk, np.abs(got - ref).max())
    assert np.abs(ref).max() > 1e-3
    pl.destroy()


# ---- 4: the diagonal -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring16_k3_c128", "spinless12_dihedral_reflection_odd_f64"])
def test_the_diagonal_is_values_block_and_a_missing_ket_is_the_bra(torch, name):
    basis, reps, _bra, ket, specs, _sections, _want = _case(name)
    pl = D.ExpectationPlan(basis, reps, specs)
    both = pl.matrix_elements(ket, ket)
    diag = pl.values_block(ket)
    tol = 2 * _tols(specs)[:, :, 0]
    got = np.stack([both[:, c, c] for c in range(5)], axis=1)
    print(f"matrix_elements {name}: diagonal against values_block, worst difference / tolerance {(np.abs(got - diag) / tol).max():.2e}")
    assert (np.abs(got - diag) <= tol).all() and np.abs(diag).max() > 1e-3
    assert pl.matrix_elements(ket).tobytes() == both.tobytes()
    pl.destroy()


# ---- 5: the adjoint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring16_k3_c128", "spinful6_k0_flip_plus_f64"])
def test_the_adjoint_operator_gives_the_conjugate_transpose(torch, name):
    """M_O(Phi, Psi)[a, b] = conj(M_{O^+}(Psi, Phi)[b, a]), O and O^+ in one plan"""
    basis, reps, bra, ket, specs, _sections, _want = _case(name)
    ops = [Operator.fromSpec(basis, s) for s in specs]
    pl = D.ExpectationPlan(basis, reps, ops + [o.adjoint() for o in ops])
    K = len(ops)
    fwd, back = pl.matrix_elements(bra, ket), pl.matrix_elements(ket, bra)
    diff = np.abs(fwd[:K] - np.conj(back[K:].transpose(0, 2, 1)))
    tol = 2 * _tols(specs)
    print(f"matrix_elements {name}: O against O^+, worst difference / tolerance {(diff / tol).max():.2e}")
    assert (diff <= tol).all() and np.abs(fwd[:K]).max() > 1e-3
    # (and the operators are not Hermitian: the plain transpose is far off)
    assert np.abs(fwd[:K] - np.conj(back[:K].transpose(0, 2, 1))).max() > 1e-3
    pl.destroy()


# ---- 6: polarisation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring16_k3_c128", "ring16_k8_reflection_inversion_minus_f64", "spinful6_k0_flip_plus_f64"])
def test_polarisation_over_values_block_agrees(torch, name, monkeypatch):
    """each of the four combinations phi +- psi, phi +- i psi has squared norm <= 4 and carries one ATOL_k per unit of it; the result
    is a quarter of their sum: 4 ATOL_k, next to the kernel's own ATOL_k -- 8 ATOL_k bounds the difference"""
    basis, reps, bra, ket, specs, _sections, want = _case(name)
    pl = D.ExpectationPlan(basis, reps, specs)
    kernel = pl.matrix_elements(bra, ket)
    assert pl.matrix_elements(bra, ket, method="kernel").tobytes() == kernel.tobytes()
    tol = 8 * _tols(specs)
    pol = pl.matrix_elements(bra, ket, method="polarisation")
    print(f"matrix_elements {name}: polarisation against the kernel, worst difference / tolerance {(np.abs(pol - kernel) / tol).max():.2e}")
    assert pol.shape == kernel.shape and (np.abs(pol - kernel) <= tol).all()
    assert pl.matrix_kernel(3, 5) == _family(name, basis) and pl.matrix_kernel(3, 5, method="polarisation") == "polarisation"
    monkeypatch.setenv("LS_AMD_EXPECT_MATRIX", "polarisation")
    assert pl.matrix_kernel(3, 5) == "polarisation"
    env = pl.matrix_elements(bra, ket)
    assert (np.abs(env - kernel) <= tol).all() and env.tobytes() == pol.tobytes()
    assert pl.matrix_elements(bra, ket, method="kernel").tobytes() == kernel.tobytes()  # (the argument wins)
    monkeypatch.setenv("LS_AMD_EXPECT_MATRIX", "kernel")
    assert pl.matrix_kernel(3, 5) == _family(name, basis) and pl.matrix_elements(bra, ket).tobytes() == kernel.tobytes()
    monkeypatch.setenv("LS_AMD_EXPECT_MATRIX", "auto")
    assert pl.matrix_kernel(3, 5) == _family(name, basis)
    monkeypatch.setenv("LS_AMD_EXPECT_MATRIX", "fast")
    with pytest.raises(LsAmdError, match="LS_AMD_EXPECT_MATRIX"):
        pl.matrix_elements(bra, ket)
    pl.destroy()


# ---- 7: the launch split -------------------------------------------------------------------------------------------------------------
def test_more_than_4096_terms_split_by_terms_and_by_both_chunk_axes(torch):
    basis, reps, psi, states, _vec, sections = _setup(torch, BIG)
    what = CASES[BIG][0]()
    specs = [s for s in (config.parse_operator(sec, basis.spec) for sec in sections) if s.terms]
    pl = D.ExpectationPlan(basis, reps, specs)
    assert pl.num_terms > 4096  # more than one launch of terms; 4096 x 9 x 9 > 8 x 4096: one launch takes one bra x 8 ket columns
    bra, ket = _columns(torch, reps, psi.dtype, range(300, 309)), _columns(torch, reps, psi.dtype, range(400, 409))
    fb, fk = _full(what, bra), _full(what, ket)
    want = np.array([raw_matrix_element(states, fb, fk, s.terms) for s in specs])
    got = pl.matrix_elements(bra, ket)
    ratio = np.abs(got - want) / _tols(specs)
    print(f"matrix_elements {BIG}: {pl.num_terms} device terms, 9 x 9 columns, worst error / tolerance {ratio.max():.2e}")
    assert got.shape == (len(specs), 9, 9) and ratio.max() <= 1.0, np.unravel_index(ratio.argmax(), ratio.shape)
    assert (np.abs(want) > 100 * _tols(specs)).mean() >= 0.25
    pl.destroy()


# ---- 8: determinism ------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_plans_are_bitwise_equal(torch):
    for name in ("ring16_k3_c128", "ring16_k8_reflection_inversion_minus_f64", "spinless12_dihedral_reflection_odd_f64",
                 "spinful6_unprojected_product_c128"):
        basis, reps, bra3, _ket, specs, _sections, _want = _case(name)
        bra, ket = _columns(torch, reps, bra3.dtype, range(20, 31)), _columns(torch, reps, bra3.dtype, range(60, 69))
        pl = D.ExpectationPlan(basis, reps, specs)
        a, b = pl.matrix_elements(bra, ket), pl.matrix_elements(bra, ket)
        assert a.tobytes() == b.tobytes() and np.abs(a).max() > 1e-3
        pl2 = D.ExpectationPlan(basis, reps, specs)
        assert pl2.matrix_elements(bra, ket).tobytes() == a.tobytes()
        pl2.destroy()
        pl.destroy()


# ---- 9: promotion --------------------------------------------------------------------------------------------------------------------
def test_float64_blocks_are_promoted(torch):
    basis, reps, _bra, _ket, specs, _sections, _want = _case("ring16_k3_c128")  # complex characters
    pl = D.ExpectationPlan(basis, reps, specs)
    rb, rk = _columns(torch, reps, torch.float64, (5, 6, 7)), _columns(torch, reps, torch.float64, (8, 9))
    a = pl.matrix_elements(rb, rk)
    assert a.tobytes() == pl.matrix_elements(rb.to(torch.complex128), rk.to(torch.complex128)).tobytes() and np.abs(a).max() > 1e-3
    pl.destroy()
    basis, reps, _bra, _ket, specs, _sections, _want = _case("ring16_k8_reflection_inversion_minus_f64")  # +-1 characters
    pl = D.ExpectationPlan(basis, reps, specs)
    rb, ck = _columns(torch, reps, torch.float64, (5, 6, 7)), _columns(torch, reps, torch.complex128, (8, 9))
    mixed = pl.matrix_elements(rb, ck)  # a float64 bra next to a complex128 ket
    assert mixed.tobytes() == pl.matrix_elements(rb.to(torch.complex128), ck).tobytes() and np.abs(mixed.imag).max() > 1e-3
    rk = _columns(torch, reps, torch.float64, (8, 9))
    real, cplx = pl.matrix_elements(rb, rk), pl.matrix_elements(rb.to(torch.complex128), rk.to(torch.complex128))
    assert (np.abs(real - cplx) <= 2 * _tols(specs)).all()  # (the f64 kernel against the c128 one)
    pl.destroy()


# ---- 10: 64-bit words ----------------------------------------------------------------------------------------------------------------
def test_64_bit_words_against_unproject_and_matvec(torch):
    """36 sites at weight 3, translations in sector k = 5 (the basis of test_64_bit_words_against_unproject_and_matvec): images above
    2^32, Ka = Kb = 2.  Reference: unproject of every column, a MatvecPlan of the same operator on the basis without symmetries, vdot.
    The last operator is the sum of a monomial over all translations -- invariant under the group; the others are not."""
    basis = D.loadConfigFromDict(E.ring(36, 3, 5))
    reps = D.enumerateStates(basis, 1)[0][0]
    assert basis.numberBits() == 36 and reps.numel() < 256
    plain = D.loadConfigFromDict(E.ring(36, 3, None))
    plain_reps, _ = D.enumerateStates(plain, 1)
    assert plain_reps[0].numel() == 7140 and int(_u64(plain_reps[0]).max()) >> 32
    rs = np.random.RandomState(36)
    sections = []
    for expr, k in (("σ⁺₀ σ⁻₁ σᶻ₂", 3), ("σ⁺₀ σ⁺₁ σ⁻₂ σ⁻₃", 4), ("σᶻ₀ σᶻ₁ σᶻ₂", 3), ("σ⁻₀ σᶻ₁ σ⁺₂ σᶻ₃", 4)):
        for _ in range(2):
            near = int(rs.randint(36))
            sites = [(near + int(d)) % 36 for d in rs.choice(6, size=k, replace=False)]
            sections.append({"terms": [{"expression": f"{_coef(rs)} × {expr}", "sites": [sites]}]})
    sections.append({"terms": [{"expression": "σ⁺₀ σ⁻₁", "sites": [[35, 33]]}, {"expression": "0.5 × σᶻ₀ σᶻ₁", "sites": [[34, 35], [31, 32]]}]})
    sections.append({"terms": [{"expression": f"{_coef(rs)} × σ⁺₀ σ⁻₁ σᶻ₂", "sites": [[i, (i + 2) % 36, (i + 3) % 36] for i in range(36)]}]})
    specs = [config.parse_operator(sec, basis.spec) for sec in sections]
    pl = D.ExpectationPlan(basis, reps, specs)
    assert pl.matrix_kernel(2, 2) == "k_expect_mat"
    bra, ket = _columns(torch, reps, torch.complex128, (11, 12)), _columns(torch, reps, torch.complex128, (13, 14))
    got = pl.matrix_elements(bra, ket)
    fb = [D.unproject(basis, reps, bra[:, a].contiguous()) for a in range(2)]
    fk = [D.unproject(basis, reps, ket[:, b].contiguous()) for b in range(2)]
    worst = 0.0
    for k, spec in enumerate(specs):
        mv = D.MatvecPlan(Operator.fromSpec(plain, spec), plain_reps, torch.complex128)
        for b in range(2):
            out = torch.zeros_like(fk[b])
            mv.matvec([fk[b]], [out])
            for a in range(2):
                want = complex(torch.vdot(fb[a], out))
                worst = max(worst, abs(got[k, a, b] - want) / _atol(spec.terms))
                assert abs(got[k, a, b] - want) <= _atol(spec.terms), (sections[k], a, b, got[k, a, b], want)
    print(f"matrix_elements ring36 weight 3 k = 5 (64-bit words): {len(specs)} operators x 2 x 2 columns, worst error / tolerance {worst:.2e}")
    assert np.abs(got).max() > 1e-3 and np.abs(got[-1]).max() > 1e-3
    pl.destroy()


# ---- 11: the sum of the bonds ----------------------------------------------------------------------------------------------------------
def _heisenberg(cfg, L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    full = dict(cfg)
    full["hamiltonian"] = {"name": "Heisenberg", "terms": [{"expression": e, "sites": bonds} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}
    # S_b . S_b+1 = sigma . sigma / 4 on one bond: H = J sum_b S_b . S_b+1 with J = 4
    ops = [{"terms": [{"expression": f"0.25 × {e}", "sites": [b]} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]} for b in bonds]
    return full, ops, 4.0


def test_the_bond_operators_sum_to_the_hamiltonian(torch):
    """16-site ring, k = 3: no S_b . S_b+1 is invariant under the translations, their sum is H / J: sum_b J M_b(Phi, Psi) = Phi^+ (H Psi)
    with H Psi from MatvecPlan.matvec_block.  Tolerance: n_bonds ATOL_b for the sum, and |Phi_a| |delta| <= sqrt(n) 1e-12 max(1, max|H Psi|)
    for an H Psi within the bound of the block-matvec parity tests (1e-12 max(1, max|want|) per element)."""
    cfg, ops, J = _heisenberg(E.ring(16, 8, 3), 16)
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps_list, _ = D.enumerateStates(basis, 1)
    reps = reps_list[0]
    n = int(reps.numel())
    specs = [config.parse_operator(sec, basis.spec) for sec in ops]
    bra, ket = _columns(torch, reps, torch.complex128, BRA_SEEDS), _columns(torch, reps, torch.complex128, KET_SEEDS)
    hk = torch.zeros_like(ket)
    D.MatvecPlan(h, reps_list, torch.complex128).matvec_block(ket, hk)
    want = (bra.conj().t() @ hk).cpu().numpy()
    got = D.matrix_elements(basis, reps, bra, ket, specs)
    assert got.shape == (16, 3, 5)
    total = J * got.sum(axis=0)
    tol = 16 * J * _atol(specs[0].terms) + np.sqrt(n) * 1e-12 * max(1.0, float(hk.abs().max()))
    print(f"matrix_elements ring16 k = 3: sum of 16 bonds against Phi^+ H Psi, error {np.abs(total - want).max():.2e} (tolerance {tol:.2e})")
    assert np.abs(total - want).max() <= tol and np.abs(want).max() > 1e-2
    # (bra and ket carry the same character: the translates of a bond have the same matrix elements, each H / (16 J) of the sum)
    assert np.abs(got - got[0]).max() <= 2 * _atol(specs[0].terms)


# ---- 12: eigenstates -------------------------------------------------------------------------------------------------------------------
def test_eigenstate_matrix_elements_of_a_ring(torch):
    from distributed_matvec_amd.diagonalize import full_spectrum

    cfg, ops, J = _heisenberg(E.ring(12, 6, 1), 12)
    # (bra and ket carry the same character, so every bond has the matrix of H / (12 J), diagonal in the eigenbasis: a second-neighbour
    # S . S, which does not commute with H, brings entries off the diagonal)
    ops = ops + [{"terms": [{"expression": f"0.25 × {e}", "sites": [[0, 2]]} for e in ("σˣ₀ σˣ₁", "σʸ₀ σʸ₁", "σᶻ₀ σᶻ₁")]}]
    energies, M = eigenstate_matrix_elements(cfg, ops)
    m = len(energies)
    assert m > 64 and M.shape == (13, m, m) and M.dtype == np.complex128  # (more than one tile of 64 x 64 columns)
    spec = full_spectrum(cfg, eigenvectors=True)
    assert np.array_equal(energies, spec.eigenvalues)
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    specs = [config.parse_operator(sec, basis.spec) for sec in ops]
    tol = _atol(specs[0].terms)
    # the diagonal: expectation_values of every eigenvector
    for i in (0, 1, 63, 64, m - 1):
        one = D.expectation_values(basis, spec.representatives, spec.eigenvectors[:, i].contiguous(), specs)
        assert np.abs(M[:, i, i] - one).max() <= 2 * tol, i
    # S_b . S_b+1 is Hermitian: so is its matrix
    assert np.abs(M - np.conj(M.transpose(0, 2, 1))).max() <= 2 * tol
    # sum_b J M_b = diag(E), up to the residuals of the eigenvectors
    V = spec.eigenvectors.to(torch.complex128).contiguous()
    HV = torch.zeros_like(V)
    mv = D.MatvecPlan(h, [spec.representatives], torch.complex128)
    for c0 in range(0, m, 64):
        mv.matvec_block(V[:, c0:c0 + 64], HV[:, c0:c0 + 64])
    resid = float(torch.linalg.vector_norm(HV - V * torch.from_numpy(energies).to(V.device), dim=0).max())
    err = np.abs(J * M[:12].sum(axis=0) - np.diag(energies)).max()
    print(f"eigenstate_matrix_elements ring12 k = 1: {m} states, sum of the bonds against diag(E) {err:.2e}, largest residual {resid:.2e}")
    assert err <= 12 * J * tol + resid and np.abs(M[12] - np.diag(np.diag(M[12]))).max() > 1e-2
    # a selection
    e5, M5 = eigenstate_matrix_elements(cfg, ops, states=slice(0, 5))
    assert np.array_equal(e5, energies[:5]) and M5.shape == (13, 5, 5) and np.abs(M5 - M[:, :5, :5]).max() <= 2 * tol
    e3, M3 = eigenstate_matrix_elements(cfg, ops[:2], states=[7, 2, m - 1])
    assert np.array_equal(e3, energies[[7, 2, m - 1]]) and np.abs(M3 - M[:2][:, [7, 2, m - 1]][:, :, [7, 2, m - 1]]).max() <= 2 * tol
    with pytest.raises(ValueError, match=f"{16 * 13 * 25} bytes; max_bytes is 4000"):
        eigenstate_matrix_elements(cfg, ops, states=slice(0, 5), max_bytes=4000)
    with pytest.raises(ValueError, match=f"{16 * 13 * m * m} bytes; max_bytes is 4000"):
        eigenstate_matrix_elements(cfg, ops, max_bytes=4000)  # (a projected sector: known once its representatives are counted)
    with pytest.raises(ValueError, match="max_dim is 10"):
        eigenstate_matrix_elements(cfg, ops, max_dim=10)


# ---- 13: errors ------------------------------------------------------------------------------------------------------------------------
def test_representatives_that_are_not_the_sector_raise_the_error_flag(torch):
    """the lower half of the representatives (tests/test_gpu_expectation.py): sigma^+_11 sends each of them to a word inside the weight
    sector that is not in the array.  The plan keeps refusing; a plan over the whole sector answers afterwards."""
    sec = {"terms": [{"expression": "σ⁻₀ σ⁺₁ σᶻ₂", "sites": [[0, 11, 7]]}]}
    for cfg in (E.ring(12, 6, 0), E.ring(12, 6, None)):  # the static index table, and the searched index of an incomplete array
        basis = D.loadConfigFromDict(cfg)
        reps = D.enumerateStates(basis, 1)[0][0]
        cut = reps[: reps.numel() // 2].contiguous()
        pl = D.ExpectationPlan(basis, cut, [sec])
        bra, ket = _columns(torch, cut, torch.float64, (1, 2, 3)), _columns(torch, cut, torch.float64, (4, 5))
        for _ in range(2):
            with pytest.raises(LsAmdError, match="not in the basis"):
                pl.matrix_elements(bra, ket)
        pl.destroy()
        whole = D.ExpectationPlan(basis, reps, [sec])
        bra, ket = _columns(torch, reps, torch.float64, (1, 2, 3)), _columns(torch, reps, torch.float64, (4, 5))
        got = whole.matrix_elements(bra, ket)
        pol = whole.matrix_elements(bra, ket, method="polarisation")
        assert np.abs(got - pol).max() <= 8 * _atol(config.parse_operator(sec, basis.spec).terms) and np.abs(got).max() > 1e-3
        whole.destroy()


def test_refusals_come_back_by_name(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    basis = D.loadConfigFromDict(E.ring(12, 6, 5))  # complex characters
    reps = D.enumerateStates(basis, 1)[0][0]
    n = int(reps.numel())
    sec = {"terms": [{"expression": "σ⁺₀ σ⁻₁ σᶻ₂", "sites": [[0, 5, 7]]}]}
    pl = D.ExpectationPlan(basis, reps, [sec])
    bra, ket = _columns(torch, reps, torch.complex128, (1, 2)), _columns(torch, reps, torch.complex128, (3, 4, 5))
    out = np.zeros(2 * 2 * 3)
    f64p = C.POINTER(C.c_double)
    pb, pk, outp = C.c_void_p(bra.data_ptr()), C.c_void_p(ket.data_ptr()), out.ctypes.data_as(f64p)
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    call = L.ls_amd_expect_matrix_elements
    assert call(None, 1, 2, pb, 2, 1, 3, pk, 3, 1, outp, None) == -1 and "ls_amd_expect_matrix_elements: NULL plan" in err()
    assert call(pl.h, 1, 2, None, 2, 1, 3, pk, 3, 1, outp, None) == -1 and "NULL bra block" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, None, 3, 1, outp, None) == -1 and "NULL ket block" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, pk, 3, 1, None, None) == -1 and "NULL output" in err()
    assert call(pl.h, 1, 0, pb, 2, 1, 3, pk, 3, 1, outp, None) == -1 and "ls_amd_expect_matrix_elements: Ka = 0 is outside [1, 64]" in err()
    assert call(pl.h, 1, 65, pb, 65, 1, 3, pk, 3, 1, outp, None) == -1 and "Ka = 65 is outside [1, 64]" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 0, pk, 3, 1, outp, None) == -1 and "Kb = 0 is outside [1, 64]" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 65, pk, 65, 1, outp, None) == -1 and "Kb = 65 is outside [1, 64]" in err()
    assert call(pl.h, 7, 2, pb, 2, 1, 3, pk, 3, 1, outp, None) == -1 and "unknown dtype 7" in err()
    assert call(pl.h, 0, 2, pb, 2, 1, 3, pk, 3, 1, outp, None) == -1
    assert "ls_amd_expect_matrix_elements: f64 needs +-1 characters (complex characters: use c128)" in err()
    assert call(pl.h, 1, 2, pb, 0, 1, 3, pk, 3, 1, outp, None) == -1 and "of the bra block must be positive" in err()
    assert call(pl.h, 1, 2, pb, 2, 0, 3, pk, 3, 1, outp, None) == -1 and "of the bra block must be positive" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, pk, -3, 1, outp, None) == -1 and "of the ket block must be positive" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, pk, 3, 0, outp, None) == -1 and "of the ket block must be positive" in err()
    assert call(pl.h, 1, 2, pb, 1, 1, 3, pk, 3, 1, outp, None) == -1 and "of the bra block make two elements" in err() and "share storage" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, pk, 2, 1, outp, None) == -1 and "of the ket block make two elements" in err() and "share storage" in err()
    assert L.ls_amd_expect_matrix_kernel_name(pl.h, 65, 1) is None and "within [1, 64]" in err()
    assert L.ls_amd_expect_matrix_kernel_name(pl.h, 1, 0) is None and "within [1, 64]" in err()
    assert L.ls_amd_expect_matrix_kernel_name(None, 1, 1) is None and "NULL plan" in err()
    assert call(pl.h, 1, 2, pb, 2, 1, 3, pk, 3, 1, outp, None) == 0  # (and the good call goes through)
    assert np.array_equal(out.view(np.complex128).reshape(2, 3), pl.matrix_elements(bra, ket)[0])
    # bra and ket may be the same memory, or overlap
    assert call(pl.h, 1, 2, pk, 3, 1, 2, C.c_void_p(ket.data_ptr() + 16), 3, 1, outp, None) == 0
    assert np.array_equal(out.view(np.complex128)[:4].reshape(2, 2), pl.matrix_elements(ket[:, :2], ket[:, 1:])[0])
    # a vector is one column
    assert pl.matrix_elements(bra[:, 0], ket).shape == (1, 1, 3) and pl.matrix_elements(bra[:, 1]).shape == (1, 1, 1)
    assert np.array_equal(pl.matrix_elements(bra[:, 1], ket)[0, 0], pl.matrix_elements(bra, ket)[0, 1])
    # an expanded view is made contiguous
    assert np.array_equal(pl.matrix_elements(bra[:, :1].expand(n, 2), ket)[0, 1], pl.matrix_elements(bra, ket)[0, 0])
    with pytest.raises(LsAmdError, match=r"bra \(.*\) must be a vector \(n,\) or a 2-D block \(n, K\)"):
        pl.matrix_elements(bra.unsqueeze(0), ket)
    with pytest.raises(LsAmdError, match=r"ket has K = 65 columns, outside \[1, 64\]"):
        pl.matrix_elements(bra, torch.zeros((n, 65), dtype=torch.complex128, device=bra.device))
    with pytest.raises(LsAmdError, match=r"bra has K = 65 columns, outside \[1, 64\]"):
        pl.matrix_elements(torch.zeros((n, 65), dtype=torch.complex128, device=bra.device))
    with pytest.raises(LsAmdError, match=f"bra .* must have {n} rows"):
        pl.matrix_elements(bra[:-1], ket)
    with pytest.raises(LsAmdError, match=f"ket .* must have {n} rows"):
        pl.matrix_elements(bra, ket[:-1])
    with pytest.raises(LsAmdError, match="ket must be a device tensor"):
        pl.matrix_elements(bra, ket.cpu())
    with pytest.raises(LsAmdError, match="bra is torch.complex64, neither float64 nor complex128"):
        pl.matrix_elements(bra.to(torch.complex64), ket)
    with pytest.raises(LsAmdError, match="method 'fast'"):
        pl.matrix_elements(bra, ket, method="fast")
    with pytest.raises(LsAmdError, match="method 'fast'"):
        pl.matrix_kernel(2, 3, method="fast")
    with pytest.raises(LsAmdError, match=r"within \[1, 64\]"):
        pl.matrix_kernel(0, 3)
    pl.destroy()
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.matrix_elements(bra, ket)
    with pytest.raises(LsAmdError, match="destroyed"):
        pl.matrix_kernel(2, 3)


def test_matrix_elements_normalises_every_column(torch):
    basis, reps, _bra, _ket, specs, _sections, _want = _case("torus_4x3_f64")
    bra, ket = _columns(torch, reps, torch.float64, (3, 4), normalise=False), _columns(torch, reps, torch.float64, (5, 6, 7), normalise=False)
    got = matrix_elements(basis, reps, bra, ket, specs)
    pl = D.ExpectationPlan(basis, reps, specs)
    want = pl.matrix_elements(bra / torch.linalg.vector_norm(bra, dim=0), ket / torch.linalg.vector_norm(ket, dim=0))
    assert got.shape == (len(specs), 2, 3) and (np.abs(got - want) <= 2 * _tols(specs)).all() and np.abs(got).max() > 1e-3
    same = matrix_elements(basis, reps, ket, None, specs)
    assert np.abs(np.stack([same[:, c, c] for c in range(3)], axis=1) - D.expectation_values_block(basis, reps, ket, specs)).max() <= 2 * _tols(specs).max()
    pl.destroy()
