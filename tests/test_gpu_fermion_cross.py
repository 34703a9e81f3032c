"""Cross-sector operators between projected fermionic bases on the GPU (CrossSectorPlan on k_cross_pull_fermi): y = A x for c+_q,
c_q, n_q and S^z_q between momentum, point-group and spin-flip sectors of spinless and spinful bases against B2^+ A B1 from the
signed projectors and the Jordan-Wigner matrix of tests/fermion_cross_reference.py (nothing of this library), the adjoint run as
its own plan in the reverse direction, free fermions on a ring -- where c+_k on the Fermi sea has an exact norm and energy --,
kpm.spectral_function(..., target=...) against an eigendecomposition of the projected target matrix, and the failures that must be
loud."""
import math

import numpy as np
import pytest

import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_jw as J
import fermion_symm as F
from distributed_matvec_amd import config, kpm
from distributed_matvec_amd.diagonalize import LocalOperator, lanczos_smallest
from helpers import product_terms
from kpm_reference import exact_moments, moment_tolerance

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _dtype(torch, name):
    return torch.complex128 if name == "c128" else torch.float64


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _setup(src, dst, model):
    """(source Basis, Operator on it, source reps, target Basis, target reps) of two sectors (fermion_cross_reference.sector)"""
    spinful = src["n_up"] is not None
    sbasis = D.loadConfigFromDict(R.basis_config(src))
    A = D.Operator.fromSpec(sbasis, config.parse_operator(R.operator_section(model, spinful), sbasis.spec))
    tbasis = D.loadConfigFromDict(R.basis_config(dst))
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    return sbasis, A, sreps[0], tbasis, treps[0]


def _compare(got, want, scale, what):
    """the bound of test_gpu_cross_sector._compare: |got - want| <= max(1e-13 sum_j |c_j| max|x|, 1e-12 max(|got|, |want|))"""
    tol = np.maximum(1e-13 * scale, 1e-12 * np.maximum(np.abs(got), np.abs(want)))
    err = np.abs(got - want)
    print(f"fermionic cross-sector {what}: rows {len(want)}, max |y| {np.abs(want).max():.3e}, max error {err.max():.3e}, smallest tolerance {tol.min():.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), (what, err.max(), tol.min())


RUNS = [(name, dt) for name in sorted(R.CASES) for dt in R.CASES[name][4]]


@pytest.mark.parametrize("name,dt", RUNS)
def test_cross_apply_matches_the_signed_projectors(torch, name, dt):
    src, dst, model, _, _, (n_src, n_dst, zero) = R.CASES[name]
    ref = R.case_reference(name)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, model)
    assert sbasis.hasFermionSigns() and tbasis.hasFermionSigns()
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert (len(ref["src"]), len(ref["dst"])) == (n_src, n_dst)
    mat = ref["matrix"]
    # nothing passes vacuously: entries of both signs, and the zero-norm images of the table are there to be dropped
    assert np.count_nonzero(np.abs(mat) > 1e-9) > 0 and (mat.real < -1e-9).any() and (mat.real > 1e-9).any() and ref["images"] > 0
    assert ref["leak"] <= 4e-14
    if zero == "> 0":
        assert ref["pull_dropped"] > 0
    elif zero is not None:
        assert ref["pull_dropped"] == zero
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    assert plan.kernel == "k_cross_pull_fermi"
    assert plan.nnz == ref["images"], (plan.nnz, ref["images"], ref["pull_dropped"])
    x = D.fillRandom(sreps, 7, dtype)
    y = torch.full((len(ref["dst"]),), float("nan"), dtype=dtype, device=x.device)
    plan.apply(x, y)
    want = mat @ x.cpu().numpy()
    if dt == "f64":
        assert np.abs(mat.imag).max() <= 1e-14
        want = want.real
    _compare(y.cpu().numpy(), want, R.coefficient_sum(model) * float(x.abs().max()), f"{name} {dt}")
    plan.destroy()


def _on_basis(basis, op):
    """the terms of `op` compiled on another basis"""
    diag, off = product_terms(op)
    return D.Operator.fromSpec(basis, config.OperatorSpec(diag + off))


@pytest.mark.parametrize("name", ["L8_cdag_q2", "L12_cdag_q5", "L34_cdag_q5", "spinful_L6_cdag_q2_up", "spinful_L6_sz_q2"])
def test_adjoint_plan_is_consistent_on_the_device(torch, name):
    """<y2|A x1> = conj <x1|A+ y2>, with A+ run as its own plan from the target back to the source.  Every monomial has norm <= 1,
    so both sides are sums bounded by sum_j |c_j| ||x1|| ||y2||; 1e-12 of that bound is ~4500 eps for a few hundred partners."""
    src, dst, model, _, _, _ = R.CASES[name]
    dtype = torch.complex128
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, model)
    Ad = _on_basis(tbasis, A.adjoint())
    assert Ad.mapsSector(sbasis, explain=True, signs=True)
    fwd = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    back = D.CrossSectorPlan(Ad, treps, sbasis, sreps, dtype)
    assert fwd.kernel == back.kernel == "k_cross_pull_fermi"
    x1, y2 = D.fillRandom(sreps, 11, dtype), D.fillRandom(treps, 12, dtype)
    Ax = torch.full_like(y2, float("nan"))
    Ady = torch.full_like(x1, float("nan"))
    fwd.apply(x1, Ax)
    back.apply(y2, Ady)
    lhs, rhs = complex(torch.vdot(y2, Ax)), complex(torch.vdot(x1, Ady)).conjugate()
    bound = R.coefficient_sum(model) * float(torch.linalg.vector_norm(x1)) * float(torch.linalg.vector_norm(y2))
    print(f"adjoint consistency {name}: <y2|A x1> = {lhs:.16g}, conj <x1|A+ y2> = {rhs:.16g}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * bound


def test_creation_operators_on_the_free_fermi_sea(torch):
    """t-V ring at V = 0, L = 12, N = 5: the ground state is the Fermi sea of the momenta 0, +-1, +-2 (non-degenerate, total
    momentum 0).  c+_k = L^-1/2 sum_j e^{-2 pi i k j / L} c+_j gives 0 on an occupied momentum and a normalised eigenstate of
    energy E0 - 2 t cos(2 pi k / L) in the N = 6 sector of momentum k otherwise; the norms sum to L - N.  1e-8: the eigensolver's
    eps = 1e-10 with margin (the bound of the Bethe-ansatz tests)."""
    L, N, tol = 12, 5, 1e-8
    dtype = torch.complex128
    energies = [F.free_ring_energy(L, N, s) for s in range(L)]
    E0 = min(energies)
    s0 = int(np.argmin(energies))
    assert sum(1 for e in energies if e <= E0 + 1e-9) == 1  # non-degenerate: one momentum sector holds it
    single = sorted(range(L), key=lambda m: -2.0 * math.cos(2.0 * math.pi * m / L))
    occupied = set(single[:N])
    assert abs(sum(-2.0 * math.cos(2.0 * math.pi * m / L) for m in occupied) - E0) <= 1e-12 and sum(occupied) % L == s0
    model_h = F.tv_model(J.ring(L))
    src = R.sector(L, N, F.translations(L), [s0])
    cfg = dict(R.basis_config(src), hamiltonian={"terms": J.yaml_terms(model_h, False)})
    sbasis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    sreps, _ = D.enumerateStates(sbasis, 1)
    res = lanczos_smallest(LocalOperator(h, sreps, dtype), num_evals=1, eps=1e-10)
    assert abs(res.eigenvalues[0] - E0) <= tol
    psi = res.eigenvectors[0].to(dtype).contiguous()
    psi = psi / torch.linalg.vector_norm(psi)
    norms = []
    for dk in range(L):
        dst = R.sector(L, N + 1, F.translations(L), [(s0 + dk) % L])
        model = [(c / math.sqrt(L), ops) for c, ops in R.c_dag(L, dk)]
        A = D.Operator.fromSpec(sbasis, config.parse_operator(R.operator_section(model, False), sbasis.spec))
        tcfg = dict(R.basis_config(dst), hamiltonian={"terms": J.yaml_terms(model_h, False)})
        tbasis, h_t = D.loadConfigFromDict(tcfg, hamiltonian=True)
        treps, _ = D.enumerateStates(tbasis, 1)
        plan = D.CrossSectorPlan(A, sreps[0], tbasis, treps[0], dtype)
        assert plan.kernel == "k_cross_pull_fermi"
        v = torch.full((treps[0].numel(),), float("nan"), dtype=dtype, device=psi.device)
        plan.apply(psi, v)
        plan.destroy()
        n2 = float(torch.vdot(v, v).real)
        norms.append(n2)
        if dk in occupied:
            assert n2 <= tol, (dk, n2)
            continue
        assert abs(n2 - 1.0) <= tol, (dk, n2)
        w = torch.zeros_like(v)
        D.MatvecPlan(h_t, treps, dtype).matvec([v], [w])
        e = float(torch.vdot(v, w).real) / n2
        want = E0 - 2.0 * math.cos(2.0 * math.pi * dk / L)
        print(f"free fermions: c+_{dk} on the Fermi sea: norm^2 {n2:.12f}, energy {e:.12f}, exact {want:.12f}")
        assert abs(e - want) <= tol, (dk, e, want)
    print("free fermions: norms", " ".join(f"{n:.3e}" for n in norms))
    assert abs(sum(norms) - (L - N)) <= tol


def test_spectral_function_into_another_fermionic_sector(torch):
    """A(k, w) of the 8-site t-V ring with V = 1: a state of the N = 3, k = 0 sector, c+_q with q = 3 into N = 4, k = 3; moments
    against the eigendecomposition of the reference's projected target matrix with v0 = (reference matrix) psi"""
    L, M_ = 8, 64
    src, dst, model, _, _, _ = R.CASES["L8_cdag_q3"]
    model_h = F.tv_model(J.ring(L), V=1.0)
    cfg = dict(R.basis_config(src), hamiltonian={"terms": J.yaml_terms(model_h, False)}, observables=[R.operator_section(model, False)])
    ref = R.case_reference("L8_cdag_q3")
    grp = F.closure(L, dst["gens"], dst["secs"])
    H = F.projected_matrix(model_h, L, dst["N"], grp, ref["dst"])
    assert np.abs(H - H.conj().T).max() <= 1e-13
    evals, U = np.linalg.eigh(H)
    w = evals[-1] - evals[0]
    bounds = (float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w))
    sbasis = D.loadConfigFromDict(R.basis_config(src))
    sreps, _ = D.enumerateStates(sbasis, 1)
    state = D.fillRandom(sreps[0], 9, torch.complex128)
    state = state / torch.linalg.vector_norm(state)
    E, S, res = kpm.spectral_function(cfg, 0, state=state, num_moments=M_, bounds=bounds, dtype=torch.complex128, target=R.basis_config(dst))
    v0 = ref["matrix"] @ state.cpu().numpy()
    assert res.target_state is not None and res.target_state.shape == (len(ref["dst"]),)
    assert np.abs(res.target_state.cpu().numpy() - v0).max() <= 1e-12 * max(1.0, np.abs(v0).max())
    mu = res.moments
    assert mu.shape == (1, M_) and mu[0, 0] > 0.1
    weights = (np.abs(U.conj().T @ v0.reshape(-1, 1)) ** 2).T
    exact = exact_moments(evals, weights, M_, bounds)
    tol, own = moment_tolerance(H, v0.reshape(-1, 1), M_, bounds, exact)
    dev = np.abs(mu - exact).max(axis=1)
    print(f"A(k, w) moments N 3 -> 4, k 0 -> 3: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}, mu_0 {exact[0, 0]:.6g}")
    assert (dev <= tol).all(), (dev, tol)
    assert E.shape == S.shape == (2 * M_,)


# ---- failures that must be loud ------------------------------------------------------------------------------------------------
def test_a_wrong_sector_is_refused_at_plan_creation(torch):
    src, dst, _, _, _, _ = R.CASES["L8_cdag_q3"]
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, R.wrong_dk_model("L8_cdag_q3"))
    with pytest.raises(D.LsAmdError, match="generator 0"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128)
    src, dst, model, _, _, _ = R.CASES["L8_dihedral_cdag_q0"]
    sbasis, A, sreps, tbasis, treps = _setup(src, dict(dst, secs=[0, 1]), model)
    with pytest.raises(D.LsAmdError, match="generator 1"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64)


def test_f64_with_complex_characters_is_refused(torch):
    # a real operator (sum_j c+_j), but k = 1 on both sides: complex characters
    sbasis, A, sreps, tbasis, treps = _setup(R.sector(8, 3, F.translations(8), [1]), R.sector(8, 4, F.translations(8), [1]), R.c_dag(8, 0))
    assert A.isReal
    with pytest.raises(D.LsAmdError, match="c128"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64)
    D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128).destroy()
    # +-1 characters on both sides, complex coefficients
    src, dst, model, _, _, _ = R.CASES["L8_cdag_q4"]
    sbasis, B, sreps, tbasis, treps = _setup(src, dst, [(1j * complex(c), ops) for c, ops in model])
    with pytest.raises(D.LsAmdError, match="c128"):
        D.CrossSectorPlan(B, sreps, tbasis, treps, torch.float64)


def test_an_operator_that_leaves_the_source_basis_raises_from_check(torch):
    """c+_q handed a target with TWO particles more: the covariance rule does not examine particle numbers, the kernel finds that
    the adjoint's images are not in the source basis, raises its flag, and check() reports it"""
    src, dst, model, _, _, _ = R.CASES["L8_cdag_q3"]
    sbasis, A, sreps, tbasis, treps = _setup(src, dict(dst, N=5), model)
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128)
    assert plan.nnz == 0
    x = D.fillRandom(sreps, 1, torch.complex128)
    y = torch.zeros(treps.numel(), dtype=torch.complex128, device=x.device)
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.apply(x, y)
    plan.apply(x, y, check=False)
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.check()
    plan.check()  # reported once
