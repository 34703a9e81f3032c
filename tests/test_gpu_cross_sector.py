"""Cross-sector operators on the GPU: y = A x between two symmetry sectors (CrossSectorPlan, k_cross_pull) against reference
matrices that use nothing of this library (tests/cross_sector_reference.py: explicit projectors up to 12 sites, the push formula
with oracle.model.state_info at 16; a dense Jordan-Wigner matrix for fermions), the adjoint run as its own plan, the sum rule of
S^z_q over all momenta, kpm.spectral_function(..., target=...) against an eigendecomposition of the target sector, and the
failures that must be loud."""
import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_jw
from distributed_matvec_amd import CrossSectorPlan  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config, kpm
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


def _setup(src_cfg, dst_cfg, op_cfg):
    """(source Basis, Operator on it, source reps, target Basis, target reps): device tensors of the representatives"""
    sbasis = D.loadConfigFromDict(src_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    tbasis = D.loadConfigFromDict(dst_cfg)
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    return sbasis, A, sreps[0], tbasis, treps[0]


def _compare(got, want, scale, what):
    """|got - want| <= max(1e-13 sum_j |c_j| max|x|, 1e-12 max(|got|, |want|)): the first term is ~450 eps times the largest
    possible row sum, which covers any summation order of up to a few hundred partners"""
    tol = np.maximum(1e-13 * scale, 1e-12 * np.maximum(np.abs(got), np.abs(want)))
    err = np.abs(got - want)
    print(f"cross-sector {what}: rows {len(want)}, max |y| {np.abs(want).max():.3e}, max error {err.max():.3e}, smallest tolerance {tol.min():.3e}")
    assert np.isfinite(got).all() and (err <= tol).all(), (what, err.max(), tol.min())


EXPECTED_ROWS = {"L8_sz_k0_k3": (10, 8), "L8_dihedral_staggered": (7, 4), "L12_w6_w5_f64": (924, 792), "L12_w6_w5_c128": (924, 792),
                 "L12_identity_index": (4096, 4096), "L16_sz_k0_k5": (810, 800), "L16_splus_w8_w7_k0_k5": (810, 715)}


@pytest.mark.parametrize("name", sorted(X.ALL_CASES))
def test_cross_apply_matches_the_reference_matrix(torch, name):
    src, dst, op, dt = X.ALL_CASES[name]
    ref = X.case_formula(name)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    if name in EXPECTED_ROWS:
        assert (len(ref["src"]), len(ref["dst"])) == EXPECTED_ROWS[name]
    mat = ref["matrix"]
    assert np.count_nonzero(np.abs(mat) > 1e-9) > 0 and ref["images"] > 0  # nothing passes vacuously
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    assert plan.kernel == "k_cross_pull"
    assert plan.nnz == ref["images"], (plan.nnz, ref["images"], ref["pull_dropped"])
    x = D.fillRandom(sreps, 7, dtype)
    y = torch.full((len(ref["dst"]),), float("nan"), dtype=dtype, device=x.device)
    plan.apply(x, y)
    want = mat @ x.cpu().numpy()
    if dt == "f64":
        assert np.abs(mat.imag).max() <= 1e-14
        want = want.real
    _compare(y.cpu().numpy(), want, X.coefficient_sum(op) * float(x.abs().max()), name)
    # a block of columns is a loop over them
    xb = torch.stack([x, 2.0 * x], dim=1)
    yb = torch.zeros((len(ref["dst"]), 2), dtype=dtype, device=x.device)
    plan.apply(xb, yb)
    scale = X.coefficient_sum(op) * float(x.abs().max())
    _compare(yb[:, 0].cpu().numpy(), want, scale, name + " column 0")  # (the order of the LDS adds is not fixed: no bitwise equality)
    _compare(yb[:, 1].cpu().numpy(), 2.0 * want, 2.0 * scale, name + " column 1")
    plan.destroy()


def test_zero_norm_images_are_met():
    """at least two cases drop images whose orbit has zero norm in the target sector (2 and 3 of them by the numpy projectors),
    and one meets, in the pull form the kernel runs, coefficients whose column state has no norm in the SOURCE sector"""
    dropped = {name: X.case_formula(name)["dropped"] for name in X.CASES}
    assert dropped["L8_sz_k0_k3"] == 2 and dropped["L8_dihedral_staggered"] == 3
    assert sum(1 for v in dropped.values() if v > 0) >= 2
    assert X.case_formula("L8_splus_w4_w3_k1_k4")["pull_dropped"] > 0


def test_spinful_fermion_creation_operator(torch):
    """c+_{2 up} from (N, N_up) = (6, 3) to (7, 4) on 6 sites against the dense Jordan-Wigner matrix: no group, the product index,
    the signs in the terms' sign masks"""
    L = 6
    model = [(1.0, [("+", 2, 0)])]
    src = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 6, "number_up": 3}}
    dst = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": 7, "number_up": 4}}
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, {"terms": fermion_jw.yaml_terms(model, True)})
    cols, rows = fermion_jw.product_states(L, 3, 3), fermion_jw.product_states(L, 4, 3)
    assert np.array_equal(_u64(sreps), cols) and np.array_equal(_u64(treps), rows)
    full = fermion_jw.dense(model, L, True).tocsr()
    mat = np.asarray(full[rows.astype(np.int64)][:, cols.astype(np.int64)].todense())
    assert np.count_nonzero(mat) > 0 and (mat.real < 0).any() and (mat.real > 0).any()
    for dt in ("f64", "c128"):
        dtype = _dtype(torch, dt)
        plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
        assert plan.nnz == np.count_nonzero(mat)  # one flip mask: an image per non-zero entry
        x = D.fillRandom(sreps, 3, dtype)
        y = torch.full((len(rows),), float("nan"), dtype=dtype, device=x.device)
        plan.apply(x, y)
        want = mat @ x.cpu().numpy()
        _compare(y.cpu().numpy(), want.real if dt == "f64" else want, float(x.abs().max()), "c+_2up (6,3)->(7,4) " + dt)


def _on_basis(basis, op):
    """the terms of `op` compiled on another basis"""
    diag, off = product_terms(op)
    return D.Operator.fromSpec(basis, config.OperatorSpec(diag + off))


@pytest.mark.parametrize("name", ["L16_sz_k0_k5", "L16_splus_w8_w7_k0_k5", "L8_splus_w4_w3_k1_k4"])
def test_adjoint_plan_is_consistent_on_the_device(torch, name):
    """<y2|A x1> = conj <A+ y2|x1>, with A+ run as its own cross plan from the target back to the source"""
    src, dst, op, dt = X.ALL_CASES[name]
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    Ad = _on_basis(tbasis, A.adjoint())
    assert Ad.mapsSector(sbasis, explain=True)
    fwd = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    back = D.CrossSectorPlan(Ad, treps, sbasis, sreps, dtype)
    x1, y2 = D.fillRandom(sreps, 11, dtype), D.fillRandom(treps, 12, dtype)
    Ax = torch.zeros_like(y2)
    Ady = torch.zeros_like(x1)
    fwd.apply(x1, Ax)
    back.apply(y2, Ady)
    lhs, rhs = complex(torch.vdot(y2, Ax)), complex(torch.vdot(Ady, x1))  # <A+ y2|x1> = <y2|A x1>
    print(f"adjoint consistency {name}: <y2|A x1> = {lhs:.16g}, <A+ y2|x1> = {rhs:.16g}, difference {abs(lhs - rhs):.3e}")
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * abs(lhs)


def test_sum_rule_over_all_momenta(torch):
    """sum_q ||S^z_q psi||^2 = L^2 for a normalised psi (sum_q A_q^+ A_q = L sum_j (sigma^z_j)^2), and the q = 0 term vanishes at
    half filling: a pin that owes nothing to this repository's references"""
    L = 12
    src = X.ring(L, L // 2, 0)
    sbasis = D.loadConfigFromDict(src)
    sreps, _ = D.enumerateStates(sbasis, 1)
    psi = D.fillRandom(sreps[0], 5, torch.complex128)
    psi = psi / torch.linalg.vector_norm(psi)
    mu0 = []
    for q in range(L):
        A = D.Operator.fromSpec(sbasis, config.parse_operator(X.sz_q(L, q), sbasis.spec))
        tbasis = D.loadConfigFromDict(X.ring(L, L // 2, q))
        treps, _ = D.enumerateStates(tbasis, 1)
        plan = D.CrossSectorPlan(A, sreps[0], tbasis, treps[0], torch.complex128)
        v = torch.zeros(treps[0].numel(), dtype=torch.complex128, device=psi.device)
        plan.apply(psi, v)
        mu0.append(float(torch.vdot(v, v).real))
        plan.destroy()
    print("sum rule: mu_0(q) =", " ".join(f"{m:.12g}" for m in mu0), " sum =", repr(sum(mu0)))
    assert abs(sum(mu0) - L * L) <= 1e-10
    assert abs(mu0[0]) <= 1e-12
    assert max(mu0) > 1.0


def _heisenberg(basis_cfg, L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "Heisenberg", "terms": [
        {"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}


def test_spectral_function_into_another_momentum_sector(torch):
    """S(q, w) of the 12-site ring: ground state in k = 0, S^z_q with q = 5 into k = 5; moments against the eigendecomposition of the
    dense k = 5 sector matrix with v0 = (reference matrix) psi"""
    from oracle import model as M

    L, M_ = 12, 256
    src, dst, op = X.ring(L, 6, 0), X.ring(L, 6, 5), X.sz_q(L, 5)
    cfg = _heisenberg(src, L)
    cfg["observables"] = [op]
    reps_t, H = M.dense_sector_matrix(_heisenberg(dst, L))
    H = np.asarray(H)
    evals, U = np.linalg.eigh(H)
    w = evals[-1] - evals[0]
    bounds = (float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w))
    E, S, res = kpm.spectral_function(cfg, 0, num_moments=M_, bounds=bounds, dtype=torch.complex128, target=dst)
    ref = X.formula_matrix(src, dst, op)
    assert np.array_equal(ref["dst"], np.asarray(reps_t, dtype=np.uint64))
    psi = res.state.cpu().numpy()
    v0 = ref["matrix"] @ psi
    assert res.target_state is not None and res.target_state.shape == (len(reps_t),)
    assert np.abs(res.target_state.cpu().numpy() - v0).max() <= 1e-12 * max(1.0, np.abs(v0).max())
    mu = res.moments
    assert mu.shape == (1, M_) and mu[0, 0] > 0.1
    weights = (np.abs(U.conj().T @ v0.reshape(-1, 1)) ** 2).T
    exact = exact_moments(evals, weights, M_, bounds)
    tol, own = moment_tolerance(H, v0.reshape(-1, 1), M_, bounds, exact)
    dev = np.abs(mu - exact).max(axis=1)
    print(f"S(q, w) moments k 0 -> 5: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}, mu_0 {exact[0, 0]:.6g}")
    assert (dev <= tol).all(), (dev, tol)
    assert E.shape == S.shape == (2 * M_,) and (S >= 0.0).all()
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    theta = np.arccos((E - b) / a)
    integral = np.sum(S * a * np.sin(theta)) * np.pi / len(E)  # Gauss-Chebyshev on the default grid
    assert abs(integral - mu[0, 0]) <= 1e-6
    # a whole config as the target is the same sector
    _, _, res2 = kpm.spectral_function(cfg, 0, state=res.state, num_moments=32, bounds=bounds, dtype=torch.complex128, target=_heisenberg(dst, L))
    assert np.abs(res2.moments[0] - mu[0, :32]).max() <= 1e-12 * mu[0, 0]


def test_spectral_function_without_a_target_is_todays_path(torch):
    """target=None with a sector-preserving observable: the moments of the recipe the function has always run (MatvecPlan of A,
    then chebyshev_moments on the config's own Hamiltonian), to 1e-12 -- and the same through a cross plan into the same sector"""
    from distributed_matvec_amd.diagonalize import LocalOperator

    L = 12
    src = X.ring(L, 6, 0)
    cfg = _heisenberg(src, L)
    cfg["observables"] = [{"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[i, (i + 1) % L] for i in range(L)]}]}]
    bounds = (-30.0, 20.0)  # |H| <= 3 L = 36 bonds' worth is far off; the ring's spectrum is [-21.6, 12]
    basis, h, obs = D.loadConfigFromDict(cfg, hamiltonian=True, observables=True)
    reps, _ = D.enumerateStates(basis, 1)
    state = D.fillRandom(reps[0], 9, torch.float64)
    state = state / torch.linalg.vector_norm(state)
    _, _, res = kpm.spectral_function(cfg, 0, state=state, num_moments=64, bounds=bounds)
    assert res.target_state is None
    op = LocalOperator(h, reps, torch.float64)
    v0 = torch.zeros_like(state)
    D.MatvecPlan(obs[0], reps, torch.float64).matvec([state], [v0])
    want = kpm.chebyshev_moments(op, v0.reshape(-1, 1), 64, bounds)
    assert want[0, 0] > 0.1 and np.abs(res.moments - want).max() <= 1e-12 * want[0, 0]
    _, _, res_t = kpm.spectral_function(cfg, 0, state=state, num_moments=64, bounds=bounds, target=src)
    assert np.abs(res_t.moments - want).max() <= 1e-12 * want[0, 0]
    assert torch.allclose(res_t.target_state, v0, rtol=0, atol=1e-12 * float(v0.abs().max()))


# ---- failures that must be loud ------------------------------------------------------------------------------------------------
def test_non_covariant_operator_is_refused_at_plan_creation(torch):
    sbasis, A, sreps, tbasis, treps = _setup(X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 2))
    with pytest.raises(D.LsAmdError, match="generator 0"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128)


def test_f64_with_complex_characters_is_refused(torch):
    sbasis, A, sreps, tbasis, treps = _setup(X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 3))
    with pytest.raises(D.LsAmdError, match="c128"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64)
    # +-1 characters on both sides and real coefficients (k 0 -> 4 by the staggered field): admitted
    sbasis, A, sreps, tbasis, treps = _setup(X.ring(8, 4, 0), X.ring(8, 4, 4), X.staggered_z(8))
    D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64).destroy()
    # ... the same characters, but complex coefficients
    _, B, _, _, _ = _setup(X.ring(8, 4, 0), X.ring(8, 4, 0), {"terms": [{"expression": "(0.0+1.0j) σᶻ₀", "sites": [[j] for j in range(8)]}]})
    basis0 = D.loadConfigFromDict(X.ring(8, 4, 0))
    reps0, _ = D.enumerateStates(basis0, 1)
    with pytest.raises(D.LsAmdError, match="c128"):
        D.CrossSectorPlan(B, reps0[0], basis0, reps0[0], torch.float64)


def test_wrong_shapes_and_dtypes_are_refused(torch):
    sbasis, A, sreps, tbasis, treps = _setup(X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 3))
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128)
    n1, n2 = sreps.numel(), treps.numel()
    assert (n1, n2) == (10, 8)
    mk = lambda n, dt=torch.complex128: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises(D.LsAmdError, match="x .* must have 10 rows"):
        plan.apply(mk(n2), mk(n2))
    with pytest.raises(D.LsAmdError, match="y .* must have 8 rows"):
        plan.apply(mk(n1), mk(n1))
    with pytest.raises(D.LsAmdError, match="x is torch.float64"):
        plan.apply(mk(n1, torch.float64), mk(n2))
    with pytest.raises(D.LsAmdError, match="y is torch.float64"):
        plan.apply(mk(n1), mk(n2, torch.float64))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        plan.apply(torch.zeros(n1, dtype=torch.complex128), mk(n2))
    with pytest.raises(D.LsAmdError, match="both be vectors or both have K columns"):
        plan.apply(torch.zeros((n1, 2), dtype=torch.complex128, device="cuda"), mk(n2))
    with pytest.raises(D.LsAmdError, match="int64"):
        D.CrossSectorPlan(A, sreps.to(torch.int32), tbasis, treps, torch.complex128)


def test_an_operator_that_leaves_the_source_basis_raises_from_check(torch):
    """sigma^+_0 handed a target of the SAME weight: there is no group, so the covariance check has nothing to object to; the
    kernel finds that the adjoint's images are not in the source basis, raises its flag, and check() reports it"""
    plain = {"basis": {"number_spins": 12, "hamming_weight": 6, "symmetries": []}}
    sbasis, A, sreps, tbasis, treps = _setup(plain, plain, {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}]})
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64)
    assert plan.nnz == 0
    x = D.fillRandom(sreps, 1, torch.float64)
    y = torch.zeros(treps.numel(), dtype=torch.float64, device=x.device)
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.apply(x, y)
    plan.apply(x, y, check=False)  # the flag is read back by check(), whenever that is called
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.check()
    plan.check()  # reported once
