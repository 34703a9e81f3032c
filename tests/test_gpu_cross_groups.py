"""Cross-sector operators between bases with DIFFERENT symmetry groups on the GPU (CrossSectorPlan(groups="restrict" | "project"),
k_cross_pull and k_cross_project): against the dense B2^+ A B1 of tests/cross_sector_reference.py and
tests/fermion_cross_reference.py up to 12 sites or modes, and above that against the library's own composition
project(target) o MatvecPlan(A on the plain basis) o unproject(source), every piece of which has its own tests.  The tolerance is
the derived one of tests/cross_groups_reference.py; every comparison prints its worst error / tolerance."""
import numpy as np
import pytest

import cross_groups_reference as G
import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_symm as F
from distributed_matvec_amd import config, kpm
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


def _apply(torch, plan, x, n):
    y = torch.full((n,), float("nan"), dtype=x.dtype, device=x.device)
    plan.apply(x, y)
    return y


def _against_dense(torch, src, dst, op, dt, groups, seed=7):
    """one plan against the dense reference: (plan, x, y, reference); the representatives, the kernel name and the bound are checked"""
    ref = G.dense(src, dst, op)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3  # nothing passes vacuously
    dtype = _dtype(torch, dt)
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype, groups=groups)
    assert plan.kernel == ("k_cross_project" if groups == "project" else "k_cross_pull")
    x = D.fillRandom(sreps, seed, dtype)
    y = _apply(torch, plan, x, len(ref["dst"]))
    want = ref["matrix"] @ x.cpu().numpy()
    if dt == "f64":
        assert np.abs(ref["matrix"].imag).max() <= 1e-14
        want = want.real
    S = G.monomials(op) * (G.group_order(dst) if groups == "project" else 1)
    scale = G.row_scale(X.coefficient_sum(op), ref["n2"], x.abs().max())
    G.compare(y.cpu().numpy(), want, S, scale, f"{groups} {dt} rows {len(ref['dst'])}")
    return plan, x, y, ref


DIHEDRAL12 = G.ring(12, 6, 0, 0, 1)


# ---- 1-4: groups="restrict" ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dk", [1, 5])
def test_restrict_sz_q_from_the_dihedral_sector(torch, dk):
    """12-site ring at weight 6: (k = 0, refl 0, inv +1) -> (k = dk), S^z_q; apply and the exported matrix against B2^+ A B1"""
    dst, op = G.ring(12, 6, dk), X.sz_q(12, dk)
    plan, x, y, ref = _against_dense(torch, DIHEDRAL12, dst, op, "c128", "restrict")
    assert ref["leak"] < 1e-12 and ref["norm"] > 1.0
    assert len(ref["src"]) < len(ref["dst"])  # the point: the source has 2-4 times fewer rows
    dense = plan.to_csr().to_dense().cpu().numpy()
    assert dense.shape == ref["matrix"].shape
    scale = G.row_scale(X.coefficient_sum(op), ref["n2"], 1.0)[:, None]
    G.compare(dense, ref["matrix"], G.monomials(op), scale, f"restrict to_csr dk {dk}")
    plan.destroy()


def test_restrict_f64_into_a_reflection_sector(torch):
    """8-site ring in f64: (0, 0, +1) -> reflection only (odd: the staggered field changes sign under i -> 7 - i)"""
    dst = G.with_generators(8, 4, [(G.reflection(8), 1)])
    plan, _, _, ref = _against_dense(torch, G.ring(8, 4, 0, 0, 1), dst, X.staggered_z(8), "f64", "restrict")
    assert ref["leak"] < 1e-12 and ref["norm"] > 1.0
    plan.destroy()


def test_restrict_refuses_a_wrong_dk_and_names_the_target_generator(torch):
    sbasis, A, sreps, tbasis, treps = _setup(DIHEDRAL12, G.ring(12, 6, 5), X.sz_q(12, 4))
    with pytest.raises(D.LsAmdError, match="generator 0"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="restrict")
    assert G.dense(DIHEDRAL12, G.ring(12, 6, 5), X.sz_q(12, 4))["leak"] > 1.0  # by the projectors the image leaves the sector


def test_restrict_refuses_a_target_generator_outside_the_source_group(torch):
    src = G.with_generators(8, 4, [(G.reflection(8), 0)])
    dst = G.with_generators(8, 4, [(G.translation(8, 2), 0)])
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, X.sz_q(8, 0))
    with pytest.raises(D.LsAmdError, match=r'generator 0 .*groups="project"'):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="restrict")
    # ... and today's path keeps today's refusal
    with pytest.raises(D.LsAmdError, match="different generators"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128)
    with pytest.raises(D.LsAmdError, match="different generators"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="same")
    with pytest.raises(D.LsAmdError, match="none of 'same', 'restrict', 'project'"):
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="subgroup")


# ---- 5-7: groups="project" -------------------------------------------------------------------------------------------------------
FREE12 = G.ring(12, None, 0, 0, 1)
_norms_by_k = {}


@pytest.mark.parametrize("k", range(12))
def test_project_local_sz_into_every_momentum_at_free_weight(torch, k):
    """12-site ring without a fixed weight, sigma^z_0 from (k = 0, refl, inv): ~350 target rows, two tiles and a seam"""
    plan, x, y, ref = _against_dense(torch, FREE12, G.ring(12, None, k), G.sz_site(0), "c128", "project")
    assert 256 < len(ref["dst"]) < 512
    assert ref["leak"] > 0.1  # covariant under nothing: the restricted route would be wrong here
    assert plan.nnz > 0
    with pytest.raises(D.LsAmdError, match="no CSR export"):
        plan.to_csr()
    _norms_by_k[k] = (float(torch.vdot(y, y).real), float(np.linalg.norm(ref["image"] @ x.cpu().numpy()) ** 2))
    plan.destroy()


def test_project_components_add_up_to_the_full_image(torch):
    """sum_k ||y_k||^2 = ||A B1 x||^2: the translation sectors are a resolution of the identity.  Every y_k is within its bound, so
    the sum of squares is within a few (S + 2) 2^-53 relative; 1e-12 is far above that and far below any missing component."""
    for k in range(12):
        if k not in _norms_by_k:
            test_project_local_sz_into_every_momentum_at_free_weight(torch, k)
    got, want = sum(v[0] for v in _norms_by_k.values()), _norms_by_k[0][1]
    print(f"sum over k of |y_k|^2 = {got!r}, |A B1 x|^2 = {want!r}")
    assert want > 1.0 and abs(got - want) <= 1e-12 * want


@pytest.mark.parametrize("dt", ["f64", "c128"])
@pytest.mark.parametrize("inv", [1, -1])
def test_project_the_identity_upwards(torch, dt, inv):
    """A = 1 from translations-only k = 0 into the dihedral (0, 0) sector with inversion +-1: the component of the state in the
    larger group's sector, equal to project(unproject(x))"""
    src, dst, op = G.ring(12, 6, 0), G.ring(12, 6, 0, 0, inv), G.identity(12)
    plan, x, y, ref = _against_dense(torch, src, dst, op, dt, "project")
    assert len(ref["dst"]) < len(ref["src"])
    sbasis, tbasis = D.loadConfigFromDict(src), D.loadConfigFromDict(dst)
    lib = D.project(tbasis, plan.target_reps, D.unproject(sbasis, plan.source_reps, x))
    S = G.monomials(op) * G.group_order(dst)
    G.compare(y.cpu().numpy(), lib.cpu().numpy(), S, G.row_scale(X.coefficient_sum(op), ref["n2"], x.abs().max()), f"identity upwards inv {inv} {dt} vs project(unproject)")
    plan.destroy()


@pytest.mark.parametrize("k", [2, 7])
def test_project_many_flip_groups_and_complex_coefficients(torch, k):
    """sum_j e^{-iqj} sigma^+_j sigma^-_{j+1} + sigma^z_0 on 12 sites: 13 groups (4 per pass), complex coefficients and characters"""
    plan, _, _, ref = _against_dense(torch, DIHEDRAL12, G.ring(12, 6, k), G.hop_q_plus_sz0(12, 1), "c128", "project")
    assert ref["leak"] > 0.1
    plan.destroy()


# ---- 8: 64-bit words against the library's composition -----------------------------------------------------------------------
def _composition(torch, src, dst, plain, op, x, fermion=False):
    """project(target) o MatvecPlan(A on the plain basis) o unproject(source)"""
    sbasis, tbasis, pbasis = D.loadConfigFromDict(src), D.loadConfigFromDict(dst), D.loadConfigFromDict(plain)
    sreps, treps, preps = D.enumerateStates(sbasis, 1)[0], D.enumerateStates(tbasis, 1)[0], D.enumerateStates(pbasis, 1)[0]
    phi = (D.fermion_unproject if fermion else D.unproject)(sbasis, sreps[0], x).to(x.dtype).contiguous()
    assert phi.numel() == preps[0].numel()
    A = D.Operator.fromSpec(pbasis, config.parse_operator(op, pbasis.spec))
    out = torch.zeros_like(phi)
    D.MatvecPlan(A, preps, x.dtype).matvec([phi], [out])
    return D.project(tbasis, treps[0], out)


@pytest.mark.parametrize("groups", ["restrict", "project"])
def test_64_bit_words_against_the_library_composition(torch, groups):
    """34-site ring at weight 2 (561 states): dihedral (0, 0) -> (k = 5); S^z_q restricted, a local bond plus sigma^z_0 projected"""
    L = 34
    src, dst, plain = G.ring(L, 2, 0, 0), G.ring(L, 2, 5), {"basis": {"number_spins": L, "hamming_weight": 2, "symmetries": []}}
    if groups == "restrict":
        op = X.sz_q(L, 5)
    else:
        op = {"terms": [{"expression": "σᶻ₀", "sites": [[0]]}, {"expression": "σ⁺₀ σ⁻₁", "sites": [[0, 1], [1, 0]]}]}
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert (sreps.numel(), treps.numel()) == (17, 16)  # 561 states: 17 dihedral orbits, 16 translation orbits with norm at k = 5
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups=groups)
    assert plan.kernel == ("k_cross_project" if groups == "project" else "k_cross_pull") and plan.nnz > 0
    x = D.fillRandom(sreps, 3, torch.complex128)
    y = _apply(torch, plan, x, treps.numel())
    want = _composition(torch, src, dst, plain, op, x)
    assert float(want.abs().max()) > 1e-3
    # n2(r') >= |G2|^-1/2: the row's sum of |coefficient| is at most sum |c_j| sqrt(|G2|)
    S = G.monomials(op) * (L if groups == "project" else 1)
    G.compare(y.cpu().numpy(), want.cpu().numpy(), S, X.coefficient_sum(op) * float(x.abs().max()) * np.sqrt(L), f"34 sites {groups}")
    plan.destroy()


# ---- 9: fermions -----------------------------------------------------------------------------------------------------------------
def _fermi_case(torch, src, dst, model, dt, groups, seed=5):
    spinful = src["n_up"] is not None
    ref = R.reference(src, dst, model)
    sbasis, A, sreps, tbasis, treps = _setup(R.basis_config(src), R.basis_config(dst), R.operator_section(model, spinful))
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3
    dtype = _dtype(torch, dt)
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype, groups=groups)
    assert plan.kernel == ("k_cross_project_fermi" if groups == "project" else "k_cross_pull_fermi")
    x = D.fillRandom(sreps, seed, dtype)
    y = _apply(torch, plan, x, len(ref["dst"]))
    want = ref["matrix"] @ x.cpu().numpy()
    if dt == "f64":
        assert np.abs(ref["matrix"].imag).max() <= 1e-14
        want = want.real
    order = len(F.closure(dst["L"], dst["gens"], dst["secs"])) if not spinful else None
    if spinful:
        import fermion_spinful_symm as FS

        order = len(FS.group(dst["L"], dst["gens"], dst["secs"], dst["flip"]))
    S = len(model) * (order if groups == "project" else 1)
    # n2(r') >= |G2|^-1/2, as above
    G.compare(y.cpu().numpy(), want, S, R.coefficient_sum(model) * float(x.abs().max()) * np.sqrt(order), f"fermions {groups} {dt} rows {len(ref['dst'])}")
    return plan, ref


FD10 = R.sector(10, 4, F.dihedral(10), [0, 0])


def test_fermions_restrict_n_q_and_c_dagger_q(torch):
    plan, ref = _fermi_case(torch, FD10, R.sector(10, 4, F.translations(10), [3]), R.n_q(10, 3), "c128", "restrict")
    assert ref["leak"] <= 4e-14 and ref["norm"] > 1.0
    plan.destroy()
    plan, ref = _fermi_case(torch, FD10, R.sector(10, 5, F.translations(10), [2]), R.c_dag(10, 2), "c128", "restrict")
    assert ref["leak"] <= 4e-14 and ref["norm"] > 1.0
    plan.destroy()


@pytest.mark.parametrize("k", range(10))
def test_fermions_project_local_c_dagger_into_every_momentum(torch, k):
    plan, ref = _fermi_case(torch, FD10, R.sector(10, 5, F.translations(10), [k]), [(1.0, [("+", 0, 0)])], "c128", "project")
    assert ref["leak"] > 0.1 * ref["norm"]
    plan.destroy()


@pytest.mark.parametrize("dt", ["f64", "c128"])
def test_fermions_project_into_a_dihedral_target_drops_zero_norm_orbits(torch, dt):
    """translations-only k = 5 (characters +-1) -> dihedral (0, 0), sum_j w_j c+_j with uneven weights: images of the adjoint whose
    orbit has no norm in the source sector must contribute nothing, and the reference meets such images"""
    src, dst = R.sector(10, 4, F.translations(10), [5]), R.sector(10, 5, F.dihedral(10), [0, 0])
    model = [(1.0 + 0.25 * j, [("+", j, 0)]) for j in range(10)]
    plan, ref = _fermi_case(torch, src, dst, model, dt, "project")
    assert ref["pull_dropped"] > 0
    plan.destroy()


@pytest.mark.parametrize("groups", ["restrict", "project"])
def test_spinful_fermions_with_spin_flip_on_the_source_only(torch, groups):
    src = R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1)
    dst = R.sector(4, 4, F.translations(4), [1], n_up=2)
    model = R.n_q(4, 1, True) if groups == "restrict" else [(1.0, [("n", 0, 0)]), (0.5, [("+", 0, 0), ("-", 1, 0)])]
    plan, ref = _fermi_case(torch, src, dst, model, "c128", groups)
    if groups == "restrict":
        assert ref["leak"] <= 4e-14
    plan.destroy()


# ---- 10, 12: the routes agree; equal bytes ---------------------------------------------------------------------------------------
def test_project_agrees_with_restrict_where_restrict_is_valid(torch):
    dst, op = G.ring(12, 6, 5), X.sz_q(12, 5)
    p1, x, y1, ref = _against_dense(torch, DIHEDRAL12, dst, op, "c128", "restrict")
    p2, _, y2, _ = _against_dense(torch, DIHEDRAL12, dst, op, "c128", "project")
    S = G.monomials(op) * (G.group_order(dst) + 1)  # both routes' summands
    G.compare(y2.cpu().numpy(), y1.cpu().numpy(), S, G.row_scale(X.coefficient_sum(op), ref["n2"], x.abs().max()), "project vs restrict")
    assert p2.nnz >= p1.nnz
    p1.destroy(), p2.destroy()


@pytest.mark.parametrize("name", ["L8_sz_k0_k3", "L8_dihedral_staggered", "L8_splus_w4_w3_k1_k4"])
def test_same_and_restrict_on_equal_generators_return_equal_bytes(torch, name):
    src, dst, op, dt = X.CASES[name]
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    dtype = _dtype(torch, dt)
    a = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    b = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype, groups="restrict")
    assert a.kernel == b.kernel == "k_cross_pull" and a.nnz == b.nnz
    x = D.fillRandom(sreps, 7, dtype)
    ya, yb = _apply(torch, a, x, treps.numel()), _apply(torch, b, x, treps.numel())
    assert float(ya.abs().max()) > 1e-3 and torch.equal(ya.view(torch.float64), yb.view(torch.float64))
    ma, mb = a.to_csr(), b.to_csr()
    assert torch.equal(ma.crow_indices, mb.crow_indices) and torch.equal(ma.col_indices, mb.col_indices)
    assert ma.nnz > 0 and torch.equal(ma.values.view(torch.float64), mb.values.view(torch.float64))


@pytest.mark.parametrize("groups", ["restrict", "project"])
def test_two_applies_of_one_plan_return_equal_bytes(torch, groups):
    """restrict: S^z_q, one packet per row (k_cross_pull adds a row's packets in LDS as they arrive; with one there is no order);
    project: 13 groups -- k_cross_project adds a row's packets in registers in a fixed order"""
    op = X.sz_q(12, 5) if groups == "restrict" else G.hop_q_plus_sz0(12, 1)
    sbasis, A, sreps, tbasis, treps = _setup(DIHEDRAL12, G.ring(12, 6, 5), op)
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups=groups)
    x = D.fillRandom(sreps, 9, torch.complex128)
    y1, y2 = _apply(torch, plan, x, treps.numel()), _apply(torch, plan, x, treps.numel())
    assert float(y1.abs().max()) > 1e-3 and torch.equal(y1.view(torch.float64), y2.view(torch.float64))
    plan.destroy()


# ---- 11: spectral_function -------------------------------------------------------------------------------------------------------
def _heisenberg(basis_cfg, L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "Heisenberg", "terms": [
        {"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}


def test_spectral_function_from_the_dihedral_ground_state(torch):
    """S(q, w) of the 12-site ring with psi from (k = 0, refl 0, inv +1) and S^z_q, q = 5, into the translations-only k = 5: moments
    against the eigendecomposition of the dense target sector with v0 = (B2^+ A B1) psi, as tests/test_gpu_cross_sector.py checks its own"""
    from oracle import model as M

    L, M_ = 12, 128
    src, dst, op = DIHEDRAL12, G.ring(L, 6, 5), X.sz_q(L, 5)
    cfg = _heisenberg(src, L)
    cfg["observables"] = [op]
    reps_t, H = M.dense_sector_matrix(_heisenberg(dst, L))
    H = np.asarray(H)
    evals, U = np.linalg.eigh(H)
    w = evals[-1] - evals[0]
    bounds = (float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w))
    with pytest.raises(D.LsAmdError, match="different generators|one basis only"):
        kpm.spectral_function(cfg, 0, num_moments=M_, bounds=bounds, dtype=torch.complex128, target=dst)
    E, S, res = kpm.spectral_function(cfg, 0, num_moments=M_, bounds=bounds, dtype=torch.complex128, target=dst, groups="restrict")
    ref = G.dense(src, dst, op)
    assert np.array_equal(ref["dst"], np.asarray(reps_t, dtype=np.uint64))
    psi = res.state.cpu().numpy()
    assert psi.shape == (len(ref["src"]),)
    v0 = ref["matrix"] @ psi
    assert np.abs(res.target_state.cpu().numpy() - v0).max() <= 1e-12 * max(1.0, np.abs(v0).max())
    mu = res.moments
    assert mu.shape == (1, M_) and mu[0, 0] > 0.1
    weights = (np.abs(U.conj().T @ v0.reshape(-1, 1)) ** 2).T
    exact = exact_moments(evals, weights, M_, bounds)
    tol, own = moment_tolerance(H, v0.reshape(-1, 1), M_, bounds, exact)
    dev = np.abs(mu - exact).max(axis=1)
    print(f"S(q, w) moments dihedral -> k 5: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}, mu_0 {exact[0, 0]:.6g}")
    assert (dev <= tol).all(), (dev, tol)
    assert E.shape == S.shape == (2 * M_,) and (S >= 0.0).all()
    # the projecting route gives the same v0 here, hence the same moments
    _, _, res_p = kpm.spectral_function(cfg, 0, state=res.state, num_moments=16, bounds=bounds, dtype=torch.complex128, target=dst, groups="project")
    assert np.abs(res_p.moments[0] - mu[0, :16]).max() <= 1e-11 * mu[0, 0]


# ---- failures that must be loud ------------------------------------------------------------------------------------------------
def test_project_refusals(torch):
    sbasis, A, sreps, tbasis, treps = _setup(DIHEDRAL12, G.ring(12, 6, 5), G.sz_site(0))
    with pytest.raises(D.LsAmdError, match="c128"):  # complex target characters
        D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64, groups="project")
    other = D.loadConfigFromDict(G.ring(10, 5, 3))
    oreps, _ = D.enumerateStates(other, 1)
    with pytest.raises(D.LsAmdError, match="different number_sites"):
        D.CrossSectorPlan(A, sreps, other, oreps[0], torch.complex128, groups="project")
    fermi = D.loadConfigFromDict({"basis": {"particle": "spinless-fermion", "number_sites": 12, "number_particles": 6}})
    freps, _ = D.enumerateStates(fermi, 1)
    with pytest.raises(D.LsAmdError, match="particle types"):
        D.CrossSectorPlan(A, sreps, fermi, freps[0], torch.complex128, groups="project")
    with pytest.raises(D.LsAmdError, match="one partition|1-D int64"):
        D.CrossSectorPlan(A, [sreps], tbasis, treps, torch.complex128, groups="project")


def test_project_reports_an_image_outside_the_source_basis(torch):
    """sigma^+_0 between two bases of the SAME weight: nothing checks covariance here, the kernel's flag does"""
    src, dst = G.ring(12, 6, 0, 0, 1), G.ring(12, 6, 3)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}]})
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="project")
    x = D.fillRandom(sreps, 1, torch.complex128)
    y = torch.zeros(treps.numel(), dtype=torch.complex128, device=x.device)
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.apply(x, y)
    plan.check()  # reported once
