"""Interior eigenpairs on the GPU: the Chebyshev series on a block (kpm.chebyshev_series, MatvecPlan.matvec_block_series,
ls_amd_matvec_block_series) against U p(Lambda) U^+ X of the dense sector matrix, and diagonalize.interior_eigenpairs /
diagonalize(sigma=...) against the full spectrum: unprojected f64, projected c128, degenerate levels, the band edge, an order too
small to converge, and the refusals through Python and through ctypes."""
import ctypes as C
import functools

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib, config, kpm
from distributed_matvec_amd import diagonalize as dg
from distributed_matvec_amd.diagonalize import LocalOperator

pytestmark = pytest.mark.gpu

EPS = 1e-9


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def ring(L, fields_seed=None, momentum=None):
    cfg = config.heisenberg_chain_config(L)
    if momentum is not None:
        cfg["basis"]["symmetries"] = [{"permutation": [(i + 1) % L for i in range(L)], "sector": momentum}]
    if fields_seed is not None:
        h = np.random.RandomState(fields_seed).uniform(-1.0, 1.0, L)
        cfg["hamiltonian"]["terms"] += [{"expression": f"{float(h[i])!r} × σᶻ₀", "sites": [[i]]} for i in range(L)]
    return cfg


MODELS = {
    "ring_12": (lambda: ring(12), "f64"),                        # 924 states, degenerate levels
    "ring_16_k3": (lambda: ring(16, momentum=3), "c128"),        # 810 states, complex characters
    "ring_14_fields": (lambda: ring(14, fields_seed=5), "f64"),  # 3432 states, no level degenerate
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(config, operator, dense matrix, eigenvalues, eigenvectors, bounds, ||H||): computed once, shared, never written to"""
    import torch

    make, dt = MODELS[name]
    cfg = make()
    dtype = torch.float64 if dt == "f64" else torch.complex128
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, dtype)
    H = h.to_dense(reps, dtype=dtype).cpu().numpy()
    assert np.abs(H - H.conj().T).max() <= 1e-13 * np.abs(H).max()
    lam, U = np.linalg.eigh(H)
    w = lam[-1] - lam[0]
    bounds = (float(lam[0] - 0.01 * w), float(lam[-1] + 0.01 * w))
    return cfg, op, H, lam, U, bounds, max(abs(bounds[0]), abs(bounds[1]))


def layout_block(torch, X, layout, dtype):
    n, K = X.shape
    t = torch.empty((n, K), dtype=dtype, device="cuda") if layout == "interleaved" else torch.empty((K, n), dtype=dtype, device="cuda").t()
    t.copy_(torch.from_numpy(np.ascontiguousarray(X)).to(dtype).cuda())
    return t


# ---------------------------------------------------------------------------------------------
# (a) the series against the dense matrix
# ---------------------------------------------------------------------------------------------
WORST = {}


# the Heisenberg ring's single-vector kernel is the staged chain kernel, so LS_AMD_BLOCK=auto sends its blocks through the column
# loop ("epilogue"); LS_AMD_BLOCK=kernel asks for the row kernel k_direct_cheb.  The column loop gets a shorter pass of its own.
@pytest.mark.parametrize("name,mode,path", [("ring_12", "kernel", "k_direct_cheb"), ("ring_16_k3", "auto", "k_pull_gather_cheb"),
                                            ("ring_12", "auto", "epilogue")])
def test_series_against_dense(torch, monkeypatch, name, mode, path):
    cfg, op, H, lam, U, bounds, h_norm = case(name)
    monkeypatch.setenv("LS_AMD_BLOCK", mode)
    dtype = op.dtype
    n = op.n_local
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    r = int((np.abs(H - np.diag(np.diag(H))) > 0).sum(axis=1).max())
    assert op.plan.series_kernel(8) == op.plan.axpby_kernel(8) == path
    rng = np.random.RandomState(17)
    worst = 0.0
    for N in (0, 1, 2, 65, 200) if path != "epilogue" else (0, 2, 65):
        c = rng.uniform(-1.0, 1.0, N + 1)
        pL = cheb.chebval((lam - b) / a, c)
        for K in (1, 3, 8) if path != "epilogue" else (3,):
            X = rng.uniform(-0.5, 0.5, (n, K)) + (1j * rng.uniform(-0.5, 0.5, (n, K)) if dtype == torch.complex128 else 0.0)
            want = (U * pL[None, :]) @ (U.conj().T @ X)
            bound = 8.0 * (r + 4) * (N + 1) * 2.0 ** -53 * np.abs(c).sum() * np.linalg.norm(X, axis=0)
            for layout in ("interleaved", "colmajor"):
                x = layout_block(torch, X, layout, dtype)
                x0 = x.clone()
                before = op.matvecs
                z = kpm.chebyshev_series(op, x, c, bounds)
                assert z.dtype == dtype and tuple(z.shape) == (n, K)  # real coefficients keep the operator's dtype
                assert torch.equal(x, x0) and op.matvecs - before == K * N
                err = np.linalg.norm(z.cpu().numpy() - want, axis=0)
                worst = max(worst, float((err / bound).max()))
                assert (err <= bound).all(), (name, N, K, layout, err / bound)
                # the binding itself, Z with strides of its own, holding NaN before: assigned, and two calls agree to the byte
                z1 = layout_block(torch, np.full((n, K), np.nan), "colmajor" if layout == "interleaved" else "interleaved", dtype)
                z2 = torch.full_like(z1, float("nan"))
                op.plan.matvec_block_series(x, z1, c, bounds)
                op.plan.matvec_block_series(x, z2, c, bounds)
                assert torch.equal(z1, z2), (name, N, K, layout)
                assert (np.linalg.norm(z1.cpu().numpy() - want, axis=0) <= bound).all(), (name, N, K, layout)
    # a vector is a block of one column; complex coefficients make the sum complex128
    v = rng.uniform(-0.5, 0.5, n)
    c = rng.uniform(-1.0, 1.0, 9) + 1j * rng.uniform(-1.0, 1.0, 9)
    z = kpm.chebyshev_series(op, torch.from_numpy(v).to(dtype).cuda(), c, bounds)
    want = (U * cheb.chebval((lam - b) / a, c)[None, :]) @ (U.conj().T @ v)
    assert z.dtype == torch.complex128 and tuple(z.shape) == (n,)
    assert np.linalg.norm(z.cpu().numpy() - want) <= 8.0 * (r + 4) * 9 * 2.0 ** -53 * np.abs(c).sum() * np.linalg.norm(v)
    WORST[name, path] = worst
    print(f"series {name} {path}: worst error / bound = {worst:.3f} (r = {r})")


@pytest.mark.parametrize("name", ["ring_12", "ring_16_k3"])
def test_bounds_that_cut_the_spectrum_are_named(torch, name):
    cfg, op, H, lam, U, bounds, h_norm = case(name)
    cut = (float(lam[0] + 0.3 * (lam[-1] - lam[0])), bounds[1])
    x = torch.from_numpy(np.random.RandomState(3).uniform(-0.5, 0.5, (op.n_local, 3))).to(op.dtype).cuda()
    with pytest.raises(D.LsAmdError) as e:
        kpm.chebyshev_series(op, x, np.ones(201), cut)
    msg = str(e.value)
    assert f"{cut[0]:.17g}" in msg and f"{cut[1]:.17g}" in msg and "order" in msg, msg
    # the plan is as good as before
    z = kpm.chebyshev_series(op, x, [0.0, 1.0], bounds)
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    assert np.abs(z.cpu().numpy() - (H @ x.cpu().numpy() - b * x.cpu().numpy()) / a).max() <= 1e-13


# ---------------------------------------------------------------------------------------------
# (b), (c), (d) interior pairs against the full spectrum
# ---------------------------------------------------------------------------------------------
def levels(lam, h_norm):
    """the distinct exact levels: lists of indices into lam (levels closer than 1e-9 ||H|| are one level)"""
    out = [[0]]
    for j in range(1, len(lam)):
        if lam[j] - lam[out[-1][-1]] <= 1e-9 * h_norm:
            out[-1].append(j)
        else:
            out.append([j])
    return out


def nudged(lam, sigma, k, margin):
    """sigma moved so that the k-th and (k + 1)-th nearest levels differ in distance by at least `margin`"""
    for shift in np.concatenate([[0.0], np.linspace(0.0, 1.0, 201)[1:] * (lam[-1] - lam[0]) * 0.01]):
        d = np.sort(np.abs(lam - (sigma + shift)))
        if d[k] - d[k - 1] >= margin:
            return float(sigma + shift)
    raise AssertionError("no sigma with an unambiguous set of nearest levels")


def check_pairs(torch, r, op, H, lam, U, sigma, k, h_norm):
    assert r.converged and len(r.eigenvalues) == k
    got = np.array(r.eigenvalues)
    assert np.all(np.diff(got) >= 0.0)
    near = np.sort(np.argsort(np.abs(lam - sigma), kind="stable")[:k])
    # the multiset of the k nearest exact levels, one to one (both ascending)
    assert np.abs(got - lam[near]).max() <= EPS * h_norm, (got, lam[near])
    assert max(r.residual_norms) <= EPS * h_norm, r.residual_norms
    groups = levels(lam, h_norm)
    worst = 0.0
    for th, y, res in zip(r.eigenvalues, r.eigenvectors, r.residual_norms):
        yh = y.cpu().numpy()
        assert abs(np.linalg.norm(H @ yh - th * yh) - res) <= 1e-12 * h_norm
        g = min(groups, key=lambda idx: abs(lam[idx[0]] - th))
        others = np.delete(lam, g)
        gap = np.abs(others - th).min()
        outside = 1.0 - float((np.abs(U[:, g].conj().T @ yh) ** 2).sum()) / float(np.vdot(yh, yh).real)
        allowed = 4.0 * (EPS * h_norm / gap) ** 2
        worst = max(worst, outside / allowed)
        assert outside <= allowed + 1e-14, (th, outside, allowed, gap)  # (1e-14: the rounding of the projection itself)
    assert r.order >= 2 and r.applications >= 1 and r.matvecs >= r.applications * r.order and r.polish_rounds <= 3
    return worst


# (mid-band on the ring with fields takes an order of about 2500: under LS_AMD_BLOCK=auto that plan's blocks go column by column,
# 24 launches per order, so the long case asks for the row kernel and the short one keeps the default path)
@pytest.mark.parametrize("name,where,mode", [("ring_14_fields", 0.5, "kernel"), ("ring_14_fields", 0.25, "auto"),
                                             ("ring_16_k3", 0.5, "auto"), ("ring_16_k3", 0.25, "auto")])
def test_interior_pairs(torch, monkeypatch, name, where, mode):
    cfg, op, H, lam, U, bounds, h_norm = case(name)
    monkeypatch.setenv("LS_AMD_BLOCK", mode)
    k = 8
    sigma = nudged(lam, lam[0] + where * (lam[-1] - lam[0]), k, 100.0 * EPS * h_norm)
    r = dg.interior_eigenpairs(op, sigma, num_evals=k, eps=EPS, bounds=bounds)
    print(f"interior {name} at {where}: order {r.order}, applications {r.applications}, restarts {r.lanczos_restarts}, polish "
          f"{r.polish_rounds}, matvecs {r.matvecs}, seconds {r.seconds:.2f} (filter {r.filter_seconds:.2f}, ritz {r.ritz_seconds:.2f}), "
          f"kernel {r.kernel}, max residual / ||H|| {max(r.residual_norms) / h_norm:.2e}")
    check_pairs(torch, r, op, H, lam, U, sigma, k, h_norm)
    assert r.sigma == sigma and r.bounds == bounds and r.eigenvectors[0].dtype == op.dtype


def test_degenerate_levels_come_with_their_multiplicity(torch):
    cfg, op, H, lam, U, bounds, h_norm = case("ring_12")
    groups = levels(lam, h_norm)
    assert max(len(g) for g in groups) >= 2  # the +-k pairs
    margin = 100.0 * EPS * h_norm
    chosen = None
    start = next(i for i, g in enumerate(groups) if lam[g[0]] >= lam[0] + 0.3 * (lam[-1] - lam[0]))
    for i in range(start, len(groups) - 1):
        for j in range(i, len(groups) - 1):
            count = sum(len(g) for g in groups[i:j + 1])
            if count > 14:
                break
            e_lo, e_hi = lam[groups[i][0]], lam[groups[j][-1]]
            sigma = 0.5 * (e_lo + e_hi)
            half = 0.5 * (e_hi - e_lo)
            if count >= 8 and min(sigma - lam[groups[i - 1][-1]], lam[groups[j + 1][0]] - sigma) >= half + margin \
                    and max(len(g) for g in groups[i:j + 1]) <= 8 and any(len(g) > 1 for g in groups[i:j + 1]):
                chosen = (float(sigma), count)
                break
        if chosen:
            break
    assert chosen, "no window of whole levels"
    sigma, k = chosen
    r = dg.interior_eigenpairs(op, sigma, num_evals=k, eps=EPS, block_size=8, bounds=bounds)
    print(f"interior ring_12 degenerate: k {k}, order {r.order}, applications {r.applications}, polish {r.polish_rounds}, seconds {r.seconds:.2f}")
    check_pairs(torch, r, op, H, lam, U, sigma, k, h_norm)


# ---------------------------------------------------------------------------------------------
# (e) the band edge, and diagonalize()
# ---------------------------------------------------------------------------------------------
def test_band_edge_and_diagonalize(torch):
    cfg, op, H, lam, U, bounds, h_norm = case("ring_14_fields")
    k = 4
    low = dg.lanczos_block_smallest(op, num_evals=k, block_size=4, eps=EPS)
    assert low.converged and np.abs(np.array(low.eigenvalues) - lam[:k]).max() <= EPS * h_norm
    sigma = 0.5 * (bounds[0] + lam[0])  # just inside the lower edge: the nearest levels are the lowest
    r = dg.interior_eigenpairs(op, sigma, num_evals=k, eps=EPS, block_size=4, bounds=bounds)
    assert r.converged and np.abs(np.array(r.eigenvalues) - np.array(low.eigenvalues)).max() <= 2.0 * EPS * h_norm
    for y, v in zip(r.eigenvectors, low.eigenvectors):
        gap = float(np.diff(lam[:k + 1]).min())
        assert 1.0 - abs(complex(torch.vdot(y, v))) ** 2 <= 2.0 * 4.0 * (EPS * h_norm / gap) ** 2 + 1e-14
    # diagonalize(sigma=...) is interior_eigenpairs (same defaults, same seed); its own bounds come from spectral_bounds
    # (a quarter of the band: the levels are sparser there and the order a few hundred)
    mid = nudged(lam, lam[0] + 0.25 * (lam[-1] - lam[0]), k, 100.0 * EPS * h_norm)
    d = dg.diagonalize(cfg, num_evals=k, eps=EPS, block_size=4, sigma=mid)
    i = dg.interior_eigenpairs(cfg, mid, num_evals=k, eps=EPS, block_size=4, max_basis=24)
    assert isinstance(d, dg.InteriorResult) and d.converged and i.converged
    assert np.abs(np.array(d.eigenvalues) - np.array(i.eigenvalues)).max() <= 2.0 * EPS * h_norm
    near = np.sort(np.argsort(np.abs(lam - mid))[:k])
    assert np.abs(np.array(d.eigenvalues) - lam[near]).max() <= EPS * h_norm
    # without sigma nothing changed: the driver is lanczos_smallest
    d0 = dg.diagonalize(cfg, num_evals=2, eps=EPS)
    l0 = dg.lanczos_smallest(op, num_evals=2, eps=EPS)
    assert isinstance(d0, dg.EigenResult) and np.abs(np.array(d0.eigenvalues) - np.array(l0.eigenvalues)).max() <= 2.0 * EPS * h_norm
    assert np.abs(np.array(d0.eigenvalues) - lam[:2]).max() <= EPS * h_norm


# ---------------------------------------------------------------------------------------------
# (f) an order too small
# ---------------------------------------------------------------------------------------------
def test_an_order_too_small_is_reported(torch):
    cfg, op, H, lam, U, bounds, h_norm = case("ring_14_fields")
    r = dg.interior_eigenpairs(op, 0.5 * (lam[0] + lam[-1]), num_evals=8, eps=EPS, bounds=bounds, order=4, max_polish=0)
    assert not r.converged and r.polish_rounds == 0 and r.order == 4 and len(r.eigenvalues) == 8
    assert max(r.residual_norms) > EPS * h_norm
    for th, y, res in zip(r.eigenvalues, r.eigenvectors, r.residual_norms):
        yh = y.cpu().numpy()
        assert abs(np.linalg.norm(H @ yh - th * yh) - res) <= 1e-12 * h_norm


# ---------------------------------------------------------------------------------------------
# (g) refusals, through Python and through ctypes
# ---------------------------------------------------------------------------------------------
def test_refusals(torch):
    L = _lib.load()
    cfg, op, H, lam, U, bounds, h_norm = case("ring_12")
    n = op.n_local
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    coeffs = (C.c_double * 8)(1.0, 0.0, 0.5, 0.0, 0.25, 0.0, 0.125, 0.0)
    x = torch.ones((n, 2), dtype=torch.float64, device="cuda")
    z = torch.zeros_like(x)

    def call(plan, K=2, N=3, c=coeffs, lo=bounds[0], hi=bounds[1], X=x, Z=z, z_cplx=0):
        return L.ls_amd_matvec_block_series(plan.h, K, N, C.cast(c, C.c_void_p) if c is not None else None, lo, hi, vp(X), X.stride(0),
                                            X.stride(1), vp(Z), Z.stride(0), Z.stride(1), z_cplx, None, None)

    assert call(op.plan) == 0 and L.ls_amd_plan_check(op.plan.h, None) == 0
    # a non-Hermitian operator
    bad = config.heisenberg_chain_config(12)
    bad["hamiltonian"]["terms"].append({"expression": "σ⁺₀ σ⁻₁", "sites": [[0, 1]]})
    basis, h = D.loadConfigFromDict(bad, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    nh = LocalOperator(h, reps, torch.float64)
    with pytest.raises(ValueError, match="not Hermitian"):
        dg.interior_eigenpairs(nh, 0.0, bounds=bounds)
    with pytest.raises(ValueError, match="not Hermitian"):
        kpm.chebyshev_series(nh, x, [1.0, 0.5], bounds)
    with pytest.raises(ValueError, match="not Hermitian"):
        dg.diagonalize(bad, num_evals=2, sigma=0.0)
    # two partitions
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps2, _ = D.enumerateStates(basis, 2)
    two = LocalOperator(h, reps2, torch.float64)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        dg.interior_eigenpairs(two, 0.0, bounds=bounds)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        kpm.chebyshev_series(two, x, [1.0, 0.5], bounds)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        two.plan.matvec_block_series(x, z, [1.0, 0.5], bounds)
    assert call(two.plan) == -1 and "one-partition" in L.ls_amd_last_error().decode()
    with pytest.raises(ValueError, match="num_partitions"):
        dg.diagonalize(cfg, num_evals=2, num_partitions=2, sigma=0.0)
    # K = 65
    big = torch.ones((n, 65), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="65"):
        kpm.chebyshev_series(op, big, [1.0, 0.5], bounds)
    with pytest.raises(D.LsAmdError, match="K = 65"):
        op.plan.matvec_block_series(big, torch.zeros_like(big), [1.0, 0.5], bounds)
    assert call(op.plan, K=65, X=big, Z=torch.zeros_like(big)) == -1 and "K = 65" in L.ls_amd_last_error().decode()
    # an f64 Z next to c128 vectors; an f64 Z with complex coefficients
    cplx = case("ring_16_k3")[1]
    xc = torch.ones((cplx.n_local, 2), dtype=torch.complex128, device="cuda")
    zr = torch.zeros((cplx.n_local, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="complex128"):
        cplx.plan.matvec_block_series(xc, zr, [1.0, 0.5], case("ring_16_k3")[5])
    assert call(cplx.plan, X=xc, Z=zr, z_cplx=0) == -1
    msg = L.ls_amd_last_error().decode()
    assert "z_cplx" in msg and "c128" in msg, msg
    with pytest.raises(D.LsAmdError, match="not real"):
        op.plan.matvec_block_series(x, z, [1.0, 0.5j], bounds)
    ci = (C.c_double * 4)(1.0, 0.0, 0.5, 0.25)
    assert call(op.plan, N=1, c=ci) == -1 and "real coefficients" in L.ls_amd_last_error().decode()
    # a NULL coeffs, N < 0, bounds that are no bounds, Z on X
    assert call(op.plan, c=None) == -1 and "coeffs is NULL" in L.ls_amd_last_error().decode()
    assert call(op.plan, N=-1) == -1 and "N = -1" in L.ls_amd_last_error().decode()
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (0.0, float("inf"))):
        assert call(op.plan, lo=lo, hi=hi) == -1 and "bounds" in L.ls_amd_last_error().decode()
        with pytest.raises((D.LsAmdError, ValueError), match="bounds"):
            kpm.chebyshev_series(op, x, [1.0, 0.5], (lo, hi))
    assert call(op.plan, Z=x) == -1 and "Z and X overlap" in L.ls_amd_last_error().decode()
    with pytest.raises(ValueError, match=r"diagonalize\(\)"):
        dg.interior_eigenpairs(op, bounds[1] + 1.0, bounds=bounds)
    with pytest.raises(ValueError, match=r"diagonalize\(\)"):
        dg.interior_eigenpairs(op, lam[-1] + 0.5 * (lam[-1] - lam[0]))  # (outside the bounds the solver finds itself)
    # nothing above left the plan unusable
    assert call(op.plan) == 0 and L.ls_amd_plan_check(op.plan.h, None) == 0
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    want = cheb.chebval((lam - b) / a, [1.0, 0.5, 0.25, 0.125])
    got = z.cpu().numpy()
    ref = (U * want[None, :]) @ (U.T @ np.ones((n, 2)))
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
