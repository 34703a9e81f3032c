"""Interior eigenpairs without a device: the delta filter and its order rule (kpm.delta_filter, kpm.filter_order), the refusals of
diagonalize.interior_eigenpairs / diagonalize(sigma=...) that need no device, FilteredOperator and the whole solver on a dense
stand-in operator (torch on the CPU) against numpy.linalg.eigh, and the C ABI of ls_amd_matvec_block_series."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from numpy.polynomial import chebyshev as cheb

from distributed_matvec_amd import config, kpm
from distributed_matvec_amd import diagonalize as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_matvec_block_series", "ls_amd_plan_series_kernel_name")


# ---------------------------------------------------------------------------------------------
# the filter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, -3.1, 6.5, -6.9])
@pytest.mark.parametrize("order", [2, 17, 200])
def test_delta_filter_on_a_grid(sigma, order):
    bounds = (-7.5, 8.5)
    a, b = 8.0, 0.5
    s = (sigma - b) / a
    c = kpm.delta_filter(sigma, bounds, order)
    assert c.shape == (order + 1,) and c.dtype == np.float64
    x = np.linspace(-1.0, 1.0, 40001)
    step = x[1] - x[0]
    p = cheb.chebval(x, c)
    assert p.min() > 0.0  # the Jackson kernel is positive
    top = int(np.argmax(p))
    # the maximum of K(x, s) / sqrt(1 - s^2) lies within O(width^2) of s (the kernel is symmetric in its arguments, not in x - s);
    # on this grid that is within one step for the narrow filter and well inside one width (pi / order) always
    assert abs(x[top] - s) <= max(step, 0.5 * math.pi / order), (x[top], s)
    if order == 200:
        assert abs(x[top] - s) <= step
    # monotone on either side of the peak down to the cut
    cut = kpm.FILTER_CUT * p[top]
    left = top - int(np.argmax(p[:top + 1][::-1] < cut)) if (p[:top + 1] < cut).any() else 0
    right = top + int(np.argmax(p[top:] < cut)) if (p[top:] < cut).any() else len(x) - 1
    assert np.all(np.diff(p[left:top + 1]) >= 0.0) and np.all(np.diff(p[top:right + 1]) <= 0.0)
    # int p(x) sqrt(1 - s^2) / sqrt(1 - x^2) dx = g_0 = 1: Gauss-Chebyshev quadrature, exact for this degree
    m = order + 1
    nodes = np.cos(math.pi * (np.arange(m) + 0.5) / m)
    integral = math.sqrt(1.0 - s * s) * (math.pi / m) * cheb.chebval(nodes, c).sum()
    assert abs(integral - 1.0) <= 1e-13 * (order + 1)
    # the width of the peak: a Gaussian of pi sqrt(1 - s^2) / order to 15 % (the rule filter_order rests on), once it is narrow
    if order == 200:
        half = p >= math.exp(-0.5) * p[top]
        width = 0.5 * (x[half][-1] - x[half][0])
        assert abs(width / (math.pi * math.sqrt(1.0 - s * s) / order) - 1.0) <= 0.15, width


def test_delta_filter_refusals():
    with pytest.raises(ValueError, match=r"diagonalize\(\)"):
        kpm.delta_filter(9.0, (-7.5, 8.5), 10)
    with pytest.raises(ValueError, match=r"diagonalize\(\)"):
        kpm.delta_filter(-7.5, (-7.5, 8.5), 10)  # the edge itself: 1 / sqrt(1 - s^2) diverges
    with pytest.raises(ValueError, match="bounds"):
        kpm.delta_filter(0.0, (1.0, 1.0), 10)
    with pytest.raises(ValueError, match="bounds"):
        kpm.delta_filter(0.0, (0.0, float("inf")), 10)
    with pytest.raises(ValueError, match="order"):
        kpm.delta_filter(0.0, (-1.0, 1.0), -1)
    with pytest.raises(ValueError, match="sigma"):
        kpm.delta_filter(float("nan"), (-1.0, 1.0), 4)


def test_filter_order_is_monotone_and_matches_the_filter():
    bounds = (-20.0, 12.0)
    orders = [kpm.filter_order(k, 100000, 0.08, bounds) for k in (4, 8, 16, 32, 64, 128)]
    assert all(o1 >= o2 for o1, o2 in zip(orders, orders[1:])) and orders[0] > orders[-1], orders  # more levels: a wider window
    orders = [kpm.filter_order(16, 100000, d, bounds) for d in (0.01, 0.02, 0.05, 0.1, 0.3)]
    assert all(o1 <= o2 for o1, o2 in zip(orders, orders[1:])) and orders[0] < orders[-1], orders  # denser levels: a narrower one
    assert kpm.filter_order(16, 100000, 0.08, bounds, cut=0.1) > kpm.filter_order(16, 100000, 0.08, bounds, cut=0.3)
    assert kpm.filter_order(16, 100000, 0.08, bounds, sigma=-4.0) > kpm.filter_order(16, 100000, 0.08, bounds, sigma=9.0)
    # a window wider than the band is the band: the order stops falling at pi sqrt(2 ln(1 / cut)) / 2, and never below 2
    assert kpm.filter_order(10 ** 6, 10, 1.0, bounds) == math.ceil(math.pi * math.sqrt(2.0 * math.log(1.0 / kpm.FILTER_CUT)) / 2.0)
    assert kpm.filter_order(10 ** 6, 10, 1.0, bounds, cut=0.9) == 2
    # the order really puts the window's edges at the cut: both see p >= cut p(sigma), and at the next order one of them does not;
    # the Gaussian estimate alone is within 15 % of it
    for sigma in (-4.0, 5.0):
        k, dim, dos = 16, 20000, 0.05
        order = kpm.filter_order(k, dim, dos, bounds, sigma=sigma)
        a, b = 16.0, -4.0
        half = k / (2.0 * dim * dos)
        at = (np.array([sigma - half, sigma + half]) - b) / a

        def ratio(n):
            c = kpm.delta_filter(sigma, bounds, n)
            return cheb.chebval(at, c) / cheb.chebval((sigma - b) / a, c)

        assert np.all(ratio(order) >= kpm.FILTER_CUT) and np.any(ratio(order + 1) < kpm.FILTER_CUT), (ratio(order), ratio(order + 1))
        s = (sigma - b) / a
        gauss = math.pi * math.sqrt(1.0 - s * s) * math.sqrt(2.0 * math.log(1.0 / kpm.FILTER_CUT)) / (half / a)
        assert abs(order / gauss - 1.0) <= 0.15, (order, gauss)
    for bad in (dict(num_states=0), dict(dimension=0), dict(dos_at_sigma=0.0), dict(dos_at_sigma=float("nan")), dict(cut=1.0),
                dict(cut=0.0), dict(bounds=(1.0, 0.0)), dict(sigma=13.0), dict(dos_at_sigma=None)):
        args = dict(num_states=8, dimension=1000, dos_at_sigma=0.1, bounds=bounds)
        args.update(bad)
        with pytest.raises(ValueError):
            kpm.filter_order(**args)


# ---------------------------------------------------------------------------------------------
# a dense stand-in for a LocalOperator: torch on the CPU
# ---------------------------------------------------------------------------------------------
class _Matrix:
    def __init__(self, hermitian=True):
        self.isHermitian = hermitian


class DensePlan:
    """the three calls the interior solver makes of a MatvecPlan, by dense products in the order the C loop takes them"""

    def __init__(self, H, hermitian=True):
        self.H = H
        self.matrix = _Matrix(hermitian)
        self.series_calls = 0

    def matvec_block_series(self, x, z, coefficients, bounds, check=True):
        lo, hi = bounds
        a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
        c = np.asarray(coefficients).reshape(-1)
        v0 = x.clone()
        acc = float(c[0]) * v0
        if len(c) > 1:
            v1 = (self.H @ v0 - b * v0) / a
            acc = acc + float(c[1]) * v1
            for n in range(2, len(c)):
                v0, v1 = v1, 2.0 * (self.H @ v1 - b * v1) / a - v0
                acc = acc + float(c[n]) * v1
        z.copy_(acc)
        self.series_calls += 1

    def matvec_block_axpby(self, x, y, alpha, beta, gamma, dots=None, check=True):
        new = alpha * (self.H @ x) + beta * x + (gamma * y if gamma != 0.0 else 0.0)
        if dots is not None:
            K = x.shape[1]
            dots[:K] = (x.conj() * x).sum(dim=0).real
            dots[K:] = (x.conj() * new).sum(dim=0).real
        y.copy_(new)

    def series_kernel(self, K):
        return "dense"

    def check(self):
        pass


class DenseOperator:
    def __init__(self, H, hermitian=True, parts=1):
        import torch

        self.torch = torch
        self.plan = DensePlan(H, hermitian)
        self.dtype = H.dtype
        self.n_local = int(H.shape[0])
        self.sizes = [self.n_local // parts] * parts
        self.device = H.device
        self.matvecs = 0

    def matvec_block(self, x, y):
        y.copy_(self.plan.H @ x)
        self.matvecs += int(x.shape[1])

    def matvec(self, x, y):
        y.copy_(self.plan.H @ x)
        self.matvecs += 1

    def check(self):
        pass

    def dot(self, a, b):
        return self.torch.vdot(a, b)

    def new_vector(self):
        return self.torch.zeros(self.n_local, dtype=self.dtype)

    def random_vector(self, seed):
        g = self.torch.Generator().manual_seed(int(seed))
        v = self.torch.rand(self.n_local, dtype=self.torch.float64, generator=g) - 0.5
        if self.dtype == self.torch.complex128:
            v = v + 1j * (self.torch.rand(self.n_local, dtype=self.torch.float64, generator=g) - 0.5)
        return v.to(self.dtype)


@pytest.fixture(scope="module")
def dense():
    """a real symmetric and a complex Hermitian matrix of 600 states with their eigendecompositions"""
    import torch

    rng = np.random.RandomState(7)
    n = 600
    A = rng.randn(n, n)
    A = (A + A.T) / math.sqrt(2.0 * n)
    B = rng.randn(n, n) + 1j * rng.randn(n, n)
    B = (B + B.conj().T) / math.sqrt(4.0 * n)
    out = {}
    for name, M in (("f64", A), ("c128", B)):
        lam, U = np.linalg.eigh(M)
        out[name] = (torch.from_numpy(M), lam, U)
    return out


@pytest.mark.parametrize("name", ["f64", "c128"])
def test_filtered_operator_is_minus_p_of_h(dense, name):
    import torch

    H, lam, U = dense[name]
    bounds = (lam[0] - 0.1, lam[-1] + 0.1)
    op = DenseOperator(H)
    c = kpm.delta_filter(0.3, bounds, 60)
    f = dg.FilteredOperator(op, c, bounds)
    for attr in ("matvec_block", "matvec", "random_vector", "new_vector", "matvecs", "check", "dtype", "n_local", "sizes", "block_kernel",
                 "applications"):
        assert hasattr(f, attr), attr
    assert not hasattr(f, "global_sum")  # (the solver would take it for a distributed operator)
    assert (f.dtype, f.n_local, f.sizes, f.order) == (op.dtype, op.n_local, op.sizes, 60)
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    P = -(U * cheb.chebval((lam - b) / a, c)[None, :]) @ U.conj().T
    rng = np.random.RandomState(3)
    X = rng.randn(op.n_local, 5) + (1j * rng.randn(op.n_local, 5) if name == "c128" else 0.0)
    # column-major views of basis rows: the layout the block solver hands over
    V = torch.from_numpy(np.ascontiguousarray(X.T))
    Y = torch.full_like(V, float("nan"))
    f.matvec_block(V.t(), Y.t())
    want = P @ X
    assert np.abs(Y.t().numpy() - want).max() <= 1e-12 * np.abs(c).sum() * np.abs(X).max() * 60
    assert torch.equal(V, torch.from_numpy(np.ascontiguousarray(X.T)))
    y1 = torch.zeros(op.n_local, dtype=op.dtype)
    f.matvec(V[2], y1)
    assert np.abs(y1.numpy() - want[:, 2]).max() <= 1e-12 * np.abs(c).sum() * np.abs(X).max() * 60
    assert f.applications == 2 and f.matvecs == (5 + 1) * 60 and op.matvecs == f.matvecs
    assert f.block_kernel(5) == "dense"
    with pytest.raises(ValueError, match="one-partition"):
        dg.FilteredOperator(DenseOperator(H, parts=2), c, bounds)
    with pytest.raises(ValueError, match="bounds"):
        dg.FilteredOperator(op, c, (1.0, -1.0))
    with pytest.raises(ValueError, match="coefficients"):
        dg.FilteredOperator(op, [], bounds)


@pytest.mark.parametrize("name,where", [("f64", 0.5), ("f64", 0.25), ("c128", 0.5), ("f64", 0.002)])
def test_interior_eigenpairs_on_the_stand_in(dense, name, where):
    """the whole solver (filter order from the stand-in's own moments, block Lanczos on -p(H), Rayleigh-Ritz against H) finds the
    levels nearest sigma of a dense matrix: mid-band, a quarter of the band, and just inside the lower edge"""
    import torch

    H, lam, U = dense[name]
    eps, k = 1e-9, 6
    bounds = (lam[0] - 0.05, lam[-1] + 0.05)
    h_norm = max(abs(bounds[0]), abs(bounds[1]))
    sigma = lam[0] + where * (lam[-1] - lam[0])
    order = np.argsort(np.abs(lam - sigma))
    sigma += 0.25 * (abs(lam[order[k]] - sigma) - abs(lam[order[k - 1]] - sigma)) * (1.0 if lam[order[k]] < sigma else -1.0)
    near = np.sort(np.argsort(np.abs(lam - sigma))[:k])
    op = DenseOperator(H)
    r = dg.interior_eigenpairs(op, sigma, num_evals=k, eps=eps, block_size=4, bounds=bounds,
                               order=None if where != 0.25 else 300)
    assert r.converged and len(r.eigenvalues) == k and r.eigenvalues == sorted(r.eigenvalues)
    assert np.abs(np.array(r.eigenvalues) - lam[near]).max() <= eps * h_norm
    assert max(r.residual_norms) <= eps * h_norm
    for th, y, res in zip(r.eigenvalues, r.eigenvectors, r.residual_norms):
        assert abs(float(torch.linalg.vector_norm(H @ y - th * y)) - res) <= 1e-12 * h_norm
        assert abs(float(torch.linalg.vector_norm(y)) - 1.0) <= 1e-12
    assert r.sigma == sigma and r.bounds == bounds and r.order >= 2 and (where != 0.25 or r.order == 300)
    assert r.applications == op.plan.series_calls and r.applications >= 1
    assert r.matvecs == op.matvecs and r.matvecs >= r.applications * r.order
    assert r.polish_rounds <= 3 and r.kernel == "dense" and r.seconds > 0.0


def test_an_order_too_small_is_reported_not_raised(dense):
    import torch

    H, lam, U = dense["f64"]
    bounds = (lam[0] - 0.05, lam[-1] + 0.05)
    h_norm = max(abs(bounds[0]), abs(bounds[1]))
    r = dg.interior_eigenpairs(DenseOperator(H), 0.1, num_evals=4, eps=1e-9, block_size=4, bounds=bounds, order=4, max_polish=0)
    assert not r.converged and r.polish_rounds == 0 and len(r.eigenvalues) == 4
    assert max(r.residual_norms) > 1e-9 * h_norm
    for th, y, res in zip(r.eigenvalues, r.eigenvectors, r.residual_norms):
        assert abs(float(torch.linalg.vector_norm(H @ y - th * y)) - res) <= 1e-12 * h_norm
    # one polish round is one more application of the filter to the whole block of num_evals + guard vectors
    r1 = dg.interior_eigenpairs(DenseOperator(H), 0.1, num_evals=4, eps=1e-9, block_size=4, bounds=bounds, order=4, max_polish=1)
    assert not r1.converged and r1.polish_rounds == 1 and r1.applications == r.applications + 1


# ---------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------
def test_interior_refusals_without_a_device(dense):
    H, lam, U = dense["f64"]
    bounds = (lam[0] - 0.05, lam[-1] + 0.05)
    op = DenseOperator(H)
    with pytest.raises(ValueError, match="not Hermitian"):
        dg.interior_eigenpairs(DenseOperator(H, hermitian=False), 0.0, bounds=bounds)
    with pytest.raises(Exception, match="one-partition"):
        dg.interior_eigenpairs(DenseOperator(H, parts=2), 0.0, bounds=bounds)
    with pytest.raises(ValueError, match=r"128"):  # 2 (50 + 12) + 3 * 8 = 148 vectors
        dg.interior_eigenpairs(op, 0.0, num_evals=50, bounds=bounds)
    with pytest.raises(ValueError, match=r"128"):
        dg.interior_eigenpairs(op, 0.0, num_evals=8, max_basis=200, bounds=bounds)
    with pytest.raises(ValueError, match=r"diagonalize\(\)"):
        dg.interior_eigenpairs(op, bounds[1] + 1.0, bounds=bounds)
    with pytest.raises(ValueError, match="order"):
        dg.interior_eigenpairs(op, 0.0, bounds=bounds, order=1)
    with pytest.raises(ValueError, match="block_size"):
        dg.interior_eigenpairs(op, 0.0, bounds=bounds, block_size=17)
    with pytest.raises(ValueError, match="num_evals"):
        dg.interior_eigenpairs(op, 0.0, bounds=bounds, num_evals=0)
    with pytest.raises(ValueError, match="eps"):
        dg.interior_eigenpairs(op, 0.0, bounds=bounds, eps=0.0)
    assert op.matvecs == 0 and op.plan.series_calls == 0
    # a non-Hermitian Hamiltonian from a config: refused when it is loaded, before representatives are enumerated
    cfg = config.heisenberg_chain_config(8)
    cfg["hamiltonian"]["terms"].append({"expression": "σ⁺₀ σ⁻₁", "sites": [[0, 1]]})
    with pytest.raises(ValueError, match="not Hermitian"):
        dg.interior_eigenpairs(cfg, 0.0)
    with pytest.raises(ValueError, match="num_partitions"):
        dg.diagonalize(config.heisenberg_chain_config(8), num_evals=2, num_partitions=2, sigma=0.0)


# ---------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------
def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _vp(a):
    return C.cast(a, C.c_void_p)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_matvec_block_series\s*\(\s*ls_amd_plan\s*\*\s*\w+\s*,\s*int\s+K\s*,\s*int\s+N\s*,\s*double\s+const\s*\*\s*coeffs\s*,"
                     r"\s*double\s+lo\s*,\s*double\s+hi\s*,[^;]*int\s+z_cplx\s*,\s*void\s*\*\s*d_work\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"char\s+const\s*\*\s*ls_amd_plan_series_kernel_name\s*\(\s*ls_amd_plan\s+const\s*\*\s*\w+\s*,\s*int\s+K\s*\)", header)
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    import distributed_matvec_amd as D

    assert callable(D.MatvecPlan.matvec_block_series) and callable(D.MatvecPlan.series_kernel)
    for name in ("chebyshev_series", "delta_filter", "filter_order"):
        assert callable(getattr(kpm, name)), name
    for name in ("FilteredOperator", "interior_eigenpairs", "InteriorResult"):
        assert hasattr(dg, name), name
    # no kernel of its own: the series is a host loop over the accumulate step, so the Makefile lists no new translation unit
    units = re.findall(r"\b(k_\w+|orth\w*|util|repl)\.(?:hip|o)\b", open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile")).read())
    assert not [u for u in units if "series" in u or "interior" in u or "filter" in u]
    integration = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "ls_amd_matvec_block_series" in integration and "matrixMatvec" in integration


def test_series_argument_errors_without_a_device():
    L = _lib()
    x, z = ((C.c_double * 16)() for _ in range(2))
    c = (C.c_double * 8)(1.0, 0.0, 0.5, 0.0, 0.25, 0.0, 0.125, 0.0)

    def call(plan, K=2, N=3, coeffs=c, lo=-1.0, hi=1.0):
        return L.ls_amd_matvec_block_series(plan, K, N, _vp(coeffs) if coeffs is not None else None, lo, hi, _vp(x), 2, 1, _vp(z), 2, 1, 0,
                                            None, None)

    assert call(None) == -1 and "NULL" in L.ls_amd_last_error().decode()
    assert L.ls_amd_plan_series_kernel_name(None, 4) is None and "NULL" in L.ls_amd_last_error().decode()
    fake = C.c_void_p(8)  # a non-NULL handle with K out of range: refused before the plan is dereferenced
    for K in (0, 65, -3):
        assert call(fake, K=K) == -1 and f"K = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_plan_series_kernel_name(fake, K) is None and "[1, 64]" in L.ls_amd_last_error().decode()
