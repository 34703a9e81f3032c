"""Kernel polynomial method, host side (no device): the Jackson kernel, the reconstruction of a curve from moments, the doubling
recurrence against an eigendecomposition, and spectral_bounds / the growth guard on a fake operator made of a dense matrix."""
import math

import numpy as np
import pytest

from distributed_matvec_amd import LsAmdError, kpm
from helpers import model_config
from kpm_reference import eigen_weights, exact_moments, moment_tolerance, recurrence_moments


@pytest.mark.parametrize("M", [2, 16, 255, 1024])
def test_jackson_kernel(M):
    g = kpm.jackson_kernel(M)
    assert g.shape == (M,)
    assert abs(g[0] - 1.0) <= 1e-15
    assert (g > 0).all()
    assert (np.diff(g) < 0).all()


@pytest.mark.parametrize("x0", [0.0, 0.37, -0.8])
def test_reconstruct_one_level(x0):
    M = 64
    bounds = (-3.0, 5.0)
    a, b = 4.0, 1.0
    mu = np.cos(np.arange(M) * math.acos(x0))  # T_n(x0)
    # the Chebyshev grid of 2 M points (kpm.chebyshev_grid: uniform in theta, where f(cos theta) sin theta is a trigonometric
    # polynomial of degree < M): the trapezoid sum in theta is the Gauss-Chebyshev rule, exact up to rounding
    N = 2 * M
    E = kpm.chebyshev_grid(bounds, N)
    theta = np.arccos((E - b) / a)
    f = kpm.reconstruct(mu, bounds, E)
    assert f.shape == E.shape and (f >= 0.0).all()
    integral = float(np.sum(f * a * np.sin(theta)) * math.pi / N)
    assert abs(integral - 1.0) <= 1e-6, integral
    # ... and a plain trapezoid sum in E on a grid fine enough for its second-order error: (h / width)^2 ~ (M / N)^2 / 12
    Nf = 400 * M
    Ef = kpm.chebyshev_grid(bounds, Nf)
    ff = kpm.reconstruct(mu, bounds, Ef)
    assert (ff >= 0.0).all()
    assert abs(float(np.sum(0.5 * (ff[1:] + ff[:-1]) * np.diff(Ef))) - 1.0) <= 1e-5
    peak = (E[np.argmax(f)] - b) / a
    assert abs(math.acos(peak) - math.acos(x0)) <= math.pi / M and abs(peak - x0) <= math.pi / M
    # outside the bounds: zero; several curves at once: one per leading index
    assert (kpm.reconstruct(mu, bounds, np.array([-3.5, -3.0, 5.0, 7.0])) == 0.0).all()
    two = kpm.reconstruct(np.stack([mu, 2.0 * mu]), bounds, E[::3])
    assert two.shape == (2, len(E[::3])) and np.allclose(two[1], 2.0 * two[0]) and np.allclose(two[0], f[::3])


def test_chebyshev_grid_and_moments_from_dots():
    E = kpm.chebyshev_grid((-1.0, 3.0), 8)
    assert (np.diff(E) > 0).all() and E[0] > -1.0 and E[-1] < 3.0
    assert np.allclose(E, 1.0 + 2.0 * np.cos(math.pi * (np.arange(8) + 0.5) / 8)[::-1])
    dots = np.array([[2.0, 3.0, 0.5, 0.25], [1.5, 2.5, 0.1, 0.2], [1.0, 2.0, 0.3, 0.4]])  # 3 steps, K = 2
    mu = kpm.moments_from_dots(dots, 2, 5)
    assert mu.shape == (2, 5)
    assert np.array_equal(mu[0], [2.0, 0.5, 2 * 1.5 - 2.0, 2 * 0.1 - 0.5, 2 * 1.0 - 2.0])
    assert np.array_equal(mu[1], [3.0, 0.25, 2 * 2.5 - 3.0, 2 * 0.2 - 0.25, 2 * 2.0 - 3.0])


@pytest.mark.parametrize("name", ["heisenberg_chain_8", "heisenberg_kagome_12_symm", "heisenberg_chain_12"])
def test_doubling_recurrence_matches_the_eigendecomposition(name):
    from oracle import model as M

    _, H = M.dense_sector_matrix(model_config(name))
    H = np.asarray(H)
    assert np.abs(H - H.conj().T).max() <= 1e-12
    if np.abs(H.imag).max() <= 1e-13:
        H = np.ascontiguousarray(H.real)
    rs = np.random.RandomState(5)
    v0 = rs.rand(len(H), 3) - 0.5
    ev = np.linalg.eigvalsh(H)
    w = ev[-1] - ev[0]
    bounds = (ev[0] - 0.01 * w, ev[-1] + 0.01 * w)
    evals, weights = eigen_weights(H, v0)
    for Mn in (7, 512):
        exact = exact_moments(evals, weights, Mn, bounds)
        got = recurrence_moments(H, v0, Mn, bounds)
        assert got.shape == exact.shape == (3, Mn)
        # 2^-53 per operation, a few operations per element and step, growing at most linearly in the steps
        assert np.abs(got - exact).max() <= 1e-12 * exact[:, 0].max(), np.abs(got - exact).max()
        tol, own = moment_tolerance(H, v0, Mn, bounds, exact)
        assert (tol >= 1e-13 * exact[:, 0]).all() and (tol >= 100 * own).all()


class DenseOperator:
    """the operator interface of lanczos_smallest / spectral_bounds on a dense numpy matrix (CPU torch vectors)"""

    def __init__(self, H):
        import torch

        self.torch = torch
        self.H = torch.from_numpy(np.ascontiguousarray(H))
        self.dtype = self.H.dtype
        self.n_local = len(H)
        self.sizes = [len(H)]
        self.matvecs = 0

    def matvec(self, x, y):
        y.copy_(self.H @ x)
        self.matvecs += 1

    def check(self):
        pass

    def dot(self, a, b):
        return self.torch.vdot(a, b)

    def new_vector(self):
        return self.torch.zeros(self.n_local, dtype=self.dtype)

    def random_vector(self, seed):
        g = self.torch.Generator().manual_seed(seed)
        return self.torch.rand(self.n_local, dtype=self.torch.float64, generator=g).to(self.dtype) - 0.5


class DensePlan:
    """MatvecPlan.matvec_block_axpby as the C entry specifies it, on the dense matrix of a DenseOperator (CPU torch)"""

    def __init__(self, op):
        self.op = op
        self.calls = []

    def matvec_block_axpby(self, x, y, alpha, beta, gamma, dots=None, check=True):
        torch = self.op.torch
        assert x.data_ptr() != y.data_ptr() and not check
        new = alpha * (self.op.H @ x) + beta * x
        if gamma != 0.0:
            new = new + gamma * y
        y.copy_(new)  # (gamma == 0: y is not read)
        if dots is not None:
            K = x.shape[1]
            dots[:K] = (x.conj() * x).real.sum(0)
            dots[K:] = (x.conj() * y).real.sum(0)
        self.calls.append((alpha, beta, gamma))

    def check(self):
        pass


def test_chebyshev_moments_driver_on_a_dense_plan():
    """the recurrence, the doubling, the block swap and the guard of kpm.chebyshev_moments, with the step done by torch on the CPU"""
    import torch

    rs = np.random.RandomState(4)
    for cplx in (False, True):
        A = rs.rand(150, 150) - 0.5 + (1j * (rs.rand(150, 150) - 0.5) if cplx else 0)
        H = 0.5 * (A + A.conj().T)
        ev = np.linalg.eigvalsh(H)
        w = ev[-1] - ev[0]
        bounds = (ev[0] - 0.01 * w, ev[-1] + 0.01 * w)
        V0 = rs.rand(150, 3) - 0.5 + (1j * (rs.rand(150, 3) - 0.5) if cplx else 0)
        op = DenseOperator(H)
        op.plan = DensePlan(op)
        start = torch.from_numpy(V0.copy())
        evals, weights = eigen_weights(H, V0)
        for M in (2, 9, 200, 300):  # fewer than, and more than, one guard interval of steps
            op.plan.calls.clear()
            before = op.matvecs
            got = kpm.chebyshev_moments(op, start, M, bounds)
            steps = (M + 1) // 2
            assert got.shape == (3, M) and got.dtype == np.float64 and op.matvecs - before == 3 * steps
            a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
            assert op.plan.calls[0] == (1.0 / a, -b / a, 0.0) and all(c == (2.0 / a, -2.0 * b / a, -1.0) for c in op.plan.calls[1:])
            assert len(op.plan.calls) == steps
            exact = exact_moments(evals, weights, M, bounds)
            tol, _ = moment_tolerance(H, V0, M, bounds, exact)
            assert (np.abs(got - exact).max(axis=1) <= tol).all()
            assert np.array_equal(start.numpy(), V0)  # the caller's block is left alone
        mid = 0.5 * (ev[0] + ev[-1])
        before = op.matvecs
        with pytest.raises(LsAmdError, match=r"step \d+ .*not inside the bounds") as info:
            kpm.chebyshev_moments(op, start, 512, (mid - 0.25 * w, mid + 0.25 * w))
        assert int(str(info.value).split("step ")[1].split()[0]) < kpm.GUARD_EVERY
        assert op.matvecs - before == 3 * kpm.GUARD_EVERY  # stopped at the first read-back


@pytest.mark.parametrize("kind", ["real", "complex", "shifted"])
def test_spectral_bounds_enclose_the_spectrum(kind):
    rs = np.random.RandomState(11)
    A = rs.rand(300, 300) - 0.5
    if kind == "complex":
        A = A + 1j * (rs.rand(300, 300) - 0.5)
    H = 0.5 * (A + A.conj().T)
    if kind == "shifted":
        H = H + 40.0 * np.eye(300)  # all levels positive: the run on -H must still find the top
    ev = np.linalg.eigvalsh(H)
    op = DenseOperator(H)
    lo, hi = kpm.spectral_bounds(op)
    width = ev[-1] - ev[0]
    assert lo < ev[0] and hi > ev[-1]
    assert ev[0] - lo <= 0.02 * width and hi - ev[-1] <= 0.02 * width  # Ritz values at eps = 1e-3, widened by 1 %
    assert op.matvecs > 0
    neg = kpm._Negated(op)
    x = op.random_vector(1)
    y, z = op.new_vector(), op.new_vector()
    neg.matvec(x, y)
    op.matvec(x, z)
    assert op.torch.equal(y, -z) and neg.n_local == 300


def test_guard_logic():
    # norms that stay below mu_0 pass, whatever the second half (the <v_n|v_n+1>) holds
    ok = np.array([[4.0, 9.0, -3.0, 50.0], [3.9, 9.0 * (1 + 5e-7), 100.0, -100.0], [0.0, 1.0, 0.0, 0.0]])
    kpm.check_guard(ok, 2, (-1.0, 1.0))
    grow = ok.copy()
    grow[2, 1] = 9.0 * (1 + 2e-6)
    with pytest.raises(LsAmdError, match=r"step 7.*not inside the bounds \(-1\.5, 2\.5\)"):
        kpm.check_guard(grow, 2, (-1.5, 2.5), first_step=5)
    nan = ok.copy()
    nan[1, 0] = float("nan")
    with pytest.raises(LsAmdError, match="step 1"):
        kpm.check_guard(nan, 2, (-1.0, 1.0))
    # the recurrence itself: inside the bounds the norms obey the guard, with bounds half as wide they break it within 64 steps
    rs = np.random.RandomState(2)
    A = rs.rand(120, 120) - 0.5
    H = 0.5 * (A + A.T)
    ev = np.linalg.eigvalsh(H)
    v0 = rs.rand(120, 2) - 0.5

    def norms(bounds, steps):
        a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
        rows, prev, cur = [], None, v0
        for n in range(steps):
            nxt = (H @ cur - b * cur) / a if n == 0 else 2.0 * (H @ cur - b * cur) / a - prev
            rows.append(np.concatenate([(cur * cur).sum(0), (cur * nxt).sum(0)]))
            prev, cur = cur, nxt
        return np.array(rows)

    w = ev[-1] - ev[0]
    kpm.check_guard(norms((ev[0] - 0.01 * w, ev[-1] + 0.01 * w), 64), 2, (0, 0))
    mid = 0.5 * (ev[0] + ev[-1])
    with pytest.raises(LsAmdError, match="not inside the bounds"):
        kpm.check_guard(norms((mid - 0.25 * w, mid + 0.25 * w), 64), 2, (mid - 0.25 * w, mid + 0.25 * w))


def test_bad_arguments_are_refused_before_any_device_work():
    op = DenseOperator(np.eye(4))
    import torch

    start = torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(ValueError, match="num_moments"):
        kpm.chebyshev_moments(op, start, 1, (-1.0, 1.0))
    for bounds in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="bounds"):
            kpm.chebyshev_moments(op, start, 8, bounds)
    with pytest.raises(LsAmdError, match=r"\(4, K\)"):
        kpm.chebyshev_moments(op, torch.zeros((5, 2), dtype=torch.float64), 8, (-1.0, 1.0))
    op.sizes = [2, 2]
    with pytest.raises(LsAmdError, match="one-partition"):
        kpm.chebyshev_moments(op, start, 8, (-1.0, 1.0))
