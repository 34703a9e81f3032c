"""Chebyshev time evolution without a device: the Bessel series behind the coefficients against scipy, the truncation rule, the
closed forms of the first coefficients and the prefactors, autocorrelation() from exact moments against the eigendecomposition, and
the refusals that need no device."""
import cmath
import math
import types

import numpy as np
import pytest
import scipy.special as special
import torch

import distributed_matvec_amd as D
from distributed_matvec_amd import evolve as E
from evolve_reference import exact_propagate, propagate_tolerance, series_propagate
from kpm_reference import exact_moments

XS = [0.0, 1e-3, 1.0, 37.5, 1000.0, 5000.0]


@pytest.mark.parametrize("x", XS)
def test_bessel_values_against_scipy(x):
    f = E.bessel_series(x, 1e-12)
    g = E.bessel_series(x, 1e-12, modified=True)
    dj = np.abs(f - special.jv(np.arange(len(f)), x)).max()
    di = np.abs(g - special.ive(np.arange(len(g)), x)).max()
    print(f"bessel_series x = {x}: N_J = {len(f) - 1}, max |dJ| = {dj:.3e}; N_I = {len(g) - 1}, max |dI| = {di:.3e}")
    assert dj <= 1e-12 and di <= 1e-12
    if x == 0.0:
        assert f.tolist() == [1.0] and g.tolist() == [1.0]
    else:
        h = E.bessel_series(-x, 1e-12)  # J_n(-x) = (-1)^n J_n(x)
        assert len(h) == len(f) and np.array_equal(h, f * (-1.0) ** np.arange(len(f)))


@pytest.mark.parametrize("modified", [False, True])
@pytest.mark.parametrize("x", [1e-3, 1.0, 37.5, 1000.0])
@pytest.mark.parametrize("eps", [1e-6, 1e-12])
def test_tail_is_below_eps_and_the_order_is_minimal(x, eps, modified):
    f = E.bessel_series(x, eps, modified)
    full = E.bessel_series(x, 1e-300, modified)  # (every order that is not zero in double precision)
    N = len(f) - 1
    assert len(full) > len(f) and np.array_equal(full[:N + 1], f)
    tail = lambda n: 2.0 * np.abs(full[n + 1:]).sum()  # noqa: E731
    assert tail(N) <= eps
    assert N == 0 or tail(N - 1) > eps


def test_bessel_series_refuses_bad_arguments():
    with pytest.raises(ValueError, match="eps"):
        E.bessel_series(1.0, 0.0)
    with pytest.raises(ValueError, match="finite"):
        E.bessel_series(float("inf"), 1e-12)
    with pytest.raises(ValueError, match="negative"):
        E.bessel_series(-1.0, 1e-12, modified=True)


def test_coefficients_match_the_closed_forms():
    lo, hi = -3.0, 5.0
    a, b = 0.5 * (hi - lo), 0.5 * (hi + lo)
    for t in (0.7, -0.7, 12.5):
        c, pref = E.propagator_coefficients(t, (lo, hi))
        assert c.dtype == np.complex128
        want = [special.jv(0, a * t), -2j * special.jv(1, a * t), -2.0 * special.jv(2, a * t), 2j * special.jv(3, a * t)]
        assert np.abs(c[:4] - np.array(want)).max() <= 1e-14
        assert abs(pref - cmath.exp(-1j * b * t)) <= 1e-15
    cp, _ = E.propagator_coefficients(0.7, (lo, hi))
    cm, pm = E.propagator_coefficients(-0.7, (lo, hi))
    assert np.array_equal(cm, cp.conj()) and abs(pm - cmath.exp(0.7j * b)) <= 1e-15  # e^{+iHt} is the conjugate series
    tau = 1.3
    c, pref = E.propagator_coefficients(tau, (lo, hi), imaginary=True)
    assert c.dtype == np.float64 and pref == 1.0  # E_ref = lo
    want = [special.ive(0, a * tau), -2.0 * special.ive(1, a * tau), 2.0 * special.ive(2, a * tau), -2.0 * special.ive(3, a * tau)]
    assert np.abs(c[:4] - np.array(want)).max() <= 1e-14
    c2, pref2 = E.propagator_coefficients(tau, (lo, hi), imaginary=True, reference_energy=-2.5)
    assert np.array_equal(c2, c) and abs(pref2 - math.exp(-(lo + 2.5) * tau)) <= 1e-15 * pref2
    c0, p0 = E.propagator_coefficients(0.0, (lo, hi))
    assert c0.tolist() == [1.0] and p0 == 1.0
    # the scalar identity the series rests on: sum_n c_n T_n(x) = e^{-i a t x}
    c, _ = E.propagator_coefficients(2.0, (lo, hi))
    xs = np.linspace(-1.0, 1.0, 41)
    T = np.cos(np.arange(len(c))[:, None] * np.arccos(xs)[None, :])
    assert np.abs(c @ T - np.exp(-1j * a * 2.0 * xs)).max() <= 1e-12
    with pytest.raises(ValueError, match="t >= 0"):
        E.propagator_coefficients(-1.0, (lo, hi), imaginary=True)


@pytest.fixture(scope="module")
def random_symmetric():
    rs = np.random.RandomState(5)
    A = rs.rand(400, 400) - 0.5
    H = 0.5 * (A + A.T)
    evals, U = np.linalg.eigh(H)
    w = evals[-1] - evals[0]
    return H, evals, U, (float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w))


def test_series_reference_agrees_with_the_eigendecomposition(random_symmetric):
    H, evals, U, bounds = random_symmetric
    psi = np.random.RandomState(6).rand(400, 2) - 0.5
    for t, imag in ((0.3, False), (7.0, False), (-7.0, False), (2.0, True)):
        tol, own = propagate_tolerance(H, psi, t, bounds, imaginary=imag)
        assert (own <= 1e-11 * np.linalg.norm(psi, axis=0)).all(), (t, imag, own)  # eps = 1e-12 and rounding
        got = series_propagate(H, psi, t, bounds, imaginary=imag)
        assert np.abs(got - exact_propagate(H, psi, t, imag, bounds[0])).max() <= tol.max()


def test_autocorrelation_from_exact_moments(random_symmetric):
    H, evals, U, bounds = random_symmetric
    v0 = np.random.RandomState(7).rand(400) - 0.5
    w = np.abs(U.T @ v0) ** 2
    times = np.array([0.0, 0.3, 7.0, 20.0])
    M = len(E.propagator_coefficients(times[-1], bounds)[0])
    mu = exact_moments(evals, w, M, bounds)
    got = E.autocorrelation(mu, bounds, times)
    want = np.array([(w * np.exp(-1j * evals * t)).sum() for t in times])
    assert got.shape == (4,) and got.dtype == np.complex128
    for j, t in enumerate(times):
        tol, _ = propagate_tolerance(H, v0, t, bounds)
        bound = tol[0]  # the tolerance of the propagated vector itself
        print(f"autocorrelation t = {t}: deviation {abs(got[j] - want[j]):.3e}, bound {bound:.3e}")
        assert abs(got[j] - want[j]) <= bound
    both = E.autocorrelation(np.stack([mu, 2.0 * mu]), bounds, times)
    assert both.shape == (2, 4) and np.allclose(both[1], 2.0 * got, rtol=0, atol=1e-13)
    with pytest.raises(ValueError, match="moments"):
        E.autocorrelation(mu[:M - 1], bounds, times)
    with pytest.raises(ValueError, match="bounds"):
        E.autocorrelation(mu, (1.0, 1.0), times)


def fake_operator(hermitian=True, partitions=1, dtype=torch.float64, n=10):
    """what propagate looks at before it touches the device"""
    plan = types.SimpleNamespace(matrix=types.SimpleNamespace(isHermitian=hermitian))
    return types.SimpleNamespace(plan=plan, sizes=[n] * partitions, n_local=n * partitions, dtype=dtype, matvecs=0)


def test_loud_failures_before_the_device():
    x = torch.zeros(10, dtype=torch.float64)
    for bad in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (0.0, float("inf"))):
        with pytest.raises(ValueError, match="bounds"):
            E.propagate(fake_operator(), x, 1.0, bounds=bad)
        with pytest.raises(ValueError, match="bounds"):
            E.propagator_coefficients(1.0, bad)
    with pytest.raises(D.LsAmdError, match="K = 65"):
        E.propagate(fake_operator(), torch.zeros((10, 65), dtype=torch.float64), 1.0, bounds=(-1.0, 1.0))
    with pytest.raises(ValueError, match="not Hermitian"):
        E.propagate(fake_operator(hermitian=False), x, 1.0, bounds=(-1.0, 1.0))
    with pytest.raises(D.LsAmdError, match="one-partition"):
        E.propagate(fake_operator(partitions=2), torch.zeros(20, dtype=torch.float64), 1.0, bounds=(-1.0, 1.0))
    with pytest.raises(D.LsAmdError, match="complex128"):
        E.propagate(fake_operator(), x.to(torch.complex128), 1.0, bounds=(-1.0, 1.0))
    with pytest.raises(D.LsAmdError, match="rows"):
        E.propagate(fake_operator(), torch.zeros(11, dtype=torch.float64), 1.0, bounds=(-1.0, 1.0))
    with pytest.raises(ValueError, match="ascending"):
        E.evolve({}, x, [1.0, 0.5])
    assert D.propagate is E.propagate and D.autocorrelation is E.autocorrelation and callable(D.evolve.evolve)
