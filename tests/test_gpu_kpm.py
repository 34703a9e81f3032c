"""Kernel polynomial method on the GPU: the Chebyshev step (MatvecPlan.matvec_block_axpby, ls_amd_matvec_block_axpby) on every path
-- k_direct_cheb, resolve + k_pull_gather_cheb, the column loop with the k_axpby_dots epilogue -- against references that do not
use this library's matvec (the C oracle, dense sector matrices, dense Jordan-Wigner matrices); the bare epilogue against numpy;
Chebyshev moments, an exact trace and a spectral function against eigendecompositions; and the failures that must be loud."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import config, kpm
from distributed_matvec_amd.diagonalize import LocalOperator
from fermion_jw import ring
from fermion_symm import closure, dihedral, projected_matrix, representatives, tv_model
from helpers import complex_translation_config, model_config
from kpm_reference import exact_moments, moment_tolerance
from test_gpu_block_matvec import device_block, hop_chain_config, hubbard_nonseparable, random_block, spinless_ring
from test_gpu_fermion_symm import cfg_of

pytestmark = pytest.mark.gpu

KS = [1, 2, 5, 8, 11, 64]
LAYOUTS = ["interleaved", "colmajor", "colmajor_ld"]
MODES = ["auto", "kernel", "columns"]
CHEB = {"k_direct_blk": "k_direct_cheb", "k_pull_gather_blk": "k_pull_gather_cheb", "columns": "epilogue"}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def fermion_sector():
    """a projected spinless-fermion sector with +-1 characters: the permutation sign rides in the packets' coefficients"""
    L, N, gens, secs = 12, 5, dihedral(12), [6, 1]
    model = tv_model(ring(L), V=1.1)
    group = closure(L, gens, secs)
    reps, _ = representatives(L, N, group)
    Hs = projected_matrix(model, L, N, group, reps)
    assert np.abs(Hs.imag).max() <= 1e-14
    return cfg_of(L, N, gens, secs, model), np.ascontiguousarray(Hs.real), reps


def searched_subset():
    """the weight-6 states of the 12-site chain handed to a plan of the basis WITHOUT a fixed weight: neither the identity nor the
    combinadic rank applies, the partners are found by search; H conserves the weight, so the subset is closed"""
    from oracle import model as M

    cfg = model_config("heisenberg_chain_12")
    states, H = M.dense_sector_matrix(cfg)
    keep = np.array([i for i, s in enumerate(states) if bin(int(s)).count("1") == 6])
    return cfg, np.ascontiguousarray(np.asarray(H)[np.ix_(keep, keep)].real), states[keep]


def oracle_apply(make):
    from oracle import c_oracle as CO
    from oracle import model as M

    o = CO.COracle(M.model_from_config(make()))
    reps = o.enumerate()
    return reps, lambda X: np.stack([o.local_matvec(reps, np.ascontiguousarray(X[:, k])) for k in range(X.shape[1])], axis=1)


def dense_apply(triple):
    _, H, states = triple
    return np.asarray(states, dtype=np.uint64), lambda X: H @ X


def sector_apply(make):
    from oracle import model as M

    reps, H = M.dense_sector_matrix(make())
    H = np.asarray(H)
    return reps, lambda X: H @ X


# name -> (config, dtype, reference (representatives, X -> H X), path `auto` takes for K >= 2 (None: whatever the block matvec takes
# there), plan options)
@functools.lru_cache(maxsize=None)
def cases():
    kagome = lambda: model_config("heisenberg_kagome_12_symm")  # noqa: E731
    momentum = lambda: complex_translation_config(12, 5)  # noqa: E731
    inversion = lambda: config.heisenberg_chain_config(12, spin_inversion=-1)  # noqa: E731
    chain24 = lambda: model_config("heisenberg_chain_24_symm")  # noqa: E731
    chain16 = lambda: model_config("heisenberg_chain_16")  # noqa: E731
    return {
        # k_direct_cheb: combinadic (f64, c128), combinadic over fermionic modes, identity, product, searched
        "hop_chain_12/f64": (lambda: hop_chain_config(12), "f64", lambda: oracle_apply(lambda: hop_chain_config(12)), "k_direct_cheb", {}),
        "hop_chain_12/c128": (lambda: hop_chain_config(12), "c128", lambda: oracle_apply(lambda: hop_chain_config(12)), "k_direct_cheb", {}),
        "spinless_ring_9_4/f64": (lambda: spinless_ring(9, 4)[0], "f64", lambda: dense_apply(spinless_ring(9, 4)), "k_direct_cheb", {}),
        "spinless_ring_8_all/f64": (lambda: spinless_ring(8, -1)[0], "f64", lambda: dense_apply(spinless_ring(8, -1)), "k_direct_cheb", {}),
        "hubbard_pair_hop_6/c128": (lambda: hubbard_nonseparable()[0], "c128", lambda: dense_apply(hubbard_nonseparable()), "k_direct_cheb", {}),
        "chain_12_weight_6_searched/f64": (lambda: searched_subset()[0], "f64", lambda: dense_apply(searched_subset()), None,
                                           {"subset": True}),
        # k_pull_gather_cheb: real and complex characters, a fermionic sector; a partial slot cache; a chunked resolve
        "heisenberg_chain_24_symm/f64": (chain24, "f64", lambda: oracle_apply(chain24), "k_pull_gather_cheb", {}),
        "heisenberg_chain_24_symm/f64/half_cached": (chain24, "f64", lambda: oracle_apply(chain24), "k_pull_gather_cheb", {"cache": 0.5}),
        "heisenberg_chain_24_symm/f64/chunked": (chain24, "f64", lambda: oracle_apply(chain24), "k_pull_gather_cheb",
                                                 {"resolve_bytes": 1 << 18}),
        "heisenberg_kagome_12_symm/c128": (kagome, "c128", lambda: sector_apply(kagome), "k_pull_gather_cheb", {}),
        "momentum_12_5/c128": (momentum, "c128", lambda: oracle_apply(momentum), "k_pull_gather_cheb", {}),
        "fermion_ring_12_dihedral_odd/f64": (lambda: fermion_sector()[0], "f64", lambda: dense_apply(fermion_sector()), "k_pull_gather_cheb", {}),
        # epilogue: the staged chain kernel, a spin-inversion sector, a push-mode plan
        "heisenberg_chain_16/f64": (chain16, "f64", lambda: oracle_apply(chain16), "epilogue", {}),
        "chain_12_inversion/f64": (inversion, "f64", lambda: oracle_apply(inversion), "epilogue", {}),
        "hop_chain_12/f64/push": (lambda: hop_chain_config(12), "f64", lambda: oracle_apply(lambda: hop_chain_config(12)), "epilogue",
                                  {"mode": "push"}),
    }


_plans = {}


def plan_of(torch, name):
    """(plan, representatives, dtype, X -> H X); built once per case"""
    if name not in _plans:
        make, dt, ref, _, opts = cases()[name]
        dtype = torch.complex128 if dt == "c128" else torch.float64
        want_reps, apply = ref()
        basis, h = D.loadConfigFromDict(make(), hamiltonian=True)
        if opts.get("subset"):
            reps = [torch.from_numpy(np.asarray(want_reps, dtype=np.uint64).view(np.int64).copy()).cuda()]
        else:
            reps, _ = D.enumerateStates(basis, 1)
            assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), want_reps), name
        pl = D.MatvecPlan(h, reps, dtype, mode=opts.get("mode", "auto"))
        n = reps[0].numel()
        if "cache" in opts:
            probe = D.MatvecPlan(h, reps, dtype)
            assert probe.cache_slots(0) == n
            rows = pl.cache_slots(int(probe.slot_cache[1] * opts["cache"]))
            probe.destroy()
            assert 0 < rows < n, (rows, n)
            x = torch.ones(n, dtype=dtype, device="cuda")
            pl.matvec([x], [torch.zeros_like(x)])  # the first matvec resolves the cached streams
            assert pl.slot_cache[0] == rows
        _plans[name] = (pl, reps, dtype, apply, h)
    return _plans[name]


def coefficient_sets(want):
    """(alpha, beta, gamma): the plain matvec, a step without Y, and the Chebyshev step for bounds around the block's scale"""
    a = max(1.0, float(np.abs(want).max()))
    b = 0.3 * a
    return [(1.0, 0.0, 0.0), (0.37, -1.2, 0.0), (2.0 / a, -2.0 * b / a, -1.0)]


def assert_close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


def assert_dots(dots, X, Ynew, what):
    """[k] = <X_k|X_k>, [K + k] = Re <X_k|Y_k> from the X given and the Y returned; no summation order is prescribed:
    1e-12 of the sum of the summands' magnitudes"""
    K = X.shape[1]
    xx = (np.abs(X) ** 2).sum(axis=0)
    terms = (X.conj() * Ynew).real
    xy = terms.sum(axis=0)
    assert dots.shape == (2 * K,)
    assert (np.abs(dots[:K] - xx) <= 1e-12 * xx).all(), (what, "xx", np.abs(dots[:K] - xx).max())
    assert (np.abs(dots[K:] - xy) <= 1e-12 * np.abs(terms).sum(axis=0)).all(), (what, "xy", np.abs(dots[K:] - xy).max())


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(cases()))
def test_step_matches_independent_reference(torch, monkeypatch, name, K):
    _, _, _, auto_path, opts = cases()[name]
    pl, reps, dtype, apply, _ = plan_of(torch, name)
    if "resolve_bytes" in opts:
        monkeypatch.setenv("LS_AMD_BLOCK_RESOLVE_BYTES", str(opts["resolve_bytes"]))
    n = reps[0].numel()
    X = random_block(torch, n, K, dtype, 11 + K)
    Y0 = random_block(torch, n, K, dtype, 31 + K)
    HX = apply(X)
    for mode in MODES:
        monkeypatch.setenv("LS_AMD_BLOCK", mode)
        path = pl.axpby_kernel(K)
        assert path == CHEB[pl.block_kernel(K)]
        if mode == "columns" or (mode == "auto" and K == 1):
            assert path == "epilogue", (name, mode, K)
        elif auto_path is None:
            pass
        elif mode == "auto":
            assert path == auto_path, (name, K, path)
        elif auto_path != "epilogue":
            assert path == auto_path, (name, mode, K, path)
        for layout in LAYOUTS:
            for ci, (al, be, ga) in enumerate(coefficient_sets(HX)):
                want = al * HX + be * X + (ga * Y0 if ga != 0.0 else 0.0)
                x = device_block(torch, X, layout, dtype)
                x0 = x.clone()
                y = device_block(torch, Y0, layout, dtype) if ga != 0.0 else device_block(torch, X, layout, dtype, fill=float("nan"))
                dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda") if ci != 1 else None
                pl.matvec_block_axpby(x, y, al, be, ga, dots=dots)
                got = y.cpu().numpy()
                what = (name, K, mode, path, layout, (al, be, ga))
                assert np.isfinite(got).all(), what  # gamma == 0: Y was not read
                assert torch.equal(x, x0), what  # X is left alone
                assert_close(got, want, what)
                if dots is not None:
                    assert_dots(dots.cpu().numpy(), X, got, what)


def test_chunked_resolve_and_partial_cache_take_several_launches(torch, monkeypatch):
    """the two special plans really are what their names say: several resolve chunks, cached rows next to resolved ones"""
    pl, reps, _, _, _ = plan_of(torch, "heisenberg_chain_24_symm/f64/half_cached")
    rows, _ = pl.slot_cache
    assert 0 < rows < reps[0].numel() and rows % 256 == 0
    # the exact packet streams of the whole basis are more than four times the 256 KiB the chunked plan may resolve at once
    pl2, reps2, _, _, _ = plan_of(torch, "heisenberg_chain_24_symm/f64/chunked")
    probe = D.MatvecPlan(plan_of(torch, "heisenberg_chain_24_symm/f64")[4], reps2, torch.float64)
    assert probe.cache_slots(0) == reps2[0].numel() and probe.slot_cache[1] > 4 * cases()["heisenberg_chain_24_symm/f64/chunked"][4]["resolve_bytes"]
    probe.destroy()


@pytest.mark.parametrize("dt", ["f64", "c128"])
@pytest.mark.parametrize("K", KS)
def test_bare_epilogue_against_numpy(torch, dt, K):
    dtype = torch.complex128 if dt == "c128" else torch.float64
    for n in (1, 2, 255, 4099, 4100):  # (odd and even: the 16-byte column-major form needs even column strides, and has a tail row)
        W, X, Y0 = (random_block(torch, n, K, dtype, s + K + n) for s in (1, 2, 3))
        for lw, lx, ly in [(a, a, a) for a in LAYOUTS] + [("interleaved", "colmajor", "colmajor_ld"), ("colmajor_ld", "interleaved", "colmajor")]:
            for al, be, ga in ((1.0, 0.0, 0.0), (0.37, -1.2, 0.0), (1.7, -0.6, -1.0)):
                w, x = device_block(torch, W, lw, dtype), device_block(torch, X, lx, dtype)
                w0, x0 = w.clone(), x.clone()
                y = device_block(torch, Y0, ly, dtype) if ga != 0.0 else device_block(torch, Y0, ly, dtype, fill=float("nan"))
                dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
                D.block_axpby_dots(w, x, y, al, be, ga, dots=dots)
                got = y.cpu().numpy()
                what = (dt, K, n, lw, lx, ly, ga)
                assert np.isfinite(got).all(), what
                assert torch.equal(w, w0) and torch.equal(x, x0), what
                assert_close(got, al * W + be * X + (ga * Y0 if ga != 0.0 else 0.0), what)
                assert_dots(dots.cpu().numpy(), X, got, what)
                if ga == 0.0:
                    y2 = device_block(torch, Y0, ly, dtype, fill=float("nan"))
                    D.block_axpby_dots(w, x, y2, al, be, ga)  # dots=None
                    assert torch.equal(y2, y), what


# ---------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(config, dtype name, dense sector matrix, eigenvalues, eigenvectors, representatives)"""
    from oracle import model as M

    if name == "fermion_ring_12_dihedral_odd":
        cfg, H, reps = fermion_sector()
        dt = "f64"
    else:
        cfg = complex_translation_config(12, 5) if name == "momentum_12_5" else model_config(name)
        reps, H = M.dense_sector_matrix(cfg)
        H = np.asarray(H)
        dt = "c128" if np.abs(H.imag).max() > 1e-13 or name == "heisenberg_kagome_12_symm" else "f64"
        if dt == "f64":
            H = np.ascontiguousarray(H.real)
    evals, U = np.linalg.eigh(H)
    return cfg, dt, H, evals, U, np.asarray(reps, dtype=np.uint64)


def widened(evals):
    w = evals[-1] - evals[0]
    return float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w)


def check_moments(got, H, evals, U, V0, M, bounds, what):
    """got [K, M] against sum_j |<j|v0_k>|^2 T_n(E~_j) under the rule of kpm_reference.moment_tolerance"""
    weights = (np.abs(U.conj().T @ V0) ** 2).T
    exact = exact_moments(evals, weights, M, bounds)
    tol, own = moment_tolerance(H, V0, M, bounds, exact)
    dev = np.abs(got - exact).max(axis=1)
    print(f"kpm moments {what}: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}, mu_0 {exact[:, 0].max():.3e}")
    assert got.shape == exact.shape
    assert (dev <= tol).all(), (what, dev, tol)


@pytest.mark.parametrize("name", ["heisenberg_chain_12", "heisenberg_chain_16", "heisenberg_kagome_12_symm", "momentum_12_5",
                                  "fermion_ring_12_dihedral_odd"])
def test_chebyshev_moments_match_the_eigendecomposition(torch, name):
    cfg, dt, H, evals, U, want_reps = dense_case(name)
    dtype = torch.complex128 if dt == "c128" else torch.float64
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), want_reps)
    op = LocalOperator(h, reps, dtype)
    K, M = 3, 512
    V0 = random_block(torch, len(evals), K, dtype, 17)
    bounds = widened(evals)
    start = torch.from_numpy(np.ascontiguousarray(V0)).to(dtype).cuda()
    got = kpm.chebyshev_moments(op, start, M, bounds)
    assert got.dtype == np.float64 and op.matvecs == K * (M // 2)
    check_moments(got, H, evals, U, V0, M, bounds, (name, op.plan.axpby_kernel(K)))
    assert np.array_equal(start.cpu().numpy(), V0)  # the start block is left alone


def test_exact_trace_on_twenty_states(torch):
    cfg, dt, H, evals, U, _ = dense_case("heisenberg_chain_6")
    n = len(evals)
    assert n == 20 and dt == "f64"
    bounds = widened(evals)
    M = 512
    E, rho, res = kpm.density_of_states(cfg, num_moments=M, bounds=bounds, start=torch.eye(n, dtype=torch.float64, device="cuda"))
    assert res.moments.shape == (n, M) and res.bounds == bounds and res.matvec_columns == n * (M // 2)
    assert res.kernel in ("k_direct_cheb", "epilogue")  # (whichever row kernel the 20-state plan took)
    check_moments(res.moments, H, evals, U, np.eye(n), M, bounds, "unit vectors of heisenberg_chain_6")
    exact = exact_moments(evals, np.full(n, 1.0 / n), M, bounds)
    tol, _ = moment_tolerance(H, np.eye(n), M, bounds, exact_moments(evals, (np.abs(U.conj().T) ** 2).T, M, bounds))
    assert np.abs(res.trace_moments - exact).max() <= tol.max()
    assert E.shape == rho.shape == (2 * M,) and (rho >= 0).all()
    theta = np.arccos((E - 0.5 * (bounds[0] + bounds[1])) / (0.5 * (bounds[1] - bounds[0])))
    assert abs(np.sum(rho * 0.5 * (bounds[1] - bounds[0]) * np.sin(theta)) * np.pi / len(E) - 1.0) <= 1e-6
    # a stochastic trace runs through the same code with generated vectors (and finds its own bounds)
    E2, rho2, res2 = kpm.density_of_states(cfg, num_moments=64, num_vectors=4, seed=3)
    assert res2.moments.shape == (4, 64) and np.allclose(res2.moments[:, 0], n) and res2.bounds[0] < evals[0] and res2.bounds[1] > evals[-1]
    _, _, res3 = kpm.density_of_states(cfg, num_moments=64, num_vectors=4, seed=3)
    assert np.array_equal(res2.moments, res3.moments) or np.allclose(res2.moments, res3.moments, rtol=0, atol=1e-10)


def test_spectral_function_of_sigma_z(torch):
    cfg, dt, H, evals, U, reps = dense_case("heisenberg_chain_16")
    cfg = dict(cfg)
    cfg["observables"] = [{"terms": [{"expression": "σᶻ₀", "sites": [[0]]}]}]
    M = 512
    bounds = widened(evals)
    E, S, res = kpm.spectral_function(cfg, 0, num_moments=M, bounds=bounds)
    mu = res.moments
    assert mu.shape == (1, M) and res.kernel == "epilogue"
    assert abs(mu[0, 0] - 1.0) <= 1e-10  # <psi|A^+ A|psi> = <psi|psi>
    psi = res.state.cpu().numpy()
    assert abs(psi @ H @ psi - evals[0]) <= 1e-8 * max(1.0, abs(evals[0]))  # the ground state
    sz = np.where((reps >> np.uint64(0)) & np.uint64(1), 1.0, -1.0)  # (the overall sign of A does not enter |<j|A|psi>|^2)
    V0 = (sz * psi).reshape(-1, 1)
    check_moments(mu, H, evals, U, V0, M, bounds, "sigma^z_0 on the ground state of heisenberg_chain_16")
    assert E.shape == S.shape == (2 * M,) and (S >= 0.0).all()
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    theta = np.arccos((E - b) / a)
    integral = np.sum(S * a * np.sin(theta)) * np.pi / len(E)  # Gauss-Chebyshev on the default grid
    assert abs(integral - mu[0, 0]) <= 1e-6
    # the same through an Operator handle and a given state
    _, _, obs = D.loadConfigFromDict(cfg, hamiltonian=True, observables=True)
    _, S2, res2 = kpm.spectral_function(cfg, obs[0], state=res.state, num_moments=64, bounds=bounds, energies=E[::8])
    assert S2.shape == E[::8].shape and np.allclose(res2.moments[0], mu[0, :64], rtol=0, atol=1e-12)


# ---------------------------------------------------------------------------------------------
# failures that must be loud
# ---------------------------------------------------------------------------------------------
def test_narrow_bounds_raise_the_guard(torch):
    cfg, dt, H, evals, U, _ = dense_case("heisenberg_chain_12")
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, torch.float64)
    mid, w = 0.5 * (evals[0] + evals[-1]), evals[-1] - evals[0]
    start = kpm.random_phase_block(len(evals), 2, torch.float64, 1)
    with pytest.raises(D.LsAmdError, match="not inside the bounds") as info:
        kpm.chebyshev_moments(op, start, 512, (mid - 0.25 * w, mid + 0.25 * w))
    step = int(re.search(r"step (\d+)", str(info.value)).group(1))
    assert step < 64 and op.matvecs == 2 * 64  # caught at the first read-back
    with pytest.raises(D.LsAmdError, match="not inside the bounds"):
        kpm.density_of_states(cfg, num_moments=256, bounds=(mid - 0.25 * w, mid + 0.25 * w))


def test_two_partitions_and_bad_arguments_are_refused(torch):
    basis, h2 = D.loadConfigFromDict(model_config("heisenberg_chain_16"), hamiltonian=True)
    reps2, _ = D.enumerateStates(basis, 2)
    pl2 = D.MatvecPlan(h2, reps2, torch.float64)
    x2 = torch.zeros((reps2[0].numel(), 2), dtype=torch.float64, device="cuda")
    y2 = torch.zeros_like(x2)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        pl2.matvec_block_axpby(x2, y2, 1.0, 0.0, 0.0)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert L.ls_amd_matvec_block_axpby(pl2.h, 2, C.c_void_p(x2.data_ptr()), 2, 1, C.c_void_p(y2.data_ptr()), 2, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "one-partition" in L.ls_amd_last_error().decode()
    with pytest.raises(D.LsAmdError, match="one-partition"):
        kpm.chebyshev_moments(LocalOperator(h2, reps2, torch.float64), torch.zeros((sum(r.numel() for r in reps2), 2), dtype=torch.float64,
                                                                                   device="cuda"), 8, (-1.0, 1.0))
    pl, reps, dtype, _, _ = plan_of(torch, "hop_chain_12/f64")
    n = reps[0].numel()
    x = torch.zeros((n, 4), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match=r"K = 65"):
        big = torch.zeros((n, 65), dtype=dtype, device="cuda")
        pl.matvec_block_axpby(big, torch.zeros_like(big), 1.0, 0.0, 0.0)
    with pytest.raises(D.LsAmdError, match="computes in"):
        pl.matvec_block_axpby(x.to(torch.complex128), torch.zeros_like(x).to(torch.complex128), 1.0, 0.0, 0.0)
    with pytest.raises(D.LsAmdError, match="2-D"):
        pl.matvec_block_axpby(x[:, 0], x[:, 1], 1.0, 0.0, 0.0)
    with pytest.raises(D.LsAmdError, match="overlap"):
        pl.matvec_block_axpby(x, x, 1.0, 0.0, 0.0)
    with pytest.raises(D.LsAmdError, match="2K = 8"):
        pl.matvec_block_axpby(x, torch.zeros_like(x), 1.0, 0.0, 0.0, dots=torch.zeros(4, dtype=torch.float64, device="cuda"))
    y = torch.zeros((n, 4), dtype=dtype, device="cuda")
    rc = L.ls_amd_matvec_block_axpby(pl.h, 4, C.c_void_p(x.data_ptr()), 1, 1, C.c_void_p(y.data_ptr()), 4, 1, 1.0, 0.0, 0.0, None, None)
    assert rc == -1 and "share" in L.ls_amd_last_error().decode()
    # the two layouts every block entry refuses (tests/test_kpm_abi.py): row stride 1, column stride 1 at K = 4, of Y as of X above ...
    rc = L.ls_amd_matvec_block_axpby(pl.h, 4, C.c_void_p(x.data_ptr()), 4, 1, C.c_void_p(y.data_ptr()), 1, 1, 1.0, 0.0, 0.0, None, None)
    assert rc == -1 and "(row 1, column 1) of Y" in L.ls_amd_last_error().decode() and "share storage" in L.ls_amd_last_error().decode()
    # ... and the interleaved halves of one buffer, whose address ranges overlap
    big = torch.zeros((n, 8), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        pl.matvec_block_axpby(big[:, :4], big[:, 4:], 1.0, 0.0, 0.0)
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        pl.matvec_block_axpby(big[:, 4:], big[:, :4], 1.0, 0.0, 0.0)


def test_non_hermitian_hamiltonian_is_refused(torch):
    cfg = hop_chain_config(8)
    cfg["hamiltonian"]["terms"] = [{"expression": "σ⁺₀ σ⁻₁", "sites": [[i, (i + 1) % 8] for i in range(8)]}]  # hops one way only
    with pytest.raises(ValueError, match="not Hermitian"):
        kpm.density_of_states(cfg, num_moments=16)
    cfg["observables"] = [{"terms": [{"expression": "σᶻ₀", "sites": [[0]]}]}]
    with pytest.raises(ValueError, match="not Hermitian"):
        kpm.spectral_function(cfg, 0, num_moments=16)
