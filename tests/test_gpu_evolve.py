"""Chebyshev time evolution on the GPU: the accumulate step (MatvecPlan.matvec_block_axpby_acc, ls_amd_matvec_block_axpby_acc) on every
path -- k_direct_evolve, resolve + k_pull_gather_evolve, the column loop with the k_axpby_acc epilogue -- against the references of
test_gpu_kpm (none of which uses this library's matvec); the bare epilogue against numpy; propagate(), evolve() and
autocorrelation() against eigendecompositions; and the failures that must be loud."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import config, evolve, kpm
from distributed_matvec_amd.diagonalize import LocalOperator
from evolve_reference import exact_propagate, propagate_tolerance
from helpers import model_config
from kpm_reference import exact_moments, moment_tolerance
from test_gpu_block_matvec import device_block, random_block
from test_gpu_kpm import CHEB, LAYOUTS, MODES, assert_close, assert_dots, cases, coefficient_sets, dense_case, plan_of, widened

pytestmark = pytest.mark.gpu

KS = [1, 2, 4, 5, 8, 9, 64]  # both sides of the column chunk (4 for c128, 8 for f64), a partial last chunk, the cap
CS = [0.7, -0.3 + 1.1j]
EVOLVE = {"epilogue": "epilogue", "k_direct_cheb": "k_direct_evolve", "k_pull_gather_cheb": "k_pull_gather_evolve"}
# LS_AMD_ACC=split: the Chebyshev kernel of the path, then one pass of k_axpby_acc over the finished Y
SPLIT = {"epilogue": "epilogue", "k_direct_cheb": "k_direct_cheb+k_axpby_acc", "k_pull_gather_cheb": "k_pull_gather_cheb+k_axpby_acc"}
FORMS = {"fused": EVOLVE, "split": SPLIT}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def assert_acc(got, Z0, c, want, what):
    """Z0 + c want: the accumulate adds one rounding to the step's own"""
    bound = 1e-12 * max(1.0, np.abs(Z0).max() + abs(c) * np.abs(want).max())
    err = np.abs(got - (Z0 + c * want)).max()
    assert err <= bound, (what, err, bound)


# ---------------------------------------------------------------------------------------------
# the step on every path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(cases()))
def test_step_accumulates_on_every_path(torch, monkeypatch, name, K):
    _, _, _, auto_path, opts = cases()[name]
    pl, reps, dtype, apply, _ = plan_of(torch, name)
    if "resolve_bytes" in opts:
        monkeypatch.setenv("LS_AMD_BLOCK_RESOLVE_BYTES", str(opts["resolve_bytes"]))
    n = reps[0].numel()
    X = random_block(torch, n, K, dtype, 11 + K)
    Y0 = random_block(torch, n, K, dtype, 31 + K)
    HX = apply(X)
    ztypes = [torch.complex128] if dtype == torch.complex128 else [torch.float64, torch.complex128]
    Z0s = {zt: random_block(torch, n, K, zt, 51 + K) for zt in ztypes}
    own_layout = 0
    for mode, form in [(m, f) for m in MODES for f in FORMS]:
        monkeypatch.setenv("LS_AMD_BLOCK", mode)
        monkeypatch.delenv("LS_AMD_ACC", raising=False)
        assert pl.acc_kernel(K) in (EVOLVE[pl.axpby_kernel(K)], SPLIT[pl.axpby_kernel(K)])  # (the default: one of the two forms)
        monkeypatch.setenv("LS_AMD_ACC", form)
        path = pl.acc_kernel(K)
        assert path == FORMS[form][pl.axpby_kernel(K)] and pl.axpby_kernel(K) == CHEB[pl.block_kernel(K)]
        if mode == "columns" or (mode == "auto" and K == 1):
            assert path == "epilogue", (name, mode, K)
            if form == "split":
                continue  # (the column loop has one form)
        elif auto_path is not None and (mode == "auto" or auto_path != "epilogue"):
            assert path == FORMS[form][auto_path], (name, mode, K, path)
        for li, layout in enumerate(LAYOUTS):
            for al, be, ga in coefficient_sets(HX)[1:]:  # gamma == 0 (Y holds NaN), and the Chebyshev triple
                want = al * HX + be * X + (ga * Y0 if ga != 0.0 else 0.0)
                for ci, c in enumerate(CS):
                    for zt in ztypes:
                        if zt == torch.float64 and complex(c).imag != 0.0:
                            continue  # (refused: test_bad_accumulators_are_refused)
                        zlayout = layout if ci == 0 else LAYOUTS[(li + 1) % len(LAYOUTS)]  # Z has strides of its own
                        own_layout += zlayout != layout
                        x = device_block(torch, X, layout, dtype)
                        x0 = x.clone()
                        y = device_block(torch, Y0, layout, dtype) if ga != 0.0 else device_block(torch, X, layout, dtype, fill=float("nan"))
                        z = device_block(torch, Z0s[zt], zlayout, zt)
                        dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
                        pl.matvec_block_axpby_acc(x, y, al, be, ga, z, c, dots=dots)
                        got = y.cpu().numpy()
                        what = (name, K, mode, path, layout, zlayout, str(zt), (al, be, ga), c)
                        assert np.isfinite(got).all(), what  # gamma == 0: Y was not read
                        assert torch.equal(x, x0), what  # X is left alone
                        assert_close(got, want, what)
                        assert_dots(dots.cpu().numpy(), X, got, what)
                        assert_acc(z.cpu().numpy(), Z0s[zt], c, want, what)
    assert own_layout > 0
    # a vector is a block of one column
    if K == 1:
        monkeypatch.setenv("LS_AMD_BLOCK", "auto")
        monkeypatch.delenv("LS_AMD_ACC", raising=False)
        x = torch.from_numpy(np.ascontiguousarray(X[:, 0])).cuda()
        y = torch.full_like(x, float("nan"))
        z = torch.from_numpy(np.ascontiguousarray(Z0s[torch.complex128][:, 0])).cuda()
        pl.matvec_block_axpby_acc(x, y, 0.37, -1.2, 0.0, z, CS[1])
        want = 0.37 * HX + -1.2 * X
        assert_close(y.cpu().numpy(), want[:, 0], (name, "vector"))
        assert_acc(z.cpu().numpy(), Z0s[torch.complex128][:, 0], CS[1], want[:, 0], (name, "vector"))


# ---------------------------------------------------------------------------------------------
# the bare epilogue
# ---------------------------------------------------------------------------------------------
def offset_block(torch, A, layout, dtype):
    """device_block, 8 bytes off the 16-byte grid (f64 only: torch keeps complex128 tensors on it)"""
    n, K = A.shape
    src = torch.from_numpy(np.ascontiguousarray(A)).to(dtype).cuda()
    if layout == "interleaved":
        t = torch.empty(n * K + 1, dtype=dtype, device="cuda")[1:].view(n, K)
    else:
        t = torch.empty(n * K + 1, dtype=dtype, device="cuda")[1:].view(K, n).t()
    assert t.data_ptr() % 16 == 8
    t.copy_(src)
    return t


@pytest.mark.parametrize("types", ["f64/f64", "f64/c128", "c128/c128"])
@pytest.mark.parametrize("K", [1, 2, 5, 8, 11, 64])
def test_bare_epilogue_against_numpy(torch, types, K):
    dtype, zt = ((torch.complex128 if s == "c128" else torch.float64) for s in types.split("/"))
    c = 0.7 if zt == torch.float64 else -0.3 + 1.1j
    for n in (1, 2, 255, 4099, 4100):  # (odd and even: the 16-byte column-major form needs even column strides, and has a tail row)
        W, X, Y0 = (random_block(torch, n, K, dtype, s + K + n) for s in (1, 2, 3))
        Z0 = random_block(torch, n, K, zt, 4 + K + n)
        combos = [(a, a, a, a, False) for a in LAYOUTS] + [("interleaved", "colmajor", "colmajor_ld", "interleaved", False),
                                                           ("colmajor", "colmajor", "colmajor", "interleaved", False),
                                                           ("interleaved", "interleaved", "interleaved", "colmajor_ld", False)]
        if dtype == torch.float64:  # the 16-byte forms must fall back: every block, then Z alone, 8 bytes off
            combos += [("interleaved",) * 4 + (True,), ("colmajor",) * 4 + (True,), ("interleaved",) * 4 + ("z",), ("colmajor",) * 4 + ("z",)]
        for lw, lx, ly, lz, off in combos:
            for al, be, ga in ((0.37, -1.2, 0.0), (1.7, -0.6, -1.0)):
                mk = offset_block if off is True else device_block
                w, x = mk(torch, W, lw, dtype), mk(torch, X, lx, dtype)
                w0, x0 = w.clone(), x.clone()
                y = mk(torch, Y0, ly, dtype)
                if ga == 0.0:
                    y.fill_(float("nan"))
                if off and zt == torch.float64:
                    z = offset_block(torch, Z0, lz, zt)
                else:
                    z = device_block(torch, Z0, lz, zt)
                dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
                D.block_axpby_acc(w, x, y, al, be, ga, z, c, dots=dots)
                got = y.cpu().numpy()
                what = (types, K, n, lw, lx, ly, lz, off, ga)
                want = al * W + be * X + (ga * Y0 if ga != 0.0 else 0.0)
                assert np.isfinite(got).all(), what
                assert torch.equal(w, w0) and torch.equal(x, x0), what
                assert_close(got, want, what)
                assert_dots(dots.cpu().numpy(), X, got, what)
                assert_acc(z.cpu().numpy(), Z0, c, want, what)


def test_bare_epilogue_with_a_c128_accumulator_off_the_16_byte_grid(torch):
    """torch cannot make such a tensor; the C ABI can be handed one"""
    from distributed_matvec_amd import _lib

    L = _lib.load()
    for n, K in ((255, 1), (255, 5), (256, 4)):
        W, X = (random_block(torch, n, K, torch.float64, s + K + n) for s in (1, 2))
        Z0 = random_block(torch, n, K, torch.complex128, 3 + K + n)
        for layout in ("interleaved", "colmajor"):
            w, x = device_block(torch, W, layout, torch.float64), device_block(torch, X, layout, torch.float64)
            y = torch.full_like(w, float("nan"))
            buf = torch.zeros(2 * n * K + 1, dtype=torch.float64, device="cuda")
            zview = torch.view_as_real(torch.from_numpy(np.ascontiguousarray(Z0)).cuda()).reshape(-1)
            buf[1:].copy_(zview)
            zp = buf.data_ptr() + 8
            assert zp % 16 == 8
            rc = L.ls_amd_block_axpby_acc(0, 1, n, K, C.c_void_p(w.data_ptr()), w.stride(0), w.stride(1), C.c_void_p(x.data_ptr()), x.stride(0),
                                          x.stride(1), C.c_void_p(y.data_ptr()), y.stride(0), y.stride(1), C.c_void_p(zp), K, 1, 0.37, -1.2, 0.0,
                                          -0.3, 1.1, None, None)
            assert rc == 0, L.ls_amd_last_error().decode()
            torch.cuda.synchronize()
            want = 0.37 * W - 1.2 * X
            assert_close(y.cpu().numpy(), want, (n, K, layout))
            got = buf[1:].cpu().numpy().view(np.complex128).reshape(n, K)
            assert_acc(got, Z0, -0.3 + 1.1j, want, (n, K, layout))
            assert buf[0].item() == 0.0


# ---------------------------------------------------------------------------------------------
# propagate
# ---------------------------------------------------------------------------------------------
# (k_direct_evolve with a real state, f64 recurrence under a c128 sum: the t-V ring -- the one-way hops of hop_chain_12, the other
# f64 case of that kernel, are not Hermitian and are refused below)
DIRECT_F64 = "spinless_ring_9_4/f64"
PROPAGATE = [DIRECT_F64, "heisenberg_kagome_12_symm/c128", "momentum_12_5/c128", "fermion_ring_12_dihedral_odd/f64",
             "heisenberg_chain_16/f64"]
TIMES = [(0.3, False), (7.0, False), (-7.0, False), (2.0, True)]


@functools.lru_cache(maxsize=None)
def dense_of(torch, name):
    """(dense sector matrix, eigenvalues, eigenvectors) of a case of test_gpu_kpm: from the case's own reference -- the 12870
    states of heisenberg_chain_16 from dense_case, whose eigendecomposition the tests of kpm share"""
    pl, reps, dtype, apply, _ = plan_of(torch, name)
    n = reps[0].numel()
    if name == "heisenberg_chain_16/f64":
        _, _, H, evals, U, want_reps = dense_case("heisenberg_chain_16")
        assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), want_reps)
        return H, evals, U
    H = np.asarray(apply(np.eye(n, dtype=np.complex128 if dtype == torch.complex128 else np.float64)))
    assert np.abs(H - H.conj().T).max() <= 1e-13
    evals, U = np.linalg.eigh(H)
    return H, evals, U


_operators = {}


def operator_of(torch, name, dtype=None):
    pl, reps, own, _, h = plan_of(torch, name)
    dtype = dtype or own
    if (name, dtype) not in _operators:
        _operators[(name, dtype)] = LocalOperator(h, reps, dtype)
    return _operators[(name, dtype)]


@functools.lru_cache(maxsize=None)
def propagated(torch, name, t, imaginary):
    """(psi [n, 3], bounds, exact e^{-iHt} psi, tolerance per column): computed once, shared by K = 1 (the first column) and K = 3"""
    _, reps, dtype, _, _ = plan_of(torch, name)
    H, evals, U = dense_of(torch, name)
    bounds = widened(evals)
    psi = random_block(torch, len(evals), 3, dtype, 17)
    exact = exact_propagate(H, psi, t, imaginary, bounds[0], eig=(evals, U))
    if t < 0.0 and dtype == torch.float64:
        # real H, real psi: the series and the exact result at -t are the complex conjugates of those at t, rounding included
        tol, own = propagated(torch, name, -t, imaginary)[3:]
    else:
        tol, own = propagate_tolerance(H, psi, t, bounds, 1e-12, imaginary, eig=(evals, U))
    for a in (psi, exact):
        a.setflags(write=False)
    return psi, bounds, exact, tol, own


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("t,imaginary", TIMES)
@pytest.mark.parametrize("name", PROPAGATE)
def test_propagate_matches_the_eigendecomposition(torch, name, t, imaginary, K):
    psi, bounds, exact, tol, own = propagated(torch, name, t, imaginary)
    op = operator_of(torch, name)
    n = psi.shape[0]
    auto_path = cases()[name][3]
    assert op.plan.acc_kernel(K) in (("epilogue",) if K == 1 else (EVOLVE[auto_path], SPLIT[auto_path]))
    state = torch.from_numpy(np.ascontiguousarray(psi[:, :K])).to(op.dtype).cuda()
    if K == 1:
        state = state[:, 0].contiguous()
    before = op.matvecs
    got_t = evolve.propagate(op, state, t, bounds=bounds, eps=1e-12, imaginary=imaginary)
    order = len(evolve.propagator_coefficients(t, bounds, 1e-12, imaginary)[0]) - 1
    assert op.matvecs - before == K * order
    assert got_t.shape == state.shape
    assert got_t.dtype == (op.dtype if imaginary else torch.complex128)
    got = got_t.cpu().numpy().reshape(n, K)
    dev = np.abs(got - exact[:, :K]).max(axis=0)
    print(f"propagate {name} t = {t} imaginary = {imaginary} K = {K} ({op.plan.acc_kernel(K)}): order {order}, device deviation "
          f"{dev.max():.3e}, numpy series {own[:K].max():.3e}, tolerance {tol[:K].min():.3e}")
    assert (dev <= tol[:K]).all(), (name, t, imaginary, K, dev, tol[:K])
    assert np.array_equal(state.cpu().numpy().reshape(n, K), psi[:, :K])  # the start is left alone
    if imaginary:
        return
    # unitary: the norm is conserved to the same tolerance
    norms = np.linalg.norm(got, axis=0)
    defect = np.abs(norms - np.linalg.norm(psi[:, :K], axis=0))
    print(f"norm defect {defect.max():.3e}")
    assert (defect <= tol[:K]).all(), (defect, tol[:K])
    # ... and back: each way within its own tolerance
    back_tol = propagated(torch, name, -t, False)[3]
    opc = operator_of(torch, name, torch.complex128)
    back = evolve.propagate(opc, got_t, -t, bounds=bounds, eps=1e-12).cpu().numpy().reshape(n, K)
    assert (np.abs(back - psi[:, :K]).max(axis=0) <= tol[:K] + back_tol[:K]).all()


# ---------------------------------------------------------------------------------------------
# evolve, autocorrelation
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def neel_chain():
    """the 12-site chain at half filling with the staggered magnetisation as two observables (even and odd sites), dense"""
    from oracle import model as M

    L = 12
    cfg = config.heisenberg_chain_config(L)
    cfg["observables"] = [{"name": "even", "terms": [{"expression": "σᶻ₀", "sites": [[i] for i in range(0, L, 2)]}]},
                          {"name": "odd", "terms": [{"expression": "σᶻ₀", "sites": [[i] for i in range(1, L, 2)]}]}]
    reps, H = M.dense_sector_matrix(cfg)
    H = np.ascontiguousarray(np.asarray(H).real)
    dense_obs = []
    for o in cfg["observables"]:
        reps_o, O = M.dense_sector_matrix({"basis": cfg["basis"], "hamiltonian": o})
        assert np.array_equal(reps_o, reps)
        dense_obs.append(np.asarray(O))
    neel = int(sum(1 << i for i in range(0, L, 2)))
    psi = np.zeros(len(reps))
    psi[int(np.searchsorted(np.asarray(reps, dtype=np.uint64), np.uint64(neel)))] = 1.0
    return cfg, H, np.linalg.eigvalsh(H), dense_obs, psi


def test_evolve_staggered_magnetisation_of_the_neel_state(torch):
    cfg, H, evals, dense_obs, psi = neel_chain()
    bounds = widened(evals)
    times = [0.0, 0.25, 0.5, 1.0, 3.0]
    state = torch.from_numpy(psi).cuda()
    res = evolve.evolve(cfg, state, times, observables=[0, 1], keep_states=True, bounds=bounds)
    assert isinstance(res, D.EvolveResult)
    assert res.values.shape == (5, 2, 1) and res.values.dtype == np.complex128 and res.norms.shape == (5, 1) and res.orders.shape == (5,)
    assert np.array_equal(res.times, np.array(times)) and res.bounds == bounds
    # segments 0, 0.25, 0.25, 0.5, 2.0: the order grows with the segment
    assert res.orders[0] == 0 and res.orders[1] == res.orders[2] and (np.diff(res.orders[1:]) >= 0).all() and res.orders[4] > res.orders[1]
    assert res.matvec_columns == int(res.orders.sum()) and res.kernel in ("epilogue", "k_direct_evolve", SPLIT["k_direct_cheb"])
    L = 12
    stag = lambda v: ((v.conj() @ (dense_obs[0] @ v)) - (v.conj() @ (dense_obs[1] @ v))) / L  # noqa: E731
    assert abs(abs(stag(psi)) - 1.0) <= 1e-14
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    op = LocalOperator(h, D.enumerateStates(basis, 1)[0], torch.complex128)
    for j, t in enumerate(times):
        exact = exact_propagate(H, psi, t)
        tol, _ = propagate_tolerance(H, psi, t, bounds) if t != 0.0 else (np.array([1e-13]), None)
        # segment after segment: every earlier segment's deviation is carried along and the last adds its own
        tol_j = (j + 1) * tol[0]
        got_state = res.states[j].cpu().numpy()
        assert np.abs(got_state - exact).max() <= tol_j, (t, np.abs(got_state - exact).max(), tol_j)
        got = (res.values[j, 0, 0] - res.values[j, 1, 0]) / L
        # <v|O|v> with |O| <= 1 for the staggered magnetisation per site and |v| = 1: twice the deviation of v
        print(f"evolve t = {t}: state {np.abs(got_state - exact).max():.3e}, m_s {abs(got - stag(exact)):.3e}, tolerance {tol_j:.3e}")
        assert abs(got - stag(exact)) <= 2.0 * tol_j, (t, got, stag(exact))
        assert abs(got.imag) <= 2.0 * tol_j
        assert abs(res.norms[j, 0] - 1.0) <= tol_j
        # keep_states: what propagate returns for the same segment from the previous state
        # (two correct runs of one segment, f64 or c128 recurrence: each within the segment's own tolerance)
        if j > 0 and times[j] != times[j - 1]:
            dt = times[j] - times[j - 1]
            again = evolve.propagate(op, res.states[j - 1].to(torch.complex128), dt, bounds=bounds)
            seg_tol, _ = propagate_tolerance(H, exact_propagate(H, psi, times[j - 1]), dt, bounds)
            assert np.abs(again.cpu().numpy() - got_state).max() <= 2.0 * seg_tol[0]
    assert abs(stag(exact_propagate(H, psi, 3.0))) < 0.5  # the order melts: the comparison above is not of constants
    assert res.states[0].dtype == torch.float64 and res.states[1].dtype == torch.complex128  # f64 recurrence first, c128 after


def test_autocorrelation_two_routes_one_number(torch):
    name = DIRECT_F64
    H, evals, U = dense_of(torch, name)
    bounds = widened(evals)
    op = operator_of(torch, name)
    v0 = random_block(torch, len(evals), 1, torch.float64, 23)
    start = torch.from_numpy(v0).cuda()
    times = np.array([0.3, 7.0])
    M = len(evolve.propagator_coefficients(times[-1], bounds)[0])
    M += M % 2
    mu = kpm.chebyshev_moments(op, start, M, bounds)
    got = evolve.autocorrelation(mu[0], bounds, times)
    weights = (np.abs(U.conj().T @ v0) ** 2).T
    exact_mu = exact_moments(evals, weights, M, bounds)
    mtol, _ = moment_tolerance(H, v0, M, bounds, exact_mu)
    for j, t in enumerate(times):
        psi_t = evolve.propagate(op, start[:, 0].contiguous(), float(t), bounds=bounds).cpu().numpy()
        route = np.vdot(v0[:, 0], psi_t)
        c, _ = evolve.propagator_coefficients(float(t), bounds)
        ptol, _ = propagate_tolerance(H, v0, float(t), bounds)
        bound = ptol[0] + np.abs(c).sum() * mtol[0]  # each route within its own tolerance
        print(f"autocorrelation t = {t}: moments {got[j]:.15g}, propagate {route:.15g}, difference {abs(got[j] - route):.3e}, bound {bound:.3e}")
        assert abs(got[j] - route) <= bound


# ---------------------------------------------------------------------------------------------
# failures that must be loud
# ---------------------------------------------------------------------------------------------
def test_bounds_inside_the_spectrum_raise_the_guard(torch):
    name = DIRECT_F64
    _, evals, _ = dense_of(torch, name)
    op = operator_of(torch, name)
    mid, w = 0.5 * (evals[0] + evals[-1]), evals[-1] - evals[0]
    narrow = (float(mid - 0.25 * w), float(mid + 0.25 * w))
    start = kpm.random_phase_block(len(evals), 2, torch.float64, 1)
    with pytest.raises(D.LsAmdError, match="not inside the bounds") as info:
        evolve.propagate(op, start, 200.0, bounds=narrow)
    assert repr(narrow[0]) in str(info.value) and repr(narrow[1]) in str(info.value)


def test_two_partitions_are_refused(torch):
    basis, h2 = D.loadConfigFromDict(model_config("heisenberg_chain_16"), hamiltonian=True)
    reps2, _ = D.enumerateStates(basis, 2)
    pl2 = D.MatvecPlan(h2, reps2, torch.float64)
    x2 = torch.zeros((reps2[0].numel(), 2), dtype=torch.float64, device="cuda")
    y2, z2 = torch.zeros_like(x2), torch.zeros_like(x2)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        pl2.matvec_block_axpby_acc(x2, y2, 1.0, 0.0, 0.0, z2, 1.0)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    assert L.ls_amd_matvec_block_axpby_acc(pl2.h, 2, C.c_void_p(x2.data_ptr()), 2, 1, C.c_void_p(y2.data_ptr()), 2, 1, 1.0, 0.0, 0.0,
                                           C.c_void_p(z2.data_ptr()), 2, 1, 0, 1.0, 0.0, None, None) == -1
    assert "one-partition" in L.ls_amd_last_error().decode()
    op2 = LocalOperator(h2, reps2, torch.float64)
    with pytest.raises(D.LsAmdError, match="one-partition"):
        evolve.propagate(op2, torch.zeros(sum(r.numel() for r in reps2), dtype=torch.float64, device="cuda"), 1.0, bounds=(-1.0, 1.0))


def test_bad_accumulators_are_refused(torch):
    pl, reps, dtype, _, _ = plan_of(torch, "hop_chain_12/f64")
    n = reps[0].numel()
    x = torch.zeros((n, 4), dtype=dtype, device="cuda")
    y, z = torch.zeros_like(x), torch.zeros_like(x)
    with pytest.raises(D.LsAmdError, match="Z and Y overlap"):
        pl.matvec_block_axpby_acc(x, y, 1.0, 0.0, 0.0, y, 1.0)
    with pytest.raises(D.LsAmdError, match="Z and X overlap"):
        pl.matvec_block_axpby_acc(x, y, 1.0, 0.0, 0.0, x, 1.0)
    both = torch.zeros((n, 8), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match="overlap"):  # interleaved halves of one buffer
        pl.matvec_block_axpby_acc(x, both[:, :4], 1.0, 0.0, 0.0, both[:, 4:], 1.0)
    with pytest.raises(D.LsAmdError, match="not real"):
        pl.matvec_block_axpby_acc(x, y, 1.0, 0.0, 0.0, z, 1.0 + 0.5j)
    with pytest.raises(D.LsAmdError, match="one shape"):
        pl.matvec_block_axpby_acc(x, y, 1.0, 0.0, 0.0, torch.zeros((n, 3), dtype=dtype, device="cuda"), 1.0)
    with pytest.raises(D.LsAmdError, match="computes in"):
        pl.matvec_block_axpby_acc(x.to(torch.complex128), y.to(torch.complex128), 1.0, 0.0, 0.0, z.to(torch.complex128), 1.0)
    with pytest.raises(D.LsAmdError, match=r"K = 65"):
        big = torch.zeros((n, 65), dtype=dtype, device="cuda")
        pl.matvec_block_axpby_acc(big, torch.zeros_like(big), 1.0, 0.0, 0.0, torch.zeros_like(big), 1.0)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    rc = L.ls_amd_matvec_block_axpby_acc(pl.h, 4, C.c_void_p(x.data_ptr()), 4, 1, C.c_void_p(y.data_ptr()), 4, 1, 1.0, 0.0, 0.0,
                                         C.c_void_p(z.data_ptr()), 1, 1, 0, 1.0, 0.0, None, None)
    assert rc == -1 and "share" in L.ls_amd_last_error().decode() and "of Z " in L.ls_amd_last_error().decode()
    rc = L.ls_amd_matvec_block_axpby_acc(pl.h, 4, C.c_void_p(x.data_ptr()), 4, 1, C.c_void_p(y.data_ptr()), 4, 1, 1.0, 0.0, 0.0, None, 4, 1, 0,
                                         1.0, 0.0, None, None)
    assert rc == -1 and "Z is NULL" in L.ls_amd_last_error().decode()
    plc, repsc, _, _, _ = plan_of(torch, "hop_chain_12/c128")
    xc = torch.zeros((n, 2), dtype=torch.complex128, device="cuda")
    with pytest.raises(D.LsAmdError, match="must be complex128"):
        plc.matvec_block_axpby_acc(xc, torch.zeros_like(xc), 1.0, 0.0, 0.0, torch.zeros((n, 2), dtype=torch.float64, device="cuda"), 1.0)
    rc = L.ls_amd_matvec_block_axpby_acc(plc.h, 2, C.c_void_p(xc.data_ptr()), 2, 1, C.c_void_p(torch.zeros_like(xc).data_ptr()), 2, 1, 1.0, 0.0,
                                         0.0, C.c_void_p(z.data_ptr()), 2, 1, 0, 1.0, 0.0, None, None)
    assert rc == -1 and "z_cplx" in L.ls_amd_last_error().decode()
    # a c128 Z off the 16-byte grid (torch cannot make one): refused where a fused row kernel would run, taken by k_axpby_acc
    buf = torch.zeros(2 * n * 4 + 1, dtype=torch.float64, device="cuda")
    xr = torch.ones((n, 4), dtype=dtype, device="cuda")
    call = lambda: L.ls_amd_matvec_block_axpby_acc(pl.h, 4, C.c_void_p(xr.data_ptr()), 4, 1, C.c_void_p(y.data_ptr()), 4, 1, 0.0, 1.0, 0.0,  # noqa: E731
                                                   C.c_void_p(buf.data_ptr() + 8), 4, 1, 1, 0.5, -2.0, None, None)
    os.environ["LS_AMD_BLOCK"] = "kernel"
    try:
        os.environ["LS_AMD_ACC"] = "fused"
        assert pl.acc_kernel(4) == "k_direct_evolve" and call() == -1 and "16-byte aligned" in L.ls_amd_last_error().decode()
        os.environ["LS_AMD_ACC"] = "split"
        assert call() == 0, L.ls_amd_last_error().decode()
        os.environ["LS_AMD_BLOCK"] = "columns"
        assert call() == 0, L.ls_amd_last_error().decode()
    finally:
        os.environ.pop("LS_AMD_ACC", None)
        os.environ.pop("LS_AMD_BLOCK", None)
    torch.cuda.synchronize()
    got = buf[1:].cpu().numpy().view(np.complex128)  # Y = X = 1 twice: Z = 2 (0.5 - 2i)
    assert buf[0].item() == 0.0 and np.abs(got - (1.0 - 4.0j)).max() <= 1e-14
    # the same refusals from the driver: a complex state on a float64 operator
    with pytest.raises(D.LsAmdError, match="complex128"):
        op = operator_of(torch, DIRECT_F64)
        evolve.propagate(op, torch.zeros(op.n_local, dtype=torch.complex128, device="cuda"), 1.0, bounds=(-1.0, 1.0))
    # ... and a Hamiltonian that is not Hermitian (hops one way only)
    with pytest.raises(ValueError, match="not Hermitian"):
        evolve.propagate(operator_of(torch, "hop_chain_12/f64"), torch.zeros(n, dtype=torch.float64, device="cuda"), 1.0, bounds=(-1.0, 1.0))
