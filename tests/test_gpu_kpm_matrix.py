"""Matrix-valued Chebyshev moments on the GPU: the bare Gram launch (kpm.block_gram, ls_amd_block_gram; csrc/k_gram.hip) in both of
its forms against an extended-precision Gram; the step with matrix-valued dots (MatvecPlan.matvec_block_axpby_gram) on every path of
the Chebyshev step against the step it wraps; moment matrices, a spectral matrix and cross correlators against eigendecompositions;
and the failures that must be loud."""
import ctypes as C
import functools

import numpy as np
import pytest

import cross_sector_reference as X
import distributed_matvec_amd as D
from distributed_matvec_amd import kpm
from distributed_matvec_amd.diagonalize import LocalOperator
from helpers import model_config
from kpm_matrix_reference import (entry_scale, exact_moment_matrices, gram_bound, gram_longdouble, matrix_tolerance, recurrence_bra_moments,
                                  recurrence_moment_matrices)
from kpm_reference import exact_moments, moment_tolerance
from test_gpu_block_matvec import random_block
from test_gpu_kpm import dense_case, plan_of, widened

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 63, 257, 1025, 100003]  # the row-group tail, fewer rows than one MFMA, one past a tile, many workgroups of partials
SHAPES = [(1, 1), (2, 5), (8, 8), (11, 3), (16, 16), (64, 8), (64, 64)]  # (64, 64) at n <= 1025
LAYOUTS = ["interleaved", "colmajor", "colmajor_ld"]
FORMS = ["auto", "mfma", "valu"]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def guarded_block(torch, Xh, layout, dtype):
    """(n, K) view holding Xh inside a buffer that is NaN before it, after it and in every gap the layout leaves"""
    n, K = Xh.shape
    pad = 37
    if layout == "interleaved":
        size, strides = n * K, (K, 1)
    elif layout == "colmajor":
        size, strides = n * K, (1, n)
    else:
        size, strides = K * (n + 5), (1, n + 5)
    buf = torch.full((pad + size + pad,), float("nan"), dtype=dtype, device="cuda")
    view = torch.as_strided(buf, (n, K), strides, pad)
    view.copy_(torch.from_numpy(np.ascontiguousarray(Xh)).to(dtype).cuda())
    return view


def host_block(n, K, cplx, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(n, K) - 0.5 + (1j * (rs.rand(n, K) - 0.5) if cplx else 0.0)


def takes_mfma(form, K_min, *blocks):
    """the form a launch takes: `mfma` forces k_block_gram_mfma exactly on the interleaved blocks, `valu` never takes it, and
    `auto` takes it there from 8 columns on -- the rule the measurements decided ("Matrix moments")"""
    return form != "valu" and all(is_interleaved(b) for b in blocks) and (form == "mfma" or K_min >= 8)


def is_interleaved(t):
    """what k_block_gram_mfma reads as it lies: a row stride equal to the width, and column stride 1 (or one column)"""
    return t.stride(0) == t.shape[1] and (t.shape[1] == 1 or t.stride(1) == 1)


def assert_gram(got, A, B, what):
    """every entry within 4 (n + 8) 2^-53 ||A_a|| ||B_b|| of the extended-precision Gram (kpm_matrix_reference.gram_bound)"""
    want = gram_longdouble(A, B)
    err = np.abs(got.astype(want.dtype) - want).astype(np.float64)
    bound = gram_bound(A, B)
    assert got.shape == bound.shape, what
    assert np.isfinite(got).all() and (err <= bound).all(), (what, float((err / bound).max()))
    return float((err / bound).max())


# ---------------------------------------------------------------------------------------------
# 1. the bare Gram
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "c128"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bare_gram_against_longdouble(torch, monkeypatch, dt, shape):
    dtype = torch.complex128 if dt == "c128" else torch.float64
    Ka, Kb = shape
    worst = 0.0
    for n in NS:
        if shape == (64, 64) and n > 1025:
            continue
        A, B = random_block(torch, n, Ka, dtype, 3 + n + Ka), random_block(torch, n, Kb, dtype, 5 + n + Kb)
        want, bound = gram_longdouble(A, B), gram_bound(A, B)
        results = {}
        for layout in LAYOUTS:
            a, b = guarded_block(torch, A, layout, dtype), guarded_block(torch, B, layout, dtype)
            for form in FORMS:
                monkeypatch.setenv("LS_AMD_GRAM", form)
                what = (dt, shape, n, layout, form)
                name = D._lib.load().ls_amd_block_gram_kernel_name(int(dt == "c128"), Ka, a.stride(0), a.stride(1), Kb, b.stride(0), b.stride(1)).decode()
                assert name == ("k_block_gram_mfma" if takes_mfma(form, min(Ka, Kb), a, b) else "k_block_gram"), what
                if layout == "interleaved" and form == "mfma":
                    assert name == "k_block_gram_mfma", what
                elif min(Ka, Kb) > 1 and layout != "interleaved":
                    assert name == "k_block_gram", what
                g1 = kpm.block_gram(a, b)
                g2 = kpm.block_gram(a, b)
                assert g1.shape == (Ka, Kb) and g1.dtype == dtype, what
                assert torch.equal(g1, g2) and bytes(g1.cpu().numpy().data) == bytes(g2.cpu().numpy().data), what  # equal bytes
                got = g1.cpu().numpy()
                err = np.abs(got.astype(want.dtype) - want).astype(np.float64)
                assert np.isfinite(got).all(), what  # nothing of the NaN around and between the columns was read
                assert (err <= bound).all(), (what, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
                results[name, layout] = got
        # the two forms agree within the same bound (each is within it of the extended-precision sum; asked of the pair as well)
        for layout in LAYOUTS:
            if ("k_block_gram_mfma", layout) in results:
                assert (np.abs(results["k_block_gram_mfma", layout] - results["k_block_gram", layout]) <= bound).all(), (dt, shape, n, layout)
        # the Gram of a block with itself: Hermitian, the bra register reused on the diagonal chunks
        if Ka == Kb:
            monkeypatch.setenv("LS_AMD_GRAM", "mfma")
            a = guarded_block(torch, A, "interleaved", dtype)
            assert_gram(kpm.block_gram(a, a).cpu().numpy(), A, A, (dt, shape, n, "A^+ A"))
    print(f"bare gram {dt} {shape}: worst error / bound {worst:.3f}")


def test_bare_gram_refusals(torch):
    a = torch.zeros((16, 4), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="both be float64 or both complex128"):
        kpm.block_gram(a, a.to(torch.complex128))
    with pytest.raises(D.LsAmdError, match="same number of rows"):
        kpm.block_gram(a, a[:8])
    with pytest.raises(D.LsAmdError, match="K = 65"):
        kpm.block_gram(torch.zeros((4, 65), dtype=torch.float64, device="cuda"), a[:4])
    with pytest.raises(D.LsAmdError, match="device tensor"):
        kpm.block_gram(a.cpu(), a.cpu())
    with pytest.raises(D.LsAmdError, match="2-D"):
        kpm.block_gram(a[:, 0], a)
    assert torch.equal(kpm.block_gram(a[:0], a[:0]), torch.zeros((4, 4), dtype=torch.float64, device="cuda"))  # no rows: zeros


# ---------------------------------------------------------------------------------------------
# 2. the step with matrix-valued dots
# ---------------------------------------------------------------------------------------------
STEP_CASES = ["hop_chain_12/c128", "momentum_12_5/c128", "fermion_ring_12_dihedral_odd/f64", "heisenberg_chain_16/f64"]


@pytest.mark.parametrize("K", [1, 5, 8])
@pytest.mark.parametrize("name", STEP_CASES)
def test_step_with_gram_wraps_the_chebyshev_step(torch, monkeypatch, name, K):
    pl, reps, dtype, _, _ = plan_of(torch, name)
    n = reps[0].numel()
    Xh, Y0 = random_block(torch, n, K, dtype, 41 + K), random_block(torch, n, K, dtype, 43 + K)
    monkeypatch.setenv("LS_AMD_BLOCK", "auto")
    for layout in ("interleaved", "colmajor"):
        for first in (True, False):
            al, be, ga = (0.31, -0.12, 0.0) if first else (0.62, -0.24, -1.0)
            for form in FORMS:
                monkeypatch.setenv("LS_AMD_GRAM", form)
                what = (name, K, layout, first, form, pl.axpby_kernel(K))
                x = guarded_block(torch, Xh, layout, dtype)
                y_in = np.full_like(Y0, np.nan) if first else Y0  # gamma == 0: Y is poisoned
                y, y_old = guarded_block(torch, y_in, layout, dtype), guarded_block(torch, y_in, layout, dtype)
                dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
                pl.matvec_block_axpby(x, y_old, al, be, ga, dots=dots)
                gram = torch.full((2, K, K), float("nan"), dtype=dtype, device="cuda")
                pl.matvec_block_axpby_gram(x, y, al, be, ga, gram)
                assert pl.gram_kernel(K, x, y) == ("k_block_gram_mfma" if takes_mfma(form, K, x, y) else "k_block_gram"), what
                assert torch.equal(y, y_old), what  # byte-equal to the step it wraps
                assert torch.equal(x.cpu(), torch.from_numpy(np.ascontiguousarray(Xh)).to(dtype)), what  # X is left alone
                Xd, Yd, g = x.cpu().numpy(), y.cpu().numpy(), gram.cpu().numpy()
                assert np.isfinite(Yd).all() and np.isfinite(g).all(), what
                assert_gram(g[0], Xd, Xd, what + ("X^+ X",))
                assert_gram(g[1], Xd, Yd, what + ("X^+ Y",))
                # the diagonals are the dots of the old call
                d = dots.cpu().numpy()
                diag = np.arange(K)
                assert (np.abs(g[0][diag, diag].real - d[:K]) <= np.diagonal(gram_bound(Xd, Xd))).all(), what
                assert (np.abs(g[1][diag, diag].real - d[K:]) <= np.diagonal(gram_bound(Xd, Yd))).all(), what
                # the A^+ [A | Y] launch equals two single launches, byte for byte
                assert torch.equal(gram[0], kpm.block_gram(x, x)) and torch.equal(gram[1], kpm.block_gram(x, y)), what
    assert pl.gram_kernel(K) == "k_block_gram"  # (LS_AMD_GRAM=valu is still set) ...
    monkeypatch.setenv("LS_AMD_GRAM", "mfma")
    assert pl.gram_kernel(K) == "k_block_gram_mfma"  # ... and the interleaved layout is the one assumed


# ---------------------------------------------------------------------------------------------
# 3. moment matrices
# ---------------------------------------------------------------------------------------------
MOMENT_MODELS = ["heisenberg_chain_12", "momentum_12_5", "fermion_ring_12_dihedral_odd"]
KM, MM = 3, 64


@functools.lru_cache(maxsize=None)
def moment_case(name):
    """(dense case, start block, bra block, bounds, exact [M, K, K], its tolerance, exact bra moments [M, 2, K], their tolerance):
    the references computed once and left unchanged"""
    case = dense_case(name)
    _, dt, H, evals, U, _ = case
    V0 = host_block(len(evals), KM, dt == "c128", 17)
    Phi = host_block(len(evals), 2, dt == "c128", 23)
    bounds = widened(evals)
    exact = exact_moment_matrices(evals, U, V0, V0, MM, bounds)
    tol, own = matrix_tolerance(recurrence_moment_matrices(H, V0, MM, bounds), exact, entry_scale(V0, V0))
    exact_b = exact_moment_matrices(evals, U, Phi, V0, MM, bounds)
    tol_b, _ = matrix_tolerance(recurrence_bra_moments(H, Phi, V0, MM, bounds), exact_b, entry_scale(Phi, V0))
    return case, V0, Phi, bounds, exact, tol, own, exact_b, tol_b


_moments = {}


def device_moments(torch, name):
    """(op, device moment matrices [M, K, K]) of moment_case(name), computed once"""
    if name not in _moments:
        (cfg, dt, _, evals, _, want_reps), V0, _, bounds = moment_case(name)[:4]
        dtype = torch.complex128 if dt == "c128" else torch.float64
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
        reps, _ = D.enumerateStates(basis, 1)
        assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), want_reps)
        op = LocalOperator(h, reps, dtype)
        start = torch.from_numpy(np.ascontiguousarray(V0)).to(dtype).cuda()
        mu = kpm.chebyshev_moment_matrices(op, start, MM, bounds)
        assert op.matvecs == KM * (MM // 2)  # K columns per step, two moments per step
        assert np.array_equal(start.cpu().numpy(), V0)  # the start block is left alone
        _moments[name] = (op, dtype, mu)
    return _moments[name]


@pytest.mark.parametrize("name", MOMENT_MODELS)
def test_moment_matrices_match_the_eigendecomposition(torch, monkeypatch, name):
    (_, dt, H, evals, U, _), V0, Phi, bounds, exact, tol, own, exact_b, tol_b = moment_case(name)
    op, dtype, mu = device_moments(torch, name)
    assert mu.shape == (MM, KM, KM) and mu.dtype == np.complex128
    dev = np.abs(mu - exact).max(axis=0)
    print(f"kpm moment matrices {name} ({op.plan.axpby_kernel(KM)}, {op.plan.gram_kernel(KM)}): device deviation {dev.max():.3e}, "
          f"numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}")
    assert (dev <= tol).all(), (name, dev, tol)
    assert np.array_equal(mu, mu.conj().transpose(0, 2, 1))  # every mu_n is Hermitian
    if dt == "f64":
        assert np.abs(mu.imag).max() == 0.0
    # K = 3 takes the vector-ALU Gram under `auto`; the same recurrence on the MFMA form, under the same rule
    start = torch.from_numpy(np.ascontiguousarray(V0)).to(dtype).cuda()
    assert op.plan.gram_kernel(KM) == "k_block_gram"
    monkeypatch.setenv("LS_AMD_GRAM", "mfma")
    assert op.plan.gram_kernel(KM) == "k_block_gram_mfma"
    mu_mfma = kpm.chebyshev_moment_matrices(op, start, MM, bounds)
    monkeypatch.delenv("LS_AMD_GRAM")
    assert (np.abs(mu_mfma - exact).max(axis=0) <= tol).all(), (name, np.abs(mu_mfma - exact).max(axis=0), tol)
    # the diagonal is what chebyshev_moments returns, within that function's own tolerance
    old = kpm.chebyshev_moments(op, start, MM, bounds)
    weights = (np.abs(U.conj().T @ V0) ** 2).T
    tol_old, _ = moment_tolerance(H, V0, MM, bounds, exact_moments(evals, weights, MM, bounds))
    diag = np.arange(KM)
    assert (np.abs(mu[:, diag, diag].real.T - old).max(axis=1) <= tol_old).all(), name
    # another bra block: mu_n = Phi^+ T_n V_0, one order per step
    before = op.matvecs
    mub = kpm.chebyshev_moment_matrices(op, start, MM, bounds, bra=torch.from_numpy(np.ascontiguousarray(Phi)).to(dtype).cuda())
    assert mub.shape == (MM, 2, KM) and op.matvecs - before == KM * (MM - 1)
    dev_b = np.abs(mub - exact_b).max(axis=0)
    assert (dev_b <= tol_b).all(), (name, dev_b, tol_b)


def test_narrow_bounds_raise_the_guard(torch):
    _, _, _, evals, _, _ = dense_case("heisenberg_chain_12")
    op, dtype, _ = device_moments(torch, "heisenberg_chain_12")
    mid, w = 0.5 * (evals[0] + evals[-1]), evals[-1] - evals[0]
    start = kpm.random_phase_block(len(evals), 2, dtype, 1)
    before = op.matvecs
    with pytest.raises(D.LsAmdError, match="not inside the bounds"):
        kpm.chebyshev_moment_matrices(op, start, 512, (mid - 0.25 * w, mid + 0.25 * w))
    assert op.matvecs - before == 2 * kpm.GUARD_EVERY  # caught at the first read-back
    with pytest.raises(D.LsAmdError, match="not inside the bounds"):
        kpm.chebyshev_moment_matrices(op, start, 512, (mid - 0.25 * w, mid + 0.25 * w), bra=start)


# ---------------------------------------------------------------------------------------------
# 5. cross correlators from the device moments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MOMENT_MODELS)
def test_cross_correlation_from_device_moments(torch, name):
    (_, _, _, evals, U, _), V0, _, bounds, _, tol, _, _, _ = moment_case(name)
    _, _, mu = device_moments(torch, name)
    a = 0.5 * (bounds[1] - bounds[0])
    t_max = 4.0 / a * MM / 8
    times = np.linspace(0.0, t_max, 9)
    eps = 1e-12
    Ct = kpm.cross_correlation(mu, bounds, times, eps=eps)
    c = U.conj().T @ V0
    w = entry_scale(V0, V0)
    for t, got in zip(times, Ct):
        want = np.einsum("ja,j,jb->ab", c.conj(), np.exp(-1j * evals * t), c)  # V_0^+ exp(-iHt) V_0
        assert (np.abs(got - want) <= eps * w + 2 * MM * tol).all(), (name, t, np.abs(got - want).max())  # |c_n| <= 2
    with pytest.raises(ValueError, match=r"needs \d+ moments"):
        kpm.cross_correlation(mu, bounds, [8.0 * t_max])


# ---------------------------------------------------------------------------------------------
# 4. spectral matrices
# ---------------------------------------------------------------------------------------------
def test_spectral_matrix_of_two_local_operators(torch):
    """ground state of heisenberg_chain_12 without symmetries, sigma^z_0 and sigma^z_3"""
    cfg, dt, H, evals, U, reps = dense_case("heisenberg_chain_12")
    cfg = dict(cfg)
    cfg["observables"] = [{"terms": [{"expression": "σᶻ₀", "sites": [[0]]}]}, {"terms": [{"expression": "σᶻ₀", "sites": [[3]]}]}]
    M = 64
    bounds = widened(evals)
    E, S, res = kpm.spectral_matrix(cfg, [0, 1], num_moments=M, bounds=bounds)
    assert res.moments.shape == (M, 2, 2) and res.bounds == bounds and res.matvecs == 2 * (M // 2)
    assert res.gram_kernel == "k_block_gram" and res.kernel in ("k_direct_cheb", "epilogue")  # (K = 2: the vector-ALU form under `auto`)
    psi = res.state.cpu().numpy()
    assert abs(psi @ H @ psi - evals[0]) <= 1e-8 * max(1.0, abs(evals[0]))  # the ground state
    sz = [np.where((reps >> np.uint64(j)) & np.uint64(1), 1.0, -1.0) for j in (0, 3)]
    V0 = np.stack([sz[0] * psi, sz[1] * psi], axis=1)
    got_v0 = res.target_states.cpu().numpy()
    sign = np.sign((got_v0[:, 0] * V0[:, 0]).sum())  # (the convention of the bit of sigma^z is one overall sign of both columns)
    assert np.abs(got_v0 - sign * V0).max() <= 1e-14
    exact = exact_moment_matrices(evals, U, V0, V0, M, bounds)
    tol, own = matrix_tolerance(recurrence_moment_matrices(H, V0, M, bounds), exact, entry_scale(V0, V0))
    dev = np.abs(res.moments - exact).max(axis=0)
    print(f"spectral matrix moments: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}")
    assert (dev <= tol).all(), (dev, tol)
    # mu_0[a][b] = <psi|A_a^+ A_b|psi> against the dense product, within the bound of a sum
    assert (np.abs(res.moments[0] - V0.conj().T @ V0) <= gram_bound(V0, V0)).all()
    assert abs(res.moments[0][0, 0] - 1.0) <= 1e-10 and abs(res.moments[0][0, 1]) > 1e-3  # (sigma^z)^2 = 1; the off-diagonal part is there
    # S(w) is the reconstruction of the exact moments within the sum over n of the moment tolerances: every moment enters
    # 1 / (pi a sin theta) (2 - delta_n0) g_n T_n(x) mu_n with |T_n| <= 1
    assert E.shape == (2 * M,) and S.shape == (2 * M, 2, 2)
    a, b = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    pref = 1.0 / (np.pi * a * np.sin(np.arccos((E - b) / a)))
    g = kpm.jackson_kernel(M)
    weight = g.sum() * 2.0 - g[0]
    want = kpm.reconstruct_matrix(exact, bounds, E)
    assert (np.abs(S - want) <= pref[:, None, None] * weight * tol[None]).all()
    lowest = np.array([np.linalg.eigvalsh(0.5 * (s + s.conj().T))[0] for s in S])
    assert (lowest >= -1e-12 * np.trace(res.moments[0]).real).all(), lowest.min()  # the Jackson kernel is positive
    # the same through Operator handles, a given state and given energies
    _, _, obs = D.loadConfigFromDict(cfg, hamiltonian=True, observables=True)
    _, S2, res2 = kpm.spectral_matrix(cfg, [obs[0], obs[1]], state=res.state, num_moments=16, bounds=bounds, energies=E[::8])
    assert S2.shape == (len(E[::8]), 2, 2) and np.abs(res2.moments - res.moments[:16]).max() <= 1e-12
    with pytest.raises(ValueError, match=r"operators\[1\] = 7"):
        kpm.spectral_matrix(cfg, [0, 7], num_moments=16, bounds=bounds)
    with pytest.raises(ValueError, match="1 <= K <= 64"):
        kpm.spectral_matrix(cfg, [], num_moments=16, bounds=bounds)


def _heisenberg(basis_cfg, L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"basis": basis_cfg["basis"], "hamiltonian": {"name": "Heisenberg", "terms": [
        {"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds}, {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}}


def zz2_q(L, dk):
    """sum_j exp(-2 pi i dk j / L) sigma^z_j sigma^z_{j+2}: covariant for k -> k + dk like X.sz_q"""
    def c(z):
        return repr(z.real) if z.imag == 0 else "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"

    return {"terms": [{"expression": c(complex(np.exp(-2j * np.pi * dk * j / L))) + " σᶻ₀ σᶻ₁", "sites": [[j, (j + 2) % L]]} for j in range(L)]}


def test_spectral_matrix_into_another_momentum_sector(torch):
    """the 12-ring with translations, ground state in k = 0, S^z_q and the bond operator of momentum q = 5 into k = 5.  H commutes
    with the global spin flip, under which S^z_q is odd and the bond operator even: their cross moments vanish, and the device has
    to return them as zeros within the floor of the tolerance.  A third operator, S^z_q with its sites shifted by one (e^{iq} S^z_q),
    puts a complex off-diagonal entry next to them."""
    from oracle import model as Mo

    L, M, q = 12, 64, 5
    src, dst = X.ring(L, 6, 0), X.ring(L, 6, q)
    shifted = {"terms": [{"expression": t["expression"], "sites": [[(t["sites"][0][0] + 1) % L]]} for t in X.sz_q(L, q)["terms"]]}
    ops = [X.sz_q(L, q), zz2_q(L, q), shifted]
    cfg = _heisenberg(src, L)
    cfg["observables"] = ops + [X.sz_q(L, 4)]
    reps_t, H = Mo.dense_sector_matrix(_heisenberg(dst, L))
    H = np.asarray(H)
    evals, U = np.linalg.eigh(H)
    bounds = widened(evals)
    E, S, res = kpm.spectral_matrix(cfg, [0, 1, 2], num_moments=M, bounds=bounds, dtype=torch.complex128, target=dst)
    assert res.moments.shape == (M, 3, 3) and res.kernel == "k_pull_gather_cheb" and res.gram_kernel == "k_block_gram"
    psi = res.state.cpu().numpy()
    refs = [X.formula_matrix(src, dst, o) for o in ops]
    assert all(np.array_equal(r["dst"], np.asarray(reps_t, dtype=np.uint64)) for r in refs)
    V0 = np.stack([r["matrix"] @ psi for r in refs], axis=1)
    assert res.target_states.shape == (len(reps_t), 3)
    assert np.abs(res.target_states.cpu().numpy() - V0).max() <= 1e-12 * max(1.0, np.abs(V0).max())
    exact = exact_moment_matrices(evals, U, V0, V0, M, bounds)
    tol, own = matrix_tolerance(recurrence_moment_matrices(H, V0, M, bounds), exact, entry_scale(V0, V0))
    dev = np.abs(res.moments - exact).max(axis=0)
    print(f"spectral matrix k 0 -> {q}: device deviation {dev.max():.3e}, numpy recurrence {own.max():.3e}, tolerance {tol.min():.3e}, "
          f"|mu_0| {np.abs(exact[0]).round(4).tolist()}")
    assert (dev <= tol).all(), (dev, tol)
    assert min(exact[0][0, 0].real, exact[0][1, 1].real) > 1e-2  # nothing passes vacuously
    assert abs(exact[0][0, 1]) <= 1e-12 and abs(exact[0][0, 2].imag) > 1e-2  # the selection rule, and a complex entry beside it
    assert S.shape == (2 * M, 3, 3)
    # an operator of another momentum in the list is refused by name
    with pytest.raises(D.LsAmdError, match=r"operators\[1\] does not map"):
        kpm.spectral_matrix(cfg, [0, 3], num_moments=M, bounds=bounds, dtype=torch.complex128, target=dst)


# ---------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------
def test_two_partitions_and_bad_arguments_are_refused(torch):
    L_ = D._lib.load()
    basis, h2 = D.loadConfigFromDict(model_config("heisenberg_chain_16"), hamiltonian=True)
    reps2, _ = D.enumerateStates(basis, 2)
    pl2 = D.MatvecPlan(h2, reps2, torch.float64)
    x2 = torch.zeros((reps2[0].numel(), 2), dtype=torch.float64, device="cuda")
    y2 = torch.zeros_like(x2)
    g2 = torch.zeros((2, 2, 2), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="one-partition"):
        pl2.matvec_block_axpby_gram(x2, y2, 1.0, 0.0, 0.0, g2)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert L_.ls_amd_matvec_block_axpby_gram(pl2.h, 2, vp(x2), 2, 1, vp(y2), 2, 1, 1.0, 0.0, 0.0, vp(g2), None) == -1
    assert "ls_amd_matvec_block_axpby_gram: one-partition plans only" in L_.ls_amd_last_error().decode()
    with pytest.raises(D.LsAmdError, match="one-partition"):
        kpm.chebyshev_moment_matrices(LocalOperator(h2, reps2, torch.float64),
                                      torch.zeros((sum(r.numel() for r in reps2), 2), dtype=torch.float64, device="cuda"), 8, (-1.0, 1.0))
    pl, reps, dtype, _, _ = plan_of(torch, "hop_chain_12/f64")
    n = reps[0].numel()
    x = torch.zeros((n, 4), dtype=dtype, device="cuda")
    y = torch.zeros_like(x)
    g = torch.zeros((2, 4, 4), dtype=dtype, device="cuda")
    with pytest.raises(D.LsAmdError, match=r"K = 65"):
        big = torch.zeros((n, 65), dtype=dtype, device="cuda")
        pl.matvec_block_axpby_gram(big, torch.zeros_like(big), 1.0, 0.0, 0.0, torch.zeros((2, 65, 65), dtype=dtype, device="cuda"))
    assert L_.ls_amd_matvec_block_axpby_gram(pl.h, 65, vp(x), 65, 1, vp(y), 65, 1, 1.0, 0.0, 0.0, vp(g), None) == -1
    assert "K = 65 is outside [1, 64]" in L_.ls_amd_last_error().decode()
    for bad in (g.to(torch.complex128), g[:1], g.cpu(), g.transpose(1, 2), None):  # dtype, size, device, layout, nothing
        with pytest.raises(D.LsAmdError, match="gram must be a contiguous device tensor of 2 K K = 32 elements"):
            pl.matvec_block_axpby_gram(x, y, 1.0, 0.0, 0.0, bad)
    # a gram tensor inside x: refused by the library, before any launch (x stays what it was)
    xs = torch.ones((n, 4), dtype=dtype, device="cuda")
    assert n * 4 >= 32
    with pytest.raises(D.LsAmdError, match="Gram output overlaps X or Y"):
        pl.matvec_block_axpby_gram(xs, y, 1.0, 0.0, 0.0, xs.view(-1)[:32])
    assert bool((xs == 1.0).all())
    assert L_.ls_amd_matvec_block_axpby_gram(pl.h, 4, vp(x), 4, 1, vp(y), 4, 1, 1.0, 0.0, 0.0, vp(y), None) == -1
    assert "Gram output overlaps X or Y" in L_.ls_amd_last_error().decode()
    assert L_.ls_amd_matvec_block_axpby_gram(pl.h, 4, vp(x), 4, 1, vp(y), 4, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "NULL" in L_.ls_amd_last_error().decode()
    assert L_.ls_amd_matvec_block_axpby_gram(pl.h, 4, None, 4, 1, vp(y), 4, 1, 1.0, 0.0, 0.0, vp(g), None) == -1
    assert "X or Y is NULL" in L_.ls_amd_last_error().decode()
    assert L_.ls_amd_matvec_block_axpby_gram(pl.h, 4, vp(x), 1, 1, vp(y), 4, 1, 1.0, 0.0, 0.0, vp(g), None) == -1
    assert "(row 1, column 1) of X" in L_.ls_amd_last_error().decode() and "share storage" in L_.ls_amd_last_error().decode()
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        pl.matvec_block_axpby_gram(x, x, 1.0, 0.0, 0.0, g)
    with pytest.raises(D.LsAmdError, match="computes in"):
        pl.matvec_block_axpby_gram(x.to(torch.complex128), y.to(torch.complex128), 1.0, 0.0, 0.0, g)
