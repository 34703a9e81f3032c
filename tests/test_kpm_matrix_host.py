"""Matrix-valued Chebyshev moments, the parts that need no device: the C ABI (ls_amd_block_gram, ls_amd_matvec_block_axpby_gram), the
build, the Python names, the arguments the library refuses before it asks for a device, and the host-side functions of kpm.py
(the doubling formulas, reconstruct_matrix, greens_matrix, cross_correlation) against a dense random Hermitian 40 x 40 matrix with
exact moments."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import kpm
from kpm_matrix_reference import (entry_scale, exact_moment_matrices, gram_bound, gram_longdouble, matrix_tolerance, recurrence_blocks,
                                  recurrence_moment_matrices)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-matvec_amd", "csrc")
C_NAMES = ("ls_amd_block_gram", "ls_amd_block_gram_work_bytes", "ls_amd_block_gram_kernel_name", "ls_amd_matvec_block_axpby_gram")
PY_NAMES = ("block_gram", "chebyshev_moment_matrices", "reconstruct_matrix", "greens_matrix", "cross_correlation", "spectral_matrix")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _vp(a):
    return C.cast(a, C.c_void_p)


def test_abi_makefile_and_python_names():
    header = open(os.path.join(ROOT, "include", "ls_amd.h"), encoding="utf-8").read()
    binding = open(os.path.join(ROOT, "distributed-matvec_amd", "_lib.py"), encoding="utf-8").read()
    L = _lib()
    for name in C_NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert '"%s"' % name in binding and hasattr(L, name), name
    assert re.search(r"int\s+ls_amd_matvec_block_axpby_gram\s*\(\s*ls_amd_plan\s*\*\s*\w+\s*,\s*int\s+K\s*,[^;]*double\s+alpha\s*,\s*double\s+beta\s*,"
                     r"\s*double\s+gamma\s*,\s*void\s*\*\s*d_gram\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    make = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "k_gram.hip" in re.search(r"^KSRC := (.*)$", make, re.M).group(1).split()
    # the new unit is not fingerprinted: the fingerprints of the existing kernels stay what they were
    assert "k_gram" not in open(os.path.join(ROOT, "scripts", "kernel_isa_sha.py"), encoding="utf-8").read()
    assert callable(D.MatvecPlan.matvec_block_axpby_gram) and callable(D.MatvecPlan.gram_kernel)
    for name in PY_NAMES:
        assert name in kpm.__all__ and name in D.__all__ and getattr(D, name) is getattr(kpm, name), name


def test_the_gram_unit_has_no_floating_point_atomics_and_uses_the_f64_mfma():
    src = open(os.path.join(CSRC, "k_gram.hip"), encoding="utf-8").read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomicAdd" not in code and "atomic" not in code.lower()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in code and "lsk_corr_sum(" in code
    assert '"k_block_gram_mfma"' in code and '"k_block_gram"' in code


def test_null_pointers_and_bad_widths_are_refused_without_a_device():
    L = _lib()
    x = (C.c_double * 64)()
    y = (C.c_double * 64)()
    g = (C.c_double * 64)()
    w = (C.c_double * 4096)()
    assert L.ls_amd_matvec_block_axpby_gram(None, 2, _vp(x), 2, 1, _vp(y), 2, 1, 1.0, 0.0, 0.0, _vp(g), None) == -1
    assert "ls_amd_matvec_block_axpby_gram: plan is NULL" in L.ls_amd_last_error().decode()
    fake = C.c_void_p(8)  # a non-NULL handle with K out of range: refused before the plan is dereferenced
    for K in (0, 65, -3):
        assert L.ls_amd_matvec_block_axpby_gram(fake, K, _vp(x), 1, 1, _vp(y), 1, 1, 1.0, 0.0, 0.0, _vp(g), None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode() and "[1, 64]" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_gram(0, 4, K, _vp(x), 2, 1, 2, _vp(y), 2, 1, _vp(w), 8 * 4096, _vp(g), None) == -1
        assert f"Ka = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_gram(0, 4, 2, _vp(x), 2, 1, K, _vp(y), 2, 1, _vp(w), 8 * 4096, _vp(g), None) == -1
        assert f"Kb = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_gram_kernel_name(0, K, 1, 1, 2, 2, 1) is None and "[1, 64]" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_gram_work_bytes(4, K, 2, 0) == -1

    def gram(a=x, b=y, work=w, out=g, n=4, a_strides=(2, 1), b_strides=(2, 1), work_bytes=8 * 4096):
        p = lambda t: _vp(t) if t is not None else None  # noqa: E731
        return L.ls_amd_block_gram(0, n, 2, p(a), a_strides[0], a_strides[1], 2, p(b), b_strides[0], b_strides[1], p(work), work_bytes, p(out), None)

    for kw in ({"a": None}, {"b": None}, {"work": None}, {"out": None}):
        assert gram(**kw) == -1 and "NULL" in L.ls_amd_last_error().decode(), kw
    assert gram(n=-1) == -1 and "negative" in L.ls_amd_last_error().decode()
    for bad in ((1, 1), (2, 3), (-2, 1), (1, 2)):  # two elements on one word, or not nested
        assert gram(a_strides=bad) == -1 and "share" in L.ls_amd_last_error().decode() and " A " in L.ls_amd_last_error().decode()
        assert gram(b_strides=bad) == -1 and "share" in L.ls_amd_last_error().decode() and " B " in L.ls_amd_last_error().decode()
    assert gram(work_bytes=8) == -1 and "work_bytes" in L.ls_amd_last_error().decode()
    assert gram(out=x) == -1 and "output overlaps" in L.ls_amd_last_error().decode()
    assert gram(work=y) == -1 and "work buffer overlaps" in L.ls_amd_last_error().decode()
    # sizes: one workgroup of partials per 256 rows, at most 512 over the chunks of 16 real bra columns, two ket blocks of Ka x Kb elements
    assert L.ls_amd_block_gram_work_bytes(1, 2, 3, 0) == 2 * 2 * 3 * 8
    assert L.ls_amd_block_gram_work_bytes(257, 2, 3, 1) == 2 * 2 * 2 * 3 * 16
    assert L.ls_amd_block_gram_work_bytes(10 ** 7, 8, 8, 1) == 512 * 2 * 64 * 16
    assert L.ls_amd_block_gram_work_bytes(10 ** 7, 64, 64, 1) == 64 * 2 * 4096 * 16
    assert L.ls_amd_block_gram_work_bytes(10 ** 7, 64, 8, 0) == 128 * 2 * 512 * 8


def test_kernel_name_follows_the_strides_and_the_knob(monkeypatch):
    """`mfma` names k_block_gram_mfma exactly on the interleaved blocks, `valu` never; `auto` takes it from 8 columns on (the rule
    the measurements of profiles/kpm_matrix_bench.jsonl decided: below that the vector-ALU form is faster)"""
    L = _lib()
    name = lambda *a: L.ls_amd_block_gram_kernel_name(*a).decode()  # noqa: E731
    for mode in ("auto", "mfma", "valu", None):
        if mode is None:
            monkeypatch.delenv("LS_AMD_GRAM", raising=False)
        else:
            monkeypatch.setenv("LS_AMD_GRAM", mode)  # (read at every call)
        wide = "k_block_gram" if mode == "valu" else "k_block_gram_mfma"
        narrow = "k_block_gram_mfma" if mode == "mfma" else "k_block_gram"
        for cplx in (0, 1):
            assert name(cplx, 8, 8, 1, 8, 8, 1) == wide
            assert name(cplx, 64, 64, 1, 11, 11, 1) == wide
            assert name(cplx, 64, 64, 1, 3, 3, 1) == narrow
            assert name(cplx, 7, 7, 1, 7, 7, 1) == narrow
            assert name(cplx, 1, 1, 1, 1, 1, 1000) == narrow  # one column: its stride does not matter
            assert name(cplx, 8, 1, 1000, 8, 8, 1) == "k_block_gram"  # a column-major bra
            assert name(cplx, 8, 8, 1, 8, 1, 1000) == "k_block_gram"  # a column-major ket
            assert name(cplx, 8, 9, 1, 8, 8, 1) == "k_block_gram"  # rows with a gap


# ---- the host side of kpm.py on a dense matrix -------------------------------------------------------------------------------------
N, K, M = 40, 3, 96


def _dense(gap=False):
    rs = np.random.RandomState(5)
    A = rs.randn(N, N) + 1j * rs.randn(N, N)
    H = 0.5 * (A + A.conj().T)
    evals, U = np.linalg.eigh(H)
    if gap:  # the same eigenvectors, the levels moved out of (-0.5, 0.5)
        evals = np.concatenate([np.linspace(-1.0, -0.5, N // 2), np.linspace(0.5, 1.0, N - N // 2)])
        H = (U * evals) @ U.conj().T
    V0 = rs.randn(N, K) + 1j * rs.randn(N, K)
    w = evals[-1] - evals[0]
    return H, evals, U, V0, (float(evals[0] - 0.01 * w), float(evals[-1] + 0.01 * w))


def test_doubling_helper_against_exact_moments():
    H, evals, U, V0, bounds = _dense()
    exact = exact_moment_matrices(evals, U, V0, V0, M, bounds)
    tol, own = matrix_tolerance(recurrence_moment_matrices(H, V0, M, bounds), exact, entry_scale(V0, V0))
    V = recurrence_blocks(H, V0, M // 2 + 1, bounds)
    grams = np.stack([np.stack([V[n].conj().T @ V[n], V[n].conj().T @ V[n + 1]]) for n in range(M // 2)])
    mu = kpm.moment_matrices_from_grams(grams, M)
    assert mu.shape == (M, K, K) and mu.dtype == np.complex128
    assert (np.abs(mu - exact).max(axis=0) <= tol).all(), (np.abs(mu - exact).max(axis=0), tol, own)
    assert np.array_equal(mu, mu.conj().transpose(0, 2, 1))  # symmetrised
    odd = kpm.moment_matrices_from_grams(grams, M - 1)
    assert odd.shape == (M - 1, K, K) and np.array_equal(odd, mu[:M - 1])
    # the extended-precision Gram of the reference agrees with numpy's within the bound of a sum
    assert (np.abs(gram_longdouble(V0, V[1]).astype(np.complex128) - V0.conj().T @ V[1]) <= gram_bound(V0, V[1])).all()


def test_reconstruct_matrix_is_reconstruct_entry_by_entry_and_positive():
    _, evals, U, V0, bounds = _dense()
    mu = exact_moment_matrices(evals, U, V0, V0, M, bounds)
    E = np.concatenate([kpm.chebyshev_grid(bounds, 50), [bounds[0] - 1.0, bounds[1] + 1.0]])
    S = kpm.reconstruct_matrix(mu, bounds, E)
    assert S.shape == (52, K, K) and S.dtype == np.complex128
    for a in range(K):
        for b in range(K):
            want = kpm.reconstruct(mu[:, a, b].real, bounds, E) + 1j * kpm.reconstruct(mu[:, a, b].imag, bounds, E)
            assert np.abs(S[:, a, b] - want).max() <= 1e-13 * np.abs(S).max(), (a, b)
    assert (S[-2:] == 0.0).all()  # outside the bounds
    assert np.abs(S - S.conj().transpose(0, 2, 1)).max() <= 1e-13 * np.abs(S).max()
    lowest = np.array([np.linalg.eigvalsh(0.5 * (s + s.conj().T))[0] for s in S])
    assert (lowest >= -1e-12 * np.trace(mu[0]).real).all(), lowest.min()  # the Jackson kernel is positive
    # Gauss-Chebyshev on the grid: the integral of S is mu_0
    a_, b_ = 0.5 * (bounds[1] - bounds[0]), 0.5 * (bounds[1] + bounds[0])
    Eg = kpm.chebyshev_grid(bounds, 2 * M)
    Sg = kpm.reconstruct_matrix(mu, bounds, Eg)
    integral = (Sg * (a_ * np.sin(np.arccos((Eg - b_) / a_)))[:, None, None]).sum(axis=0) * np.pi / len(Eg)
    assert np.abs(integral - mu[0]).max() <= 1e-10 * np.abs(mu[0]).max()


def test_greens_matrix_has_the_reconstruction_as_its_spectral_part():
    _, evals, U, V0, bounds = _dense()
    mu = exact_moment_matrices(evals, U, V0, V0, M, bounds)
    E = kpm.chebyshev_grid(bounds, 64)
    G = kpm.greens_matrix(mu, bounds, E)
    S = kpm.reconstruct_matrix(mu, bounds, E)
    assert G.shape == S.shape and G.dtype == np.complex128
    spectral = -(G - G.conj().transpose(0, 2, 1)) / (2j * np.pi)
    assert np.abs(spectral - S).max() <= 1e-13 * np.abs(S).max()
    diag = np.arange(K)
    assert np.abs(-G[:, diag, diag].imag / np.pi - S[:, diag, diag].real).max() <= 1e-13 * np.abs(S).max()
    assert (kpm.greens_matrix(mu, bounds, [bounds[1] + 1.0]) == 0.0).all()


def test_greens_matrix_inside_a_gap_is_the_resolvent():
    """far from every level (0.5 against a kernel width of pi a / M ~ 0.006) the damped series is the resolvent itself up to
    O((width / distance)^2): sign, prefactor and the order of the indices of G_ab = <v_a|(E - H)^-1|v_b>"""
    _, evals, U, V0, bounds = _dense(gap=True)
    big = 512
    mu = exact_moment_matrices(evals, U, V0, V0, big, bounds)
    G = kpm.greens_matrix(mu, bounds, [0.0, 0.1])
    c = U.conj().T @ V0
    for g, E in zip(G, (0.0, 0.1)):
        want = np.einsum("ja,j,jb->ab", c.conj(), 1.0 / (E - evals), c)
        assert np.abs(g - want).max() <= 1e-2 * np.abs(want).max(), (E, np.abs(g - want).max(), np.abs(want).max())


def test_cross_correlation_against_the_dense_propagator():
    H, evals, U, V0, bounds = _dense()
    a_ = 0.5 * (bounds[1] - bounds[0])
    big = 256
    mu = exact_moment_matrices(evals, U, V0, V0, big, bounds)
    times = np.array([0.0, 0.3, 1.7, -2.0, 4.0 / a_ * big / 8])
    Ct = kpm.cross_correlation(mu, bounds, times, eps=1e-12)
    assert Ct.shape == (len(times), K, K) and Ct.dtype == np.complex128
    assert np.abs(Ct[0] - mu[0]).max() <= 1e-14 * np.abs(mu[0]).max()  # C(0) = mu_0
    c = U.conj().T @ V0
    w = entry_scale(V0, V0)
    for t, got in zip(times, Ct):
        want = np.einsum("ja,j,jb->ab", c.conj(), np.exp(-1j * evals * t), c)
        # eps w for the truncated tail; every kept order adds |c_n| <= 2 times the rounding of an exact moment (a few u w)
        assert (np.abs(got - want) <= 1e-12 * w + 2 * big * 1e-15 * w).all(), (t, np.abs(got - want).max())
    # a bra block of its own: [M, Ka, Kb] moments
    Phi = np.random.RandomState(8).randn(N, 2) + 0j
    mub = exact_moment_matrices(evals, U, Phi, V0, big, bounds)
    got = kpm.cross_correlation(mub, bounds, [1.1])[0]
    want = np.einsum("ja,j,jb->ab", (U.conj().T @ Phi).conj(), np.exp(-1j * evals * 1.1), c)
    assert got.shape == (2, K) and (np.abs(got - want) <= (1e-12 + 2 * big * 1e-15) * entry_scale(Phi, V0)).all()
    with pytest.raises(ValueError, match=r"needs \d+ moments"):
        kpm.cross_correlation(mu[:8], bounds, [50.0 / a_])
    with pytest.raises(ValueError, match="moments"):
        kpm.cross_correlation(mu[:, 0, 0], bounds, [0.1])
