"""Projected spinless-fermion bases on the GPU against the independent reference (tests/fermion_symm.py): representatives and
norms bit for bit, ls_hs_state_info / ls_hs_is_representative on batches, y = B+ H B x on every one-partition pull path (fused,
resolve + gather, block matvec, slot cache), free-fermion ground energies per momentum in closed form through diagonalize(), the
union of the sector spectra of an interacting model, and the refusal of every other path at plan creation."""
import ctypes as C

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib
from distributed_matvec_amd.diagonalize import diagonalize
from fermion_jw import ring, square, yaml_terms
from fermion_symm import closure, dihedral, projected_matrix, representatives, state_info, torus, translations, tv_model, free_ring_energy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def cfg_of(L, N, gens, secs, model):
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N,
                      "symmetries": [{"permutation": list(p), "sector": int(s)} for p, s in zip(gens, secs)]},
            "hamiltonian": {"terms": yaml_terms(model, False)}}


def enumerate_(torch, cfg):
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    return basis, h, reps


# (L, N, generators, sectors): translations, dihedral groups (complex and +-1 characters), the 4 x 4 torus with D4 (network elements)
CASES = [
    (8, 4, translations(8), [0]), (8, 4, translations(8), [3]), (8, 2, translations(8), [4]), (10, 5, translations(10), [0]),
    (10, 4, translations(10), [5]), (12, 6, translations(12), [1]), (13, 5, translations(13), [6]), (14, 7, translations(14), [7]),
    (8, 4, dihedral(8), [0, 0]), (8, 4, dihedral(8), [4, 1]), (10, 5, dihedral(10), [0, 1]), (12, 6, dihedral(12), [6, 0]),
    (14, 6, dihedral(14), [0, 0]), (16, 3, torus(4, 4), [0, 0, 0, 0]), (16, 4, torus(4, 4), [2, 2, 0, 1]),
    (16, 2, torus(4, 4, point_group=False), [1, 0]), (16, 5, torus(4, 4, point_group=False), [1, 3]),
]


@pytest.mark.parametrize("L,N,gens,secs", CASES)
def test_enumeration_norms_and_state_info_match_the_reference(torch, L, N, gens, secs):
    group = closure(L, gens, secs)
    want_reps, want_norms = representatives(L, N, group)
    basis, h, reps = enumerate_(torch, cfg_of(L, N, gens, secs, tv_model(ring(L))))
    assert basis.hasFermionSigns()
    got = reps[0].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want_reps), (len(got), len(want_reps))
    # a batch of every weight-N state: representatives, characters, norms and the representative flags
    lib = _lib.load()
    from fermion_jw import weight_states

    alphas = weight_states(L, N)
    n = len(alphas)
    betas, chars, norms = np.zeros(n, np.uint64), np.zeros(2 * n), np.zeros(n)
    flags, norms2 = np.zeros(n, np.uint8), np.zeros(n)
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lib.ls_hs_state_info(basis.payload, n, alphas.ctypes.data_as(u64p), 1, betas.ctypes.data_as(u64p), 1, chars.ctypes.data_as(f64p),
                         norms.ctypes.data_as(f64p))
    lib.ls_hs_is_representative(basis.payload, n, alphas.ctypes.data_as(u64p), 1, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                norms2.ctypes.data_as(f64p))
    for i, a in enumerate(alphas):
        r, ch, nr = state_info(group, int(a))
        assert int(betas[i]) == r and abs(norms[i] - nr) <= 1e-14 and norms2[i] == norms[i], (hex(int(a)), int(betas[i]), r, norms[i], nr)
        if nr > 0:  # (on a vanishing orbit the minimising elements disagree in chi sign: no character is defined)
            assert abs(complex(chars[2 * i], chars[2 * i + 1]) - ch) <= 1e-12, (hex(int(a)), chars[2 * i: 2 * i + 2], ch)
        assert bool(flags[i]) == (r == int(a))
    rows = np.searchsorted(alphas, want_reps)
    assert np.array_equal(norms[rows], want_norms)  # the plan's norms are the same kernel's


# (every operator commutes with its group: a bond phase breaks the reflections, so it only appears with translations)
MATVEC_CASES = {
    "ring_10_k0_tV": (10, 4, translations(10), [0], tv_model(ring(10), V=0.7)),
    "ring_10_k3_phase": (10, 5, translations(10), [3], tv_model(ring(10), V=0.4, phase=0.3)),
    "ring_12_dihedral_odd": (12, 5, dihedral(12), [6, 1], tv_model(ring(12), V=1.1)),
    "ring_12_dihedral_nnn": (12, 6, dihedral(12), [0, 0], tv_model(ring(12), V=0.5) + tv_model([(i, (i + 2) % 12) for i in range(12)], t=0.3)),
    "torus_4x4_d4": (16, 4, torus(4, 4), [2, 2, 0, 1], tv_model(square(4, 4), V=0.8)),
    "torus_4x4_k": (16, 3, torus(4, 4, point_group=False), [1, 2], tv_model(square(4, 4), V=0.6, phase=0.2)),
    # 64-bit words: rotations and reflections past bit 32, and network elements (the x translations of a 4 x 9 torus)
    "ring_34_dihedral": (34, 3, dihedral(34), [0, 1], tv_model(ring(34), V=0.6)),
    "torus_4x9_k": (36, 3, torus(4, 9), [1, 3], tv_model(square(4, 9), V=0.5, phase=0.1)),
}


def close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


@pytest.mark.parametrize("name", sorted(MATVEC_CASES))
def test_matvec_paths_match_the_projected_reference(torch, monkeypatch, name):
    L, N, gens, secs, model = MATVEC_CASES[name]
    group = closure(L, gens, secs)
    reps_ref, _ = representatives(L, N, group)
    Hs = projected_matrix(model, L, N, group, reps_ref)
    cfg = cfg_of(L, N, gens, secs, model)
    basis, h, reps = enumerate_(torch, cfg)
    assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), reps_ref)
    n = len(reps_ref)
    real = np.abs(Hs.imag).max() <= 1e-14 and all(abs(np.imag(ch)) < 1e-14 for _, ch in group)
    rs = np.random.RandomState(3)
    dtypes = [torch.complex128] + ([torch.float64] if real else [])
    for dt in dtypes:
        x = rs.rand(n) - 0.5 + (1j * (rs.rand(n) - 0.5) if dt == torch.complex128 else 0)
        want = Hs @ x
        for path in ("fused", "split", "cached"):
            if path == "split":
                monkeypatch.setenv("LS_AMD_PULL_SPLIT", str(1 << 20))
            pl = D.MatvecPlan(h, reps, dt)
            monkeypatch.delenv("LS_AMD_PULL_SPLIT", raising=False)
            if path == "cached":
                assert pl.cache_slots(1 << 30) > 0
            assert pl.kernel == ("tile-pull+indexed+cached" if path == "cached" else "tile-pull+indexed"), (path, pl.kernel)
            xd = torch.from_numpy(np.ascontiguousarray(x)).to(dt).cuda()
            yd = torch.zeros_like(xd)
            pl.matvec([xd], [yd])
            got = yd.cpu().numpy()
            close(got, want if dt == torch.complex128 else want.real, (name, path, dt))
            K = 5
            X = rs.rand(n, K) - 0.5 + (1j * (rs.rand(n, K) - 0.5) if dt == torch.complex128 else 0)
            for layout in ("interleaved", "colmajor"):
                src = torch.from_numpy(np.ascontiguousarray(X)).to(dt)
                if layout == "interleaved":
                    Xd = src.cuda()
                    Yd = torch.zeros((n, K), dtype=dt, device="cuda")
                else:
                    Xd = src.t().contiguous().cuda().t()
                    Yd = torch.zeros((K, n), dtype=dt, device="cuda").t()
                monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
                assert pl.block_kernel(K) == "k_pull_gather_blk"
                pl.matvec_block(Xd, Yd)
                monkeypatch.delenv("LS_AMD_BLOCK")
                Wt = Hs @ X
                close(Yd.cpu().numpy(), Wt if dt == torch.complex128 else Wt.real, (name, path, layout, dt))


def test_free_fermions_per_momentum_closed_form(torch):
    # 32-bit words (f64 and c128 sectors, single-vector and block Lanczos), then 64-bit words.  (Above 60 modes the static index
    # table of the pull kernel does not fit, and such plans are refused: test_other_paths_are_refused_at_creation.)
    for L, N, runs in ((28, 14, ((0, 1), (14, 2), (5, 1), (5, 2))), (40, 5, ((0, 1), (3, 1))), (44, 3, ((0, 1), (17, 2)))):
        for s, bs in runs:
            cfg = cfg_of(L, N, translations(L), [s], tv_model(ring(L)))
            dt = torch.complex128 if (2 * s) % L != 0 else torch.float64
            r = diagonalize(cfg, num_evals=1, eps=1e-9, dtype=dt, block_size=bs)
            want = free_ring_energy(L, N, s)
            assert abs(r.eigenvalues[0] - want) <= 1e-8, (L, N, s, bs, r.eigenvalues[0], want)


def dense_columns(torch, pl, n, dt):
    M = np.zeros((n, n), dtype=complex)
    for j in range(n):
        e = torch.zeros(n, dtype=dt, device="cuda")
        e[j] = 1
        y = torch.zeros_like(e)
        pl.matvec([e], [y])
        M[:, j] = y.cpu().numpy()
    return M


@pytest.mark.parametrize("L,N,gens,bonds", [(10, 4, translations(10), ring(10)), (16, 3, torus(4, 4, point_group=False), square(4, 4))])
def test_union_of_sector_spectra_is_the_unprojected_spectrum(torch, L, N, gens, bonds):
    model = tv_model(bonds, V=1.3)
    full = {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N},
            "hamiltonian": {"terms": yaml_terms(model, False)}}
    _, hf, rf = enumerate_(torch, full)
    nf = int(rf[0].numel())
    want = np.linalg.eigvalsh(dense_columns(torch, D.MatvecPlan(hf, rf, torch.complex128), nf, torch.complex128))
    import itertools

    orders = [len(closure(L, [p], [0])) for p in gens]
    got = []
    for secs in itertools.product(*[range(o) for o in orders]):
        _, h, reps = enumerate_(torch, cfg_of(L, N, gens, list(secs), model))
        n = int(reps[0].numel())
        if n:
            M = dense_columns(torch, D.MatvecPlan(h, reps, torch.complex128), n, torch.complex128)
            assert np.abs(M - M.conj().T).max() < 1e-12
            got.extend(np.linalg.eigvalsh(M))
    assert len(got) == nf
    assert np.abs(np.sort(got) - want).max() < 1e-10


def test_ground_state_over_sectors_equals_the_unprojected_one(torch):
    L, N = 24, 6
    model = tv_model(ring(L), V=0.9)
    full = {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": N},
            "hamiltonian": {"terms": yaml_terms(model, False)}}
    e0 = diagonalize(full, num_evals=1, eps=1e-10)
    best = min(diagonalize(cfg_of(L, N, translations(L), [s], model), num_evals=1, eps=1e-10,
                           dtype=torch.float64 if (2 * s) % L == 0 else torch.complex128).eigenvalues[0] for s in range(L))
    assert abs(best - e0.eigenvalues[0]) <= 1e-9, (best, e0.eigenvalues[0])


def test_other_paths_are_refused_at_creation(torch, monkeypatch):
    L, N = 10, 4
    cfg = cfg_of(L, N, translations(L), [0], tv_model(ring(L), V=0.5))
    basis, h, reps = enumerate_(torch, cfg)

    def refused(what, reps_=reps, **kw):
        with pytest.raises(D.LsAmdError, match=what):
            D.MatvecPlan(h, reps_, torch.float64, **kw)

    refused("more than one partition", reps_=D.enumerateStates(basis, 3)[0])
    refused("one partition per process", reps_=reps[0], my_partition=0, num_partitions=2)
    refused("push mode", mode="push")
    for var, val, what in (("LS_AMD_MODE", "push", "push mode"), ("LS_AMD_PULL_VALUES", "1", "LS_AMD_PULL_VALUES=1"),
                           ("LS_AMD_PULL_INDEXED", "0", "LS_AMD_PULL_INDEXED=0")):
        monkeypatch.setenv(var, val)
        refused(what)
        monkeypatch.delenv(var)
    # a non-Hermitian operator: one directed hop
    nh = cfg_of(L, N, translations(L), [0], [(-1.0, [("+", i, 0), ("-", (i + 1) % L, 0)]) for i in range(L)])
    _, hn, rn = enumerate_(torch, nh)
    with pytest.raises(D.LsAmdError, match="non-Hermitian"):
        D.MatvecPlan(hn, rn, torch.float64)
    assert D.MatvecPlan(h, reps, torch.float64).kernel == "tile-pull+indexed"  # and the default still builds
    # 64 modes: no static index table (tag bits), and the hash-table pull has no signs
    _, h64, r64 = enumerate_(torch, cfg_of(64, 2, translations(64), [0], tv_model(ring(64))))
    with pytest.raises(D.LsAmdError, match="no static index table"):
        D.MatvecPlan(h64, r64, torch.float64)
