"""Projected spinful-fermion bases on the GPU against the independent reference (tests/fermion_spinful_symm.py): representatives and
norms bit for bit, ls_hs_state_info / ls_hs_is_representative on batches, y = B+ H B x on every one-partition pull path (fused,
resolve + gather, block matvec, slot cache) for Hubbard rings and tori with cross-species terms, 64-bit words, the spinless basis
on the 2 L modes as a second device path, sectors that partition the (N↑, N↓) space, free-fermion energies per momentum through
diagonalize(), the ground state over all sectors, and the refusal of every other path at plan creation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib
from distributed_matvec_amd.diagonalize import diagonalize
from fermion_jw import hubbard_model, product_states, ring, square, yaml_terms
from fermion_spinful_symm import (as_spinless, exchange_model, free_spinful_ring_energy, group, lift, pair_hopping_model, projected_matrix,
                                  representatives, state_info_v)
from fermion_symm import closure, dihedral, free_ring_energy, torus, translations

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def cfg_of(L, nu, nd, gens, secs, flip, model):
    basis = {"particle": "spinful-fermion", "number_sites": L, "number_particles": nu + nd, "number_up": nu,
             "symmetries": [{"permutation": list(p), "sector": int(s)} for p, s in zip(gens, secs)]}
    if flip:
        basis["spin_flip"] = flip
    return {"basis": basis, "hamiltonian": {"terms": yaml_terms(model, True)}}


def enumerate_(torch, cfg):
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    return basis, h, reps


# (L, N↑, N↓, site generators, sectors, flip): complex characters, +-1 characters, network elements (tori), an empty and a full species
CASES = [
    (6, 3, 3, translations(6), [1], 0), (7, 3, 2, translations(7), [2], 0), (8, 4, 4, dihedral(8), [0, 0], 1),
    (8, 4, 4, dihedral(8), [4, 1], -1), (10, 5, 5, translations(10), [0], -1), (9, 2, 2, torus(3, 3, point_group=False), [1, 2], 0),
    (16, 2, 2, torus(4, 4), [0, 0, 0, 0], 1), (8, 0, 3, dihedral(8), [0, 1], 0), (6, 6, 2, translations(6), [3], 0),
    (6, 3, 3, [], [], -1), (4, 2, 2, translations(4), [0], 1),
]
SIZES = {0: 66, 1: 105, 2: 181, 3: 145, 4: 3202, 5: 144, 6: 91}  # the representative counts of the first seven cases


@pytest.mark.parametrize("case", range(len(CASES)))
def test_enumeration_norms_and_state_info_match_the_reference(torch, case):
    L, nu, nd, gens, secs, flip = CASES[case]
    grp = group(L, gens, secs, flip)
    want_reps, want_norms = representatives(L, nu, nd, grp)
    if case in SIZES:
        assert len(want_reps) == SIZES[case]
    basis, h, reps = enumerate_(torch, cfg_of(L, nu, nd, gens, secs, flip, hubbard_model(L, ring(L))))
    assert basis.hasFermionSigns() and basis.spinFlip() == flip and basis.groupOrder() == len(grp)
    got = reps[0].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want_reps), (len(got), len(want_reps))
    # a batch of every product state: representatives, characters, norms and the representative flags
    lib = _lib.load()
    alphas = product_states(L, nu, nd)
    n = len(alphas)
    betas, chars, norms = np.zeros(n, np.uint64), np.zeros(2 * n), np.zeros(n)
    flags, norms2 = np.zeros(n, np.uint8), np.zeros(n)
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lib.ls_hs_state_info(basis.payload, n, alphas.ctypes.data_as(u64p), 1, betas.ctypes.data_as(u64p), 1, chars.ctypes.data_as(f64p),
                         norms.ctypes.data_as(f64p))
    lib.ls_hs_is_representative(basis.payload, n, alphas.ctypes.data_as(u64p), 1, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                norms2.ctypes.data_as(f64p))
    rep, ch0, nr = state_info_v(grp, alphas)
    assert np.array_equal(betas, rep)
    assert np.abs(norms - nr).max() <= 1e-14 and np.array_equal(norms, norms2)
    live = nr > 0  # (on a vanishing orbit the minimising elements disagree in chi sign: no character is defined)
    assert np.abs((chars[0::2] + 1j * chars[1::2] - ch0)[live]).max(initial=0.0) <= 1e-12
    assert np.array_equal(flags.astype(bool), rep == alphas)
    assert np.array_equal(norms[np.searchsorted(alphas, want_reps)], want_norms)  # the plan's norms are the same kernel's


def hubbard_plus(L, bonds, extra, **kw):
    return hubbard_model(L, bonds, **kw) + extra


# (every operator commutes with its group: a bond phase breaks the reflections, so it appears with translations and the flip only;
# the exchange and pair-hopping terms are summed over all bonds and cross the species, so their Jordan-Wigner strings do)
MATVEC_CASES = {
    "ring_8_dihedral_flip_p": (8, 4, 4, dihedral(8), [0, 0], 1, hubbard_model(8, ring(8), U=4.0)),
    "ring_8_dihedral_flip_m_exchange": (8, 4, 4, dihedral(8), [4, 1], -1, hubbard_plus(8, ring(8), exchange_model(ring(8)), U=3.0)),
    "ring_7_k2_phase": (7, 3, 2, translations(7), [2], 0, hubbard_model(7, ring(7), U=2.5, phase=0.3)),
    "ring_8_k3_phase_flip": (8, 3, 3, translations(8), [3], -1, hubbard_model(8, ring(8), U=2.0, phase=0.2)),
    "ring_6_k1_pair_hopping": (6, 3, 3, translations(6), [1], 1, hubbard_plus(6, ring(6), pair_hopping_model(ring(6)), U=1.5, V=0.3)),
    "ring_10_k0_flip_exchange": (10, 5, 5, translations(10), [0], -1, hubbard_plus(10, ring(10), exchange_model(ring(10)), U=4.0)),
    "ring_9_dihedral_odd_filling": (9, 4, 2, dihedral(9), [0, 1], 0, hubbard_plus(9, ring(9), pair_hopping_model(ring(9)), U=3.0)),
    "torus_3x3_k_exchange": (9, 2, 2, torus(3, 3, point_group=False), [1, 2], 0,
                             hubbard_plus(9, square(3, 3), exchange_model(square(3, 3)), U=2.0)),
    "torus_4x4_d4_flip": (16, 2, 2, torus(4, 4), [0, 0, 0, 0], 1, hubbard_plus(16, square(4, 4), exchange_model(square(4, 4)), U=4.0)),
    # 64-bit words: the swap and the per-half reversal past bit 32, and network elements (a torus of more than 16 sites)
    "ring_17_dihedral_flip": (17, 2, 2, dihedral(17), [0, 1], -1, hubbard_plus(17, ring(17), exchange_model(ring(17)), U=4.0)),
    "ring_22_dihedral_flip": (22, 2, 2, dihedral(22), [11, 0], 1, hubbard_plus(22, ring(22), pair_hopping_model(ring(22)), U=2.0)),
    "ring_20_k3_phase": (20, 2, 1, translations(20), [3], 0, hubbard_model(20, ring(20), U=3.0, phase=0.25)),
    "torus_4x5_k_flip": (20, 2, 2, torus(4, 5), [1, 2], 1, hubbard_plus(20, square(4, 5), exchange_model(square(4, 5)), U=3.0)),
}


def close(got, want, what):
    err = np.abs(got - want).max()
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (what, err)


@pytest.mark.parametrize("name", sorted(MATVEC_CASES))
def test_matvec_paths_match_the_projected_reference(torch, monkeypatch, name):
    L, nu, nd, gens, secs, flip, model = MATVEC_CASES[name]
    grp = group(L, gens, secs, flip)
    reps_ref, _ = representatives(L, nu, nd, grp)
    assert len(reps_ref) > 0
    Hs = projected_matrix(model, L, nu, nd, grp, reps_ref, dense=False)
    assert abs(Hs - Hs.conj().T).max() < 1e-12  # the operator commutes with the group
    basis, h, reps = enumerate_(torch, cfg_of(L, nu, nd, gens, secs, flip, model))
    assert np.array_equal(reps[0].cpu().numpy().view(np.uint64), reps_ref)
    n = len(reps_ref)
    real = abs(Hs.imag).max() <= 1e-14 and all(abs(np.imag(ch)) < 1e-14 for _, ch in grp)
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
            close(yd.cpu().numpy(), want if dt == torch.complex128 else want.real, (name, path, dt))
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


@pytest.mark.parametrize("L,nu,nd,gens,secs", [(10, 5, 5, dihedral(10), [0, 0]), (10, 5, 5, translations(10), [3]), (12, 6, 5, dihedral(12), [6, 1]),
                                               (12, 6, 5, translations(12), [5])])
def test_the_spinless_basis_on_the_modes_is_a_second_device_path(torch, L, nu, nd, gens, secs):
    """without a flip, the projected SPINLESS basis on the 2 L modes with the lifted generators (network + table K4 throughout)
    holds the new basis as the rows whose low half has N↑ particles: same representatives, same norms, and the same matvec on
    vectors supported there"""
    model = hubbard_model(L, ring(L), U=4.0) if len(gens) == 2 else hubbard_model(L, ring(L), U=4.0, phase=0.2)
    basis, h, reps = enumerate_(torch, cfg_of(L, nu, nd, gens, secs, 0, model))
    wide = {"basis": {"particle": "spinless-fermion", "number_sites": 2 * L, "number_particles": nu + nd,
                      "symmetries": [{"permutation": lift(p, L), "sector": int(s)} for p, s in zip(gens, secs)]},
            "hamiltonian": {"terms": yaml_terms(as_spinless(model, L), False)}}
    wbasis, wh, wreps = enumerate_(torch, wide)
    r_new, r_wide = reps[0].cpu().numpy().view(np.uint64), wreps[0].cpu().numpy().view(np.uint64)
    rows = np.nonzero(np.bitwise_count(r_wide & np.uint64((1 << L) - 1)) == nu)[0]
    assert len(r_new) > 0 and np.array_equal(r_wide[rows], r_new)
    dt = torch.float64 if len(gens) == 2 else torch.complex128
    pl, wpl = D.MatvecPlan(h, reps, dt), D.MatvecPlan(wh, wreps, dt)
    assert pl.kernel == wpl.kernel == "tile-pull+indexed"
    lib = _lib.load()
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    norms = []
    for b, r in ((basis, r_new), (wbasis, np.ascontiguousarray(r_wide[rows]))):
        nn, bb, cc = np.zeros(len(r)), np.zeros(len(r), np.uint64), np.zeros(2 * len(r))
        lib.ls_hs_state_info(b.payload, len(r), r.ctypes.data_as(u64p), 1, bb.ctypes.data_as(u64p), 1, cc.ctypes.data_as(f64p), nn.ctypes.data_as(f64p))
        norms.append(nn)
    assert np.array_equal(norms[0], norms[1]) and norms[0].min() > 0
    rs = np.random.RandomState(11)
    x = rs.rand(len(r_new)) - 0.5 + (1j * (rs.rand(len(r_new)) - 0.5) if dt == torch.complex128 else 0)
    xw = np.zeros(len(r_wide), dtype=x.dtype)
    xw[rows] = x
    xd, xwd = torch.from_numpy(x).to(dt).cuda(), torch.from_numpy(xw).to(dt).cuda()
    yd, ywd = torch.zeros_like(xd), torch.zeros_like(xwd)
    pl.matvec([xd], [yd])
    wpl.matvec([xwd], [ywd])
    yw = ywd.cpu().numpy()
    close(yd.cpu().numpy(), yw[rows], (L, nu, nd, secs))
    mask = np.ones(len(r_wide), bool)
    mask[rows] = False
    assert np.abs(yw[mask]).max(initial=0.0) <= 1e-12  # the Hubbard model conserves N↑


def dense_columns(torch, pl, n, dt):
    M = np.zeros((n, n), dtype=complex)
    for j in range(n):
        e = torch.zeros(n, dtype=dt, device="cuda")
        e[j] = 1
        y = torch.zeros_like(e)
        pl.matvec([e], [y])
        M[:, j] = y.cpu().numpy()
    return M


@pytest.mark.parametrize("L,nu,nd,gens,flip,bonds", [(6, 3, 3, translations(6), True, ring(6)), (8, 4, 4, translations(8), True, ring(8)),
                                                     (9, 2, 2, torus(3, 3, point_group=False), False, square(3, 3)),
                                                     (6, 2, 3, torus(3, 2), False, square(3, 2))])
def test_sectors_partition_the_product_space(torch, L, nu, nd, gens, flip, bonds):
    model = hubbard_plus(L, bonds, exchange_model(bonds, J=0.3), U=4.0)
    full = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": nu + nd, "number_up": nu},
            "hamiltonian": {"terms": yaml_terms(model, True)}}
    _, hf, rf = enumerate_(torch, full)
    nf = int(rf[0].numel())
    assert nf == len(product_states(L, nu, nd))
    want = np.linalg.eigvalsh(dense_columns(torch, D.MatvecPlan(hf, rf, torch.complex128), nf, torch.complex128))
    orders = [len(closure(L, [p], [0])) for p in gens]
    got, total = [], 0
    for secs in itertools.product(*[range(o) for o in orders]):
        for f in ((1, -1) if flip else (0,)):
            _, h, reps = enumerate_(torch, cfg_of(L, nu, nd, gens, list(secs), f, model))
            n = int(reps[0].numel())
            total += n  # (an empty sector contributes 0; none is skipped: the groups are abelian)
            if n:
                M = dense_columns(torch, D.MatvecPlan(h, reps, torch.complex128), n, torch.complex128)
                assert np.abs(M - M.conj().T).max() < 1e-12
                got.extend(np.linalg.eigvalsh(M))
    assert total == nf
    assert np.abs(np.sort(got) - want).max() < 1e-10


def test_free_fermions_per_momentum_closed_form(torch):
    # 24 modes (32-bit words: f64 and c128 sectors, single-vector and block Lanczos), then 40 modes (64-bit words)
    for L, nu, nd, runs in ((12, 6, 5, ((0, 1), (6, 2), (5, 1), (5, 2))), (20, 2, 2, ((0, 1), (10, 2), (7, 1), (7, 2)))):
        model = hubbard_model(L, ring(L), U=0.0)
        for s, bs in runs:
            cfg = cfg_of(L, nu, nd, translations(L), [s], 0, model)
            dt = torch.complex128 if (2 * s) % L != 0 else torch.float64
            r = diagonalize(cfg, num_evals=1, eps=1e-9, dtype=dt, block_size=bs)
            want = free_spinful_ring_energy(L, nu, nd, s, free_ring_energy)
            assert abs(r.eigenvalues[0] - want) <= 1e-8, (L, nu, nd, s, bs, r.eigenvalues[0], want)


def test_ground_state_over_sectors_equals_the_unprojected_one(torch):
    L, nu, nd = 12, 6, 6
    model = hubbard_model(L, ring(L), U=4.0)
    full = {"basis": {"particle": "spinful-fermion", "number_sites": L, "number_particles": nu + nd, "number_up": nu},
            "hamiltonian": {"terms": yaml_terms(model, True)}}
    e0 = diagonalize(full, num_evals=1, eps=1e-10)
    best = min(diagonalize(cfg_of(L, nu, nd, translations(L), [s], f, model), num_evals=1, eps=1e-10,
                           dtype=torch.float64 if (2 * s) % L == 0 else torch.complex128).eigenvalues[0]
               for s in range(L) for f in (1, -1))
    assert abs(best - e0.eigenvalues[0]) <= 1e-9, (best, e0.eigenvalues[0])


def test_other_paths_are_refused_at_creation(torch, monkeypatch):
    L, nu, nd = 8, 3, 3
    model = hubbard_model(L, ring(L), U=2.0)
    basis, h, reps = enumerate_(torch, cfg_of(L, nu, nd, dihedral(L), [0, 0], 1, model))

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
    # a non-Hermitian operator: one directed hop per species
    nh = cfg_of(L, nu, nd, translations(L), [0], 0, [(-1.0, [("+", i, s), ("-", (i + 1) % L, s)]) for i in range(L) for s in (0, 1)])
    _, hn, rn = enumerate_(torch, nh)
    with pytest.raises(D.LsAmdError, match="non-Hermitian"):
        D.MatvecPlan(hn, rn, torch.float64)
    assert D.MatvecPlan(h, reps, torch.float64).kernel == "tile-pull+indexed"  # and the default still builds
    # 31 sites = 62 modes: no static index table (tag bits), and the hash-table pull has no signs
    _, h62, r62 = enumerate_(torch, cfg_of(31, 1, 1, translations(31), [0], 0, hubbard_model(31, ring(31))))
    assert int(r62[0].numel()) == 31
    with pytest.raises(D.LsAmdError, match="no static index table"):
        D.MatvecPlan(h62, r62, torch.float64)
