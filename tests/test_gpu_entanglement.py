"""Sector-state expansion and entanglement on the GPU (SectorExpansion / k_expand_push, unproject, reduced_density_matrix,
entanglement_spectrum, entanglement_entropy) against tests/entanglement_reference.py (pure numpy on oracle.model), the norm and
trace identities, an eigenvector check in the unprojected space beyond dense sizes, the analytic one- and two-site spectra of a
total singlet, and the failures that must be loud."""
import ctypes as C
import math

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
from distributed_matvec_amd import SectorExpansion  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from helpers import model_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _setup(cfg):
    basis = D.loadConfigFromDict({"basis": cfg["basis"]})
    reps, _ = D.enumerateStates(basis, 1)
    return basis, reps[0]


SCATTERED, ONE = [0, 2, 5, 7], [3]


def _sites(L, what):
    if what == "all":
        return None
    if what == "low":
        return list(range(L // 2))
    if what == "high":
        return list(range(L - L // 2, L))
    if what == "high3":
        return list(range(L - 3, L))
    return list(what)


# name: (basis config, dtype of psi, subsystems)
CASES = {
    "ring8_k0_f64": (lambda: E.ring(8, 4, 0), "f64", ["low", "all", SCATTERED]),
    "ring8_k1_zero_norm_orbits": (lambda: E.ring(8, 4, 1), "c128", ["all", "high", ONE]),
    "ring8_k3_promoted_f64": (lambda: E.ring(8, 4, 3), "f64", ["all", SCATTERED]),
    "ring12_k0_f64": (lambda: E.ring(12, 6, 0), "f64", ["low", "high", SCATTERED, ONE, "all"]),
    "ring12_k0_c128": (lambda: E.ring(12, 6, 0), "c128", ["high3", "all"]),
    "ring12_k5_c128": (lambda: E.ring(12, 6, 5), "c128", ["low", SCATTERED, "all"]),
    "ring16_k0_f64": (lambda: E.ring(16, 8, 0), "f64", ["low", "all"]),
    "ring16_k3_c128": (lambda: E.ring(16, 8, 3), "c128", ["high", SCATTERED]),
    "ring12_reflection_odd": (lambda: E.ring(12, 6, None, reflect=1), "f64", ["low", SCATTERED, "all"]),
    "ring12_inversion_plus_only": (lambda: E.ring(12, 6, None, inv=1), "f64", ["high", ONE, "all"]),
    "ring12_inversion_minus_only": (lambda: E.ring(12, 6, None, inv=-1), "f64", ["low", "all"]),
    "ring12_k0_reflection_inversion_plus": (lambda: E.ring(12, 6, 0, inv=1, reflect=0), "f64", ["low", SCATTERED, "all"]),
    "ring12_k6_reflection_inversion_minus": (lambda: E.ring(12, 6, 6, inv=-1, reflect=1), "c128", ["high", "all"]),
    "ring12_unprojected": (lambda: E.ring(12, 6, None), "f64", ["low", SCATTERED, "all"]),
    "ring12_unprojected_weight_4": (lambda: E.ring(12, 4, None), "c128", ["high", SCATTERED, ONE]),
    "chain10_all_weights_k1": (lambda: {"basis": {"number_spins": 10, "symmetries": [{"permutation": [(i + 1) % 10 for i in range(10)], "sector": 1}]}},
                               "c128", ["low", "high", SCATTERED, ONE, "all"]),
    "chain10_all_weights_unprojected": (lambda: {"basis": {"number_spins": 10, "symmetries": []}}, "f64", ["low", SCATTERED, "all"]),
    "square_4x4_lattice_group": (lambda: {"basis": model_config("heisenberg_square_4x4")["basis"]}, "f64", ["low", SCATTERED, "all"]),
    "ring34_weight_2_k0": (lambda: E.ring(34, 2, 0), "f64", ["low", "high", SCATTERED, "all"]),
    "ring34_weight_2_k5": (lambda: E.ring(34, 2, 5), "c128", ["high3", SCATTERED, "all"]),
    "ring20_translations_9252_rows": (lambda: E.ring(20, 10, 0), "f64", ["low", "all"]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_expand_matches_the_reference(torch, name):
    make, dt, subsystems = CASES[name]
    cfg = make()
    model, full, want_reps, _idx, _coef, live = E.tables(cfg)
    basis, reps = _setup(cfg)
    assert np.array_equal(_u64(reps), want_reps)
    if name == "ring20_translations_9252_rows":
        assert len(want_reps) == 9252 and len(want_reps) % 256 != 0
    if name == "ring8_k1_zero_norm_orbits":
        assert (~live).any()
    dtype = torch.complex128 if dt == "c128" else torch.float64
    psi = D.fillRandom(reps, 11, dtype)
    psi_np = psi.cpu().numpy()
    scale = float(np.abs(psi_np).max())
    vec = E.expand_full(cfg, psi_np)
    L = model.number_sites
    for what in subsystems:
        sites = _sites(L, what)
        want = E.bipartition(cfg, vec, sites)
        reached = E.bipartition(cfg, live.astype(np.float64), sites)
        ex = D.SectorExpansion(basis, reps, sites)
        assert ex.blocks == [(n, m.shape[0], m.shape[1]) for n, m in want], (name, what)
        got = ex.expand(psi)
        assert ex.kernel == "k_expand_push"
        worst = 0.0
        for g, (n, m), (_, r) in zip(got, want, reached):
            g = g.cpu().numpy()
            assert g.shape == m.shape and np.isfinite(g).all()
            worst = max(worst, float(np.abs(g - m).max()))
            assert (g[r == 0.0] == 0.0).all(), (name, what, n)  # states of zero-norm orbits read exactly 0
        print(f"expand {name} A={what}: {len(want_reps)} rows -> {len(full)} elements in {len(want)} blocks, max error {worst:.2e} "
              f"(bound {1e-13 * scale:.2e})")
        assert worst <= 1e-13 * scale, (name, what, worst)
        if sites is None:
            flat = D.unproject(basis, reps, psi)
            assert flat.dim() == 1 and flat.numel() == len(full)
            assert float(np.abs(flat.cpu().numpy() - vec).max()) <= 1e-13 * scale
        ex.destroy()


def test_selected_block_alone_and_the_rest_of_out_untouched(torch):
    cfg = E.ring(12, 6, 5)
    basis, reps = _setup(cfg)
    psi = D.fillRandom(reps, 5, torch.complex128)
    ex = D.SectorExpansion(basis, reps, [0, 2, 5, 7])
    assert [b[0] for b in ex.blocks] == [0, 1, 2, 3, 4]
    whole = [m.clone() for m in ex.expand(psi)]
    poison = complex(7.25, -3.5)
    out = torch.full((ex.total,), poison, dtype=torch.complex128, device=psi.device)
    views = ex.expand(psi, blocks=[2], out=out)
    assert torch.equal(views[2], whole[2])
    for i in (0, 1, 3, 4):
        assert bool((views[i] == poison).all()), i
    lo, hi = ex.offsets[2], ex.offsets[3]
    assert bool((out[:lo] == poison).all()) and bool((out[hi:] == poison).all())
    # a run of blocks, and a single block without a buffer of the caller's
    views = ex.expand(psi, blocks=[1, 2, 3], out=out)
    assert all(torch.equal(views[i], whole[i]) for i in (1, 2, 3)) and bool((views[0] == poison).all()) and bool((views[4] == poison).all())
    alone = ex.expand(psi, blocks=3)
    assert alone[0] is None and alone[4] is None and torch.equal(alone[3], whole[3])
    ex.destroy()


@pytest.mark.parametrize("name", ["ring12_k5_c128", "ring16_k0_f64", "square_4x4_lattice_group", "ring34_weight_2_k5"])
def test_norm_and_trace_are_preserved(torch, name):
    make, dt, _ = CASES[name]
    cfg = make()
    basis, reps = _setup(cfg)
    psi = D.fillRandom(reps, 3, torch.complex128 if dt == "c128" else torch.float64)
    psi = psi / torch.linalg.vector_norm(psi)
    full = D.unproject(basis, reps, psi)
    assert abs(float(torch.linalg.vector_norm(full)) - 1.0) <= 1e-12
    L = cfg["basis"]["number_spins"]
    for sites in (list(range(L // 2)), [0, 2, 5, 7]):
        blocks = D.reduced_density_matrix(basis, reps, psi, sites)
        tr = sum(float(torch.diagonal(rho).real.sum()) for _, rho in blocks)
        assert abs(tr - 1.0) <= 1e-12, (name, sites, tr)
        for na, rho in blocks:
            assert rho.shape[0] == rho.shape[1] == math.comb(len(sites), na)
            assert float((rho - rho.conj().transpose(0, 1)).abs().max()) <= 1e-15


def test_expanded_ground_state_is_an_eigenvector_of_the_unprojected_hamiltonian(torch):
    """20-site ring, sector (k = 0, reflection even, inversion +1): 184 756 states without symmetries, no dense matrix anywhere.
    The isometry commutes with H, so the residual in the full space equals the residual in the sector up to rounding:
    1e-10 x sum |coefficients of H| (3 Pauli products of coefficient 1 on each of the 20 bonds)."""
    from distributed_matvec_amd.diagonalize import diagonalize

    L = 20
    cfg = config.heisenberg_chain_config(L, symm=True)
    r = diagonalize(cfg, num_evals=1, eps=1e-10)
    e0, psi = r.eigenvalues[0], r.eigenvectors[0]
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    hpsi = torch.zeros_like(psi)
    D.MatvecPlan(h, reps, psi.dtype).matvec([psi], [hpsi])
    res_sector = float(torch.linalg.vector_norm(hpsi - e0 * psi))
    phi = D.unproject(basis, reps[0], psi)
    fbasis, fh = D.loadConfigFromDict(config.heisenberg_chain_config(L), hamiltonian=True)
    freps, _ = D.enumerateStates(fbasis, 1)
    assert phi.numel() == freps[0].numel() == math.comb(L, L // 2)
    hphi = torch.zeros_like(phi)
    D.MatvecPlan(fh, freps, phi.dtype).matvec([phi], [hphi])
    res_full = float(torch.linalg.vector_norm(hphi - e0 * phi))
    coefficient_sum = 3.0 * L
    print(f"E0 = {e0:.12f}: residual in the sector {res_sector:.3e}, in the full space {res_full:.3e}, |phi| = {float(torch.linalg.vector_norm(phi)):.15f}")
    assert abs(float(torch.linalg.vector_norm(phi)) - float(torch.linalg.vector_norm(psi))) <= 1e-12
    assert abs(res_full - res_sector) <= 1e-10 * coefficient_sum
    assert res_full <= 1e-6 * coefficient_sum  # (and it IS an eigenvector: the solver converged to eps = 1e-10)


@pytest.fixture(scope="module")
def ring12_ground_state(torch):
    from distributed_matvec_amd.diagonalize import diagonalize

    cfg = config.heisenberg_chain_config(12, symm=True)  # the (0, 0, +1) sector: momentum 0, reflection even, inversion +1
    r = diagonalize(cfg, num_evals=1, eps=1e-12)
    basis, reps = _setup(cfg)
    psi = r.eigenvectors[0]
    psi = psi / torch.linalg.vector_norm(psi)
    return cfg, basis, reps, psi, E.expand_full(cfg, psi.cpu().numpy())


@pytest.mark.parametrize("what", ["half", "A025", "complement_of_A025"])
def test_entanglement_of_the_ring12_ground_state(torch, ring12_ground_state, what):
    cfg, basis, reps, psi, vec = ring12_ground_state
    sites = {"half": [0, 1, 2, 3, 4, 5], "A025": [0, 2, 5], "complement_of_A025": [1, 3, 4, 6, 7, 8, 9, 10, 11]}[what]
    want, want_na = E.spectrum(E.bipartition(cfg, vec, sites))
    got, got_na = D.entanglement_spectrum(basis, reps, psi, sites)
    assert (np.diff(got) <= 0).all() and got.min() >= 0.0
    big = want > 1e-12
    k = int(big.sum())
    assert k > 0 and (got[k:] <= 1e-12 + 1e-10).all()
    print(f"ring12 {what}: {k} eigenvalues above 1e-12, max deviation {np.abs(got[:k] - want[:k]).max():.2e}")
    assert np.abs(got[:k] - want[:k]).max() <= 1e-10
    gaps = want[:k - 1] - want[1:k]
    clear = np.concatenate([[True], gaps > 1e-9]) & np.concatenate([gaps > 1e-9, [True]])  # (degenerate values may swap their n_a)
    assert np.array_equal(got_na[:k][clear], want_na[:k][clear])
    for q in (1.0, 2.0, 0.5):
        s = D.entanglement_entropy(basis, reps, psi, sites, renyi=q)
        assert abs(s - E.entropy(want, q)) <= 1e-10, (what, q, s)
    # Renyi-2 is -ln Tr rho^2, straight from the blocks of rho
    tr2 = sum(float((rho.abs() ** 2).sum()) for _, rho in D.reduced_density_matrix(basis, reps, psi, sites))
    assert abs(D.entanglement_entropy(basis, reps, psi, sites, renyi=2.0) + math.log(tr2)) <= 1e-10
    if what == "half":
        assert abs(D.entanglement_entropy(cfg, sites, state=psi) - E.entropy(want, 1.0)) <= 1e-10
        assert abs(D.entanglement_entropy(cfg, sites) - E.entropy(want, 1.0)) <= 1e-8  # (its own Lanczos run, eps = 1e-10)


def test_entropy_of_a_subsystem_equals_that_of_its_complement(torch, ring12_ground_state):
    """|A| = 3 against |B| = 9: blocks of 1 x 84 ... 1 x 84 on one side, their transposes on the other"""
    cfg, basis, reps, psi, _ = ring12_ground_state
    a, b = [0, 2, 5], [1, 3, 4, 6, 7, 8, 9, 10, 11]
    assert [blk[1:] for blk in D.SectorExpansion(basis, reps, a).blocks] == [blk[:0:-1] for blk in D.SectorExpansion(basis, reps, b).blocks][::-1]
    for q in (1.0, 2.0):
        sa, sb = D.entanglement_entropy(basis, reps, psi, a, renyi=q), D.entanglement_entropy(basis, reps, psi, b, renyi=q)
        assert sa > 0.1 and abs(sa - sb) <= 1e-10, (q, sa, sb)
    # the full matrices of rho_A (8 x 8 in blocks) and of rho_B on its smaller side have the same non-zero spectrum
    rho_b = D.reduced_density_matrix(basis, reps, psi, b)
    assert [r.shape[0] for _, r in rho_b] == [math.comb(9, n) for n, _ in rho_b]
    rho_b_small = D.reduced_density_matrix(basis, reps, psi, b, smaller=True)
    assert [r.shape[0] for _, r in rho_b_small] == [min(math.comb(9, n), math.comb(3, 6 - n)) for n, _ in rho_b_small]


def test_singlet_spectra_of_the_ring16_ground_state(torch):
    """The ground state of the 16-site ring is a total singlet.  One site: rho = 1/2, S = ln 2.  Two neighbours: the singlet weight is
    p_s = <(1 - s.s) / 4> = (1 - E0 / L) / 4 with E0 = sum over the L bonds of <s.s>, and the three triplet weights are equal."""
    from distributed_matvec_amd.diagonalize import diagonalize

    L = 16
    cfg = config.heisenberg_chain_config(L, symm=True)
    r = diagonalize(cfg, num_evals=1, eps=1e-10)
    e0, psi, res = r.eigenvalues[0], r.eigenvectors[0], float(r.residual_norms[0])
    basis, reps = _setup(cfg)
    psi = psi / torch.linalg.vector_norm(psi)
    one, na = D.entanglement_spectrum(basis, reps, psi, [5])
    print(f"ring16: E0 = {e0:.12f}, residual {res:.2e}; one site {one}, n_a {na}")
    assert len(one) == 2 and np.abs(one - 0.5).max() <= 1e-10 and sorted(na) == [0, 1]
    assert abs(D.entanglement_entropy(basis, reps, psi, [5]) - math.log(2.0)) <= 1e-10
    two, na2 = D.entanglement_spectrum(basis, reps, psi, [7, 8])
    p_s = (1.0 - e0 / L) / 4.0
    tol = 10.0 * res + 1e-10
    print(f"ring16: two neighbours {two}, n_a {na2}; p_s = {p_s:.12f}, triplets {(1.0 - p_s) / 3.0:.12f}, tolerance {tol:.2e}")
    assert len(two) == 4 and sorted(na2) == [0, 1, 1, 2] and na2[0] == 1
    assert abs(two[0] - p_s) <= tol and np.abs(two[1:] - (1.0 - p_s) / 3.0).max() <= tol


def test_errors_are_loud(torch):
    cfg = E.ring(12, 6, 5)
    basis, reps = _setup(cfg)
    n = reps.numel()
    # representatives of another weight sector: the images leave the basis, check() says so, nothing is stored out of range
    _, other = _setup(E.ring(12, 5, 5))
    ex = D.SectorExpansion(basis, other, [0, 1, 2, 3, 4, 5])
    psi = D.fillRandom(other, 1, torch.complex128)
    with pytest.raises(D.LsAmdError, match="not a state of the basis"):
        ex.expand(psi)
    ex.check()  # the flag is cleared by the report
    ex.destroy()
    # f64 with complex characters: refused by ls_amd_expand_apply itself
    ex = D.SectorExpansion(basis, reps, [0, 1, 2, 3, 4, 5])
    from distributed_matvec_amd import _lib

    Lc = _lib.load()
    x = torch.zeros(n, dtype=torch.float64, device=reps.device)
    out = torch.zeros(ex.total, dtype=torch.float64, device=reps.device)
    rc = Lc.ls_amd_expand_apply(ex._plan(), 0, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0, len(ex.blocks), None)
    assert rc == -1 and "f64 needs +-1 characters" in Lc.ls_amd_last_error().decode()
    assert Lc.ls_amd_expand_apply(ex._plan(), 1, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 3, len(ex.blocks), None) == -1
    assert Lc.ls_amd_expand_num_blocks(ex._plan()) == len(ex.blocks) and Lc.ls_amd_expand_total(ex._plan()) == ex.total == math.comb(12, 6)
    na, rows, cols, off = C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
    assert Lc.ls_amd_expand_block(ex._plan(), 2, C.byref(na), C.byref(rows), C.byref(cols), C.byref(off)) == 0
    assert (na.value, rows.value, cols.value, off.value) == (ex.blocks[2] + (ex.offsets[2],))
    assert Lc.ls_amd_expand_block(ex._plan(), len(ex.blocks), None, None, None, None) == -1
    # wrong shapes of psi
    good = D.fillRandom(reps, 1, torch.complex128)
    with pytest.raises(D.LsAmdError, match="ONE vector"):
        ex.expand(torch.stack([good, good], dim=1))
    with pytest.raises(D.LsAmdError, match=f"{n - 1} elements"):
        ex.expand(good[:-1])
    with pytest.raises(D.LsAmdError, match="neither float64 nor complex128"):
        ex.expand(good.to(torch.complex64))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        ex.expand(good.cpu())
    with pytest.raises(D.LsAmdError, match="out must be"):
        ex.expand(good, out=torch.zeros(ex.total - 1, dtype=torch.complex128, device=reps.device))
    # max_bytes: the size and the way out are in the message
    with pytest.raises(D.LsAmdError, match=rf"{ex.total * 16} bytes.*blocks="):
        ex.expand(good, max_bytes=1000)
    b = 3
    need = ex.blocks[b][1] * ex.blocks[b][2] * 16
    assert ex.expand(good, blocks=b, max_bytes=need)[b].shape == ex.blocks[b][1:]
    with pytest.raises(D.LsAmdError, match="max_bytes"):
        ex.expand(good, blocks=b, max_bytes=need - 1)
    ex.destroy()
