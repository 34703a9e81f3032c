"""Expansion and entanglement of fermionic sector states on the GPU (FermionSectorExpansion / k_expand_push_fermi, fermion_unproject,
reduced_density_matrix, entanglement_spectrum, entanglement_entropy) against tests/fermion_entanglement_reference.py (projector
columns @ psi over the unprojected states, the bipartition sign counted pair by pair): the expansion itself, the order of the
unprojected vector, an eigenvector check in the unprojected space beyond dense sizes (fails when an orbit sign is wrong), the
one-body identity Tr(rho_A c+_i c_j) = <psi|c+_i c_j|psi> on interacting states and Peschel's formula for free fermions (both fail
when the bipartition sign is missing or has the other orientation), the conventions of the spectrum, and the failures that must be
loud."""
import ctypes as C
import math

import numpy as np
import pytest

import distributed_matvec_amd as D
import fermion_entanglement_reference as R
import fermion_jw as JW
import fermion_symm as F
from distributed_matvec_amd import FermionSectorExpansion  # noqa: F401  (the feature under test: without it nothing here can run)

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


def _setup(case, model=None):
    cfg = case.config(model)
    if model is None:
        basis = D.loadConfigFromDict(cfg)
        h = None
    else:
        basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    return basis, h, reps


def _subsystem(case, what):
    """keyword arguments of FermionSectorExpansion: lattice sites, or (one case) the modes of one species"""
    L = case.L
    if what == "all":
        return {}
    if what == "low":
        return dict(sites=list(range(L // 2)))
    if what == "high":
        return dict(sites=list(range(L - L // 2, L)))
    if what == "one":
        return dict(sites=[3])
    if what == "scattered":
        return dict(sites=[0, 2, 5, 7] if L >= 8 else [0, 2, 3])
    if what == "up_modes":
        return dict(modes=[0, 2, 3])
    if what == "mixed_modes":
        return dict(modes=[1, 4, L + 0, L + 4, L + 5])
    raise KeyError(what)


EVERY = ["low", "high", "scattered", "one", "all"]
# name: (case, dtype of psi, subsystems)
CASES = {
    "ring8_k0_zero_norm_orbits_f64": (lambda: R.Case(8, 4, gens=F.translations(8), secs=[0]), "f64", EVERY),
    "ring8_k1_c128": (lambda: R.Case(8, 4, gens=F.translations(8), secs=[1]), "c128", EVERY),
    "ring8_k3_promoted_f64": (lambda: R.Case(8, 4, gens=F.translations(8), secs=[3]), "f64", EVERY),
    "ring10_dihedral_reflection_odd": (lambda: R.Case(10, 5, gens=F.dihedral(10), secs=[0, 1]), "f64", EVERY),
    "ring10_unprojected": (lambda: R.Case(10, 5), "f64", EVERY),
    "ring10_every_number_k1": (lambda: R.Case(10, None, gens=F.translations(10), secs=[1]), "c128", EVERY),
    "torus_4x3_point_group": (lambda: R.Case(12, 5, gens=R.torus_point_group(4, 3), secs=[0, 0, 1, 0]), "f64", EVERY),
    "ring34_two_particles_k5": (lambda: R.Case(34, 2, gens=F.translations(34), secs=[5]), "c128", EVERY),
    "ring16_k0_more_than_256_rows": (lambda: R.Case(16, 8, gens=F.translations(16), secs=[0]), "f64", ["scattered", "all"]),
    "spinful6_unprojected": (lambda: R.Case(6, up=(3, 3)), "f64", EVERY),
    "spinful6_k0": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0]), "f64", EVERY + ["up_modes"]),
    "spinful6_k2": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2]), "c128", EVERY + ["mixed_modes"]),
    "spinful6_dihedral": (lambda: R.Case(6, up=(3, 3), gens=F.dihedral(6), secs=[0, 1]), "f64", EVERY),
    "spinful6_k0_flip_plus": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1), "f64", EVERY),
    "spinful6_k1_flip_minus": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[1], flip=-1), "c128", EVERY),
    "spinful17_one_up_one_down": (lambda: R.Case(17, up=(1, 1), gens=F.translations(17), secs=[3]), "c128", EVERY),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_expand_matches_the_reference(torch, name):
    make, dt, subsystems = CASES[name]
    case = make()
    basis, _, reps = _setup(case)
    assert np.array_equal(_u64(reps[0]), case.reps)
    if name == "ring8_k0_zero_norm_orbits_f64":
        assert (~case.live).any()  # fermions: the sector k = 0 is the one with vanishing orbits (0101 0101 under T^2)
    if name == "ring16_k0_more_than_256_rows":
        assert len(case.reps) > 256 and len(case.reps) % 256 != 0
    if name == "ring34_two_particles_k5":
        assert int(case.states.max()) >> 32  # the words cross bit 32
    if name == "spinful17_one_up_one_down":
        assert len(case.states) == 289 and case.M == 34
    dtype = torch.complex128 if dt == "c128" else torch.float64
    psi = D.fillRandom(reps[0], 11, dtype)
    psi_np = psi.cpu().numpy()
    scale = float(np.abs(psi_np).max())
    vec = case.full_vector(psi_np)
    for what in subsystems:
        sub = _subsystem(case, what)
        a_modes = case.modes_of(**sub)
        want = R.bipartition(case, vec, a_modes)
        reached = R.bipartition(case, case.live.astype(np.float64), a_modes, signed=False)
        ex = D.FermionSectorExpansion(basis, reps[0], **sub)
        assert ex.blocks == [(lab, m.shape[0], m.shape[1]) for lab, m in want], (name, what)
        got = ex.expand(psi)
        assert ex.kernel == "k_expand_push_fermi"
        worst = 0.0
        for g, (lab, m), (_, r) in zip(got, want, reached):
            g = g.cpu().numpy()
            assert g.shape == m.shape and np.isfinite(g).all()
            worst = max(worst, float(np.abs(g - m).max()))
            assert (g[r == 0.0] == 0.0).all(), (name, what, lab)  # states of zero-norm orbits read exactly 0
        print(f"expand {name} A={what}: {len(case.reps)} rows -> {len(case.states)} elements in {len(want)} blocks, max error {worst:.2e} "
              f"(bound {1e-13 * scale:.2e})")
        assert worst <= 1e-13 * scale, (name, what, worst)
        if not sub:
            flat = D.fermion_unproject(basis, reps[0], psi)
            assert flat.dim() == 1 and flat.numel() == len(case.states)
            assert float(np.abs(flat.cpu().numpy() - vec).max()) <= 1e-13 * scale
        ex.destroy()


def test_unprojected_vector_has_the_order_of_the_plain_basis(torch):
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2], flip=-1)
    basis, _, reps = _setup(case)
    _, _, plain = _setup(case.plain())
    assert np.array_equal(_u64(plain[0]), case.states) and len(case.states) == 400
    psi = D.fillRandom(reps[0], 2, torch.complex128)
    flat = D.fermion_unproject(basis, reps[0], psi)
    assert flat.numel() == plain[0].numel()
    want = case.full_vector(psi.cpu().numpy())
    assert float(np.abs(flat.cpu().numpy() - want).max()) <= 1e-13 * float(psi.abs().max())
    # the plain basis expands onto itself
    x = D.fillRandom(plain[0], 3, torch.float64)
    pbasis = D.loadConfigFromDict(case.plain().config())
    assert torch.equal(D.fermion_unproject(pbasis, plain[0], x), x)


FULL_SPACE = {
    # (case, model, sum of |coefficients|)
    "tv_ring20_translations_reflection": (lambda: R.Case(20, 10, gens=F.dihedral(20), secs=[0, 0]), lambda: F.tv_model(JW.ring(20), V=1.3),
                                          20 * (2.0 + 1.3)),
    "hubbard_ring8_translations_flip": (lambda: R.Case(8, up=(4, 4), gens=F.translations(8), secs=[0], flip=1),
                                        lambda: JW.hubbard_model(8, JW.ring(8), U=4.0), 8 * (4.0 + 4.0)),
}


@pytest.mark.parametrize("name", sorted(FULL_SPACE))
def test_expanded_ground_state_is_an_eigenvector_of_the_unprojected_hamiltonian(torch, name):
    """No dense matrix anywhere (t-V: 184 756 states without symmetries).  The isometry commutes with H, so the residual in the full
    space equals the residual in the sector up to rounding: 1e-10 x sum |coefficients of H|.  A wrong orbit sign breaks it."""
    from distributed_matvec_amd.diagonalize import diagonalize

    make, make_model, coefficient_sum = FULL_SPACE[name]
    case, model = make(), make_model()
    r = diagonalize(case.config(model), num_evals=1, eps=1e-10)
    e0, psi = r.eigenvalues[0], r.eigenvectors[0]
    basis, h, reps = _setup(case, model)
    hpsi = torch.zeros_like(psi)
    D.MatvecPlan(h, reps, psi.dtype).matvec([psi], [hpsi])
    res_sector = float(torch.linalg.vector_norm(hpsi - e0 * psi))
    phi = D.fermion_unproject(basis, reps[0], psi)
    _, fh, freps = _setup(case.plain(), model)
    want = math.comb(20, 10) if not case.spinful else math.comb(8, 4) ** 2
    assert phi.numel() == freps[0].numel() == want
    hphi = torch.zeros_like(phi)
    D.MatvecPlan(fh, freps, phi.dtype).matvec([phi], [hphi])
    res_full = float(torch.linalg.vector_norm(hphi - e0 * phi))
    print(f"{name}: E0 = {e0:.12f}: residual in the sector {res_sector:.3e}, in the full space {res_full:.3e}, "
          f"|phi| = {float(torch.linalg.vector_norm(phi)):.15f}")
    assert abs(float(torch.linalg.vector_norm(phi)) - float(torch.linalg.vector_norm(psi))) <= 1e-12
    assert abs(res_full - res_sector) <= 1e-10 * coefficient_sum
    assert res_full <= 1e-6 * coefficient_sum  # (and it IS an eigenvector: the solver converged to eps = 1e-10)


def _assemble_rho(case, a_modes, blocks):
    """rho_A over the 2^|A| compacted words from the blocks of reduced_density_matrix"""
    rho = np.zeros((1 << len(a_modes),) * 2, dtype=complex)
    for lab, blk in blocks:
        w = R.block_words(case, a_modes, lab).astype(np.int64)
        blk = blk.cpu().numpy()
        assert blk.shape == (len(w), len(w))
        rho[np.ix_(w, w)] = blk
    return rho


ONE_BODY = {
    "tv_ring10_V1.3_k0": (lambda: R.Case(10, 5, gens=F.translations(10), secs=[0]), lambda: F.tv_model(JW.ring(10), V=1.3), dict(sites=[0, 2, 5, 7])),
    "hubbard_ring6_U4_flip_plus": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1),
                                   lambda: JW.hubbard_model(6, JW.ring(6), U=4.0), dict(sites=[0, 2, 3])),
    "hubbard_ring6_U4_flip_plus_mixed_modes": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1),
                                               lambda: JW.hubbard_model(6, JW.ring(6), U=4.0), dict(modes=[1, 4, 6, 10, 11])),
}


@pytest.mark.parametrize("name", sorted(ONE_BODY))
def test_one_body_expectations_from_the_reduced_density_matrix(torch, name):
    """Tr(rho_A c+_i c_j) = <psi|c+_i c_j|psi> for all i, j in a scattered A, the operators on A by Jordan-Wigner over A's own
    compacted modes: the test of the bipartition sign (without sigma, or with the other orientation, the strings over the modes of
    B between two modes of A are lost)."""
    make, make_model, sub = ONE_BODY[name]
    case, model = make(), make_model()
    _, psi_np = case.ground_state(model)
    vec = case.full_vector(psi_np)
    basis, _, reps = _setup(case)
    assert np.array_equal(_u64(reps[0]), case.reps)
    psi = torch.from_numpy(psi_np).cuda()
    a_modes = case.modes_of(**sub)
    blocks = D.reduced_density_matrix(basis, reps[0], psi, sub.get("sites"), modes=sub.get("modes"))
    for _, blk in blocks:
        assert float((blk - blk.conj().transpose(0, 1)).abs().max()) <= 1e-15
    rho = _assemble_rho(case, a_modes, blocks)
    assert abs(np.trace(rho) - 1.0) <= 1e-12
    k = len(a_modes)
    c = [JW.annihilator(q, k) for q in range(k)]
    worst, strings = 0.0, 0
    for qi, i in enumerate(a_modes):
        for qj, j in enumerate(a_modes):
            got = np.trace(rho @ (c[qi].T @ c[qj]).toarray())
            want = R.one_body(case, vec, i, j)
            worst = max(worst, abs(got - want))
            strings += abs(want) > 1e-3 and any(m not in a_modes for m in range(min(i, j) + 1, max(i, j)))
    print(f"{name}: A = {a_modes}, max |Tr(rho c+c) - <c+c>| = {worst:.2e}; {strings} sizeable elements whose string crosses B")
    assert strings > 0  # (else the subsystem would not see the sign)
    assert worst <= 1e-12


PESCHEL = {
    "spinless10_A0257": (lambda: R.Case(10, 5, gens=F.translations(10), secs=[0]), [0, 2, 5, 7]),
    "spinless10_A146": (lambda: R.Case(10, 5, gens=F.translations(10), secs=[0]), [1, 4, 6]),
    "spinful6_sites023": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0]), [0, 2, 3]),
}


def _free(case):
    return JW.hubbard_model(case.L, JW.ring(case.L), U=0.0) if case.spinful else F.tv_model(JW.ring(case.L))


@pytest.fixture(scope="module")
def free_ground_states():
    """{spinful: (case, psi of the closed-shell ground state by numpy eigh of the reference's sector matrix)}"""
    out = {}
    for name in ("spinless10_A0257", "spinful6_sites023"):
        case = PESCHEL[name][0]()
        w = np.linalg.eigvalsh(case.sector_matrix(_free(case)))
        assert w[1] - w[0] > 1e-6  # a closed shell: the ground state is alone
        out[case.spinful] = (case, case.ground_state(_free(case))[1])
    return out


@pytest.mark.parametrize("name", sorted(PESCHEL))
def test_free_fermion_entropy_is_peschels(torch, free_ground_states, name):
    """V = 0 (U = 0): the entropy of a scattered subsystem from the correlation matrix C = projector on the N lowest orbitals,
    restricted to A.  Without the bipartition sign the same inputs are off by 0.3 to 0.5."""
    sites = PESCHEL[name][1]
    case, psi_np = free_ground_states[PESCHEL[name][0]().spinful]
    n_orb = case.up[0] if case.spinful else case.N
    want = R.peschel_entropy(R.ring_hopping(case.L), n_orb, sites) * (2 if case.spinful else 1)  # (two independent species)
    basis, _, reps = _setup(case)
    psi = torch.from_numpy(psi_np).cuda()
    got = D.entanglement_entropy(basis, reps[0], psi, sites)
    unsigned = R.entropy(R.spectrum(R.bipartition(case, case.full_vector(psi_np), case.modes_of(sites=sites), signed=False))[0])
    print(f"{name}: S = {got:.14f}, Peschel {want:.14f} (difference {abs(got - want):.2e}); without sigma {unsigned:.6f}")
    assert abs(unsigned - want) > 0.1  # (the subsystem does see the sign)
    assert abs(got - want) <= 1e-10
    if name != "spinless10_A146":
        # the config form with its own Lanczos run (eps = 1e-10)
        assert abs(D.entanglement_entropy(case.config(_free(case)), sites) - want) <= 1e-8


def _hubbard_slow_down_species(L, U, t_dn):
    """the Hubbard ring with the hopping of the down species scaled by t_dn: no symmetry between the species is left"""
    return [(coef * t_dn if len(ops) == 2 and ops[0][0] == "+" and ops[0][2] == 1 else coef, ops) for coef, ops in JW.hubbard_model(L, JW.ring(L), U=U)]


# (the labels need eigenvalues that stand alone.  In the flip sector of ONE_BODY the blocks (n_up, n_dn) and (n_dn, n_up) carry the same
# eigenvalues pair by pair, and the SU(2)-symmetric ring keeps its eigenvalues in pairs too; two up and two down particles at momentum 1
# with a slower down species have nine of their 29 eigenvalues alone)
SPECTRUM = {
    "tv_ring10_V1.3_k0": ONE_BODY["tv_ring10_V1.3_k0"],
    "hubbard_ring6_2up_2down_k1_slow_down_species": (lambda: R.Case(6, up=(2, 2), gens=F.translations(6), secs=[1]),
                                                     lambda: _hubbard_slow_down_species(6, 4.0, 0.6), dict(sites=[0, 2, 3])),
}


@pytest.mark.parametrize("name", sorted(SPECTRUM))
def test_spectrum_conventions(torch, name):
    make, make_model, sub = SPECTRUM[name]
    case, model = make(), make_model()
    _, psi_np = case.ground_state(model)
    vec = case.full_vector(psi_np)
    basis, _, reps = _setup(case)
    psi = torch.from_numpy(psi_np).cuda()
    sites = sub["sites"]
    rest = [s for s in range(case.L) if s not in sites]
    want, want_lab = R.spectrum(R.bipartition(case, vec, case.modes_of(sites=sites)))
    got, got_lab = D.entanglement_spectrum(basis, reps[0], psi, sites)
    assert (np.diff(got) <= 0).all() and got.min() >= 0.0
    assert got_lab.shape == ((len(got), 2) if case.spinful else (len(got),))
    big = want > 1e-12
    k = int(big.sum())
    assert k > 0 and (got[k:] <= 1e-12 + 1e-10).all()
    assert np.abs(got[:k] - want[:k]).max() <= 1e-10
    gaps = want[:k - 1] - want[1:k]
    clear = np.concatenate([[True], gaps > 1e-9]) & np.concatenate([gaps > 1e-9, [True]])  # (degenerate values may swap their labels)
    assert int(clear.sum()) >= 6
    for i in np.nonzero(clear)[0]:
        assert (tuple(int(v) for v in got_lab[i]) if case.spinful else int(got_lab[i])) == want_lab[i], i
    sa, sb = D.entanglement_entropy(basis, reps[0], psi, sites), D.entanglement_entropy(basis, reps[0], psi, rest)
    assert sa > 0.1 and abs(sa - sb) <= 1e-10 and abs(sa - R.entropy(want)) <= 1e-10
    # modes= of the same subsystem is the same thing
    assert abs(D.entanglement_entropy(basis, reps[0], psi, None, modes=case.modes_of(sites=sites)) - sa) <= 1e-14


@pytest.mark.parametrize("spinful", [False, True])
def test_selected_block_alone_and_the_rest_of_out_untouched(torch, spinful):
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2]) if spinful else R.Case(10, 5, gens=F.translations(10), secs=[3])
    basis, _, reps = _setup(case)
    psi = D.fillRandom(reps[0], 5, torch.complex128)
    ex = D.FermionSectorExpansion(basis, reps[0], sites=[0, 2, 3] if spinful else [0, 2, 5, 7])
    nb = len(ex.blocks)
    assert nb == (16 if spinful else 5)
    whole = [m.clone() for m in ex.expand(psi)]
    poison = complex(7.25, -3.5)
    out = torch.full((ex.total,), poison, dtype=torch.complex128, device=psi.device)
    b = 6 if spinful else 2  # spinful: (n_up, n_dn) = (1, 2), in the middle of the table
    views = ex.expand(psi, blocks=[b], out=out)
    assert torch.equal(views[b], whole[b]) and bool((whole[b] != 0).any())
    for i in range(nb):
        if i != b:
            assert bool((views[i] == poison).all()), i
    lo, hi = ex.offsets[b], ex.offsets[b + 1]
    assert bool((out[:lo] == poison).all()) and bool((out[hi:] == poison).all())
    # a run of blocks (spinful: across n_up), and a single block without a buffer of the caller's
    run = [2, 3, 4, 5] if spinful else [1, 2, 3]
    views = ex.expand(psi, blocks=run, out=out)
    assert all(torch.equal(views[i], whole[i]) for i in run + [b])
    assert bool((views[0] == poison).all()) and bool((views[nb - 1] == poison).all())
    alone = ex.expand(psi, blocks=3)
    assert alone[0] is None and alone[4] is None and torch.equal(alone[3], whole[3])
    ex.destroy()


def test_errors_are_loud(torch):
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2])
    basis, _, reps = _setup(case)
    reps = reps[0]
    n = reps.numel()
    from distributed_matvec_amd import _lib

    Lc = _lib.load()
    # representatives of another particle-number sector: (2, 4) has the particle number of (3, 3), but neither half's
    for other_case in (R.Case(6, up=(2, 4), gens=F.translations(6), secs=[2]), R.Case(6, up=(3, 2), gens=F.translations(6), secs=[2])):
        _, _, other = _setup(other_case)
        ex = D.FermionSectorExpansion(basis, other[0], sites=[0, 1, 2])
        psi = D.fillRandom(other[0], 1, torch.complex128)
        with pytest.raises(D.LsAmdError, match="not a state of the basis"):
            ex.expand(psi)
        ex.check()  # the flag is cleared by the report
        ex.destroy()
    sl = R.Case(10, 5, gens=F.translations(10), secs=[3])
    sbasis, _, _ = _setup(sl)
    _, _, other = _setup(R.Case(10, 4, gens=F.translations(10), secs=[3]))
    ex = D.FermionSectorExpansion(sbasis, other[0], sites=[0, 2, 5, 7])
    with pytest.raises(D.LsAmdError, match="not a state of the basis"):
        ex.expand(D.fillRandom(other[0], 1, torch.complex128))
    ex.check()
    ex.destroy()
    # f64 with complex characters: refused by ls_amd_expand_apply itself
    ex = D.FermionSectorExpansion(basis, reps, sites=[0, 1, 2])
    x = torch.zeros(n, dtype=torch.float64, device=reps.device)
    out = torch.zeros(ex.total, dtype=torch.float64, device=reps.device)
    rc = Lc.ls_amd_expand_apply(ex._plan(), 0, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 0, len(ex.blocks), None)
    assert rc == -1 and "f64 needs +-1 characters" in Lc.ls_amd_last_error().decode()
    assert Lc.ls_amd_expand_apply(ex._plan(), 1, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 3, len(ex.blocks), None) == -1
    assert Lc.ls_amd_expand_num_blocks(ex._plan()) == len(ex.blocks) == 16 and Lc.ls_amd_expand_total(ex._plan()) == ex.total == 400
    na, nu, nd, rows, cols, off = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64(), C.c_int64()
    assert Lc.ls_amd_fermi_expand_block(ex._plan(), 6, C.byref(nu), C.byref(nd), C.byref(rows), C.byref(cols), C.byref(off)) == 0
    assert ((nu.value, nd.value), rows.value, cols.value, off.value) == (ex.blocks[6] + (ex.offsets[6],)) and (nu.value, nd.value) == (1, 2)
    assert Lc.ls_amd_expand_block(ex._plan(), 6, C.byref(na), C.byref(rows), C.byref(cols), C.byref(off)) == 0
    assert (na.value, rows.value, cols.value, off.value) == (3, ex.blocks[6][1], ex.blocks[6][2], ex.offsets[6])  # n_a = n_up + n_dn
    assert Lc.ls_amd_fermi_expand_block(ex._plan(), len(ex.blocks), None, None, None, None, None) == -1
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
    b = 5
    need = ex.blocks[b][1] * ex.blocks[b][2] * 16
    assert ex.expand(good, blocks=b, max_bytes=need)[b].shape == ex.blocks[b][1:]
    with pytest.raises(D.LsAmdError, match="max_bytes"):
        ex.expand(good, blocks=b, max_bytes=need - 1)
    ex.destroy()
    # a spin basis, by name; and the spin plan of a fermionic basis stays refused
    spin = D.loadConfigFromDict({"basis": {"number_spins": 8, "hamming_weight": 4}})
    sreps, _ = D.enumerateStates(spin, 1)
    with pytest.raises(D.LsAmdError, match="spin-1/2"):
        D.FermionSectorExpansion(spin, sreps[0], [0, 1])
    h = C.c_void_p()
    assert Lc.ls_amd_fermi_expand_create(C.byref(h), spin.payload, C.c_void_p(sreps[0].data_ptr()), sreps[0].numel(), C.c_uint64(3), None) == -1
    assert "spin-1/2" in Lc.ls_amd_last_error().decode() and h.value is None
    with pytest.raises(D.LsAmdError, match="mode-ordering signs"):
        D.SectorExpansion(basis, reps, [0, 1])
    # a spin plan has no fermionic block table
    sx = D.SectorExpansion(spin, sreps[0], [0, 1])
    assert Lc.ls_amd_fermi_expand_block(sx._plan(), 0, None, None, None, None, None) == -1 and sx.kernel == "k_expand_push"
    sx.destroy()
