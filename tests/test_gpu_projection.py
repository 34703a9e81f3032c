"""Projection of full-basis vectors into symmetry sectors on the GPU (SectorProjection / k_project_pull, k_project_pull_fermi, project,
product_state) against B+ Phi with the projector columns B of tests/entanglement_reference.py and
tests/fermion_entanglement_reference.py: every branch of the kernels entry by entry, adjointness and isometry against the shipped
expansion kernels, completeness over the sectors of a ring, blocks of columns in every layout, determinism, the symmetry resolution
of an eigenvector against the projected matvec kernels, a quench from the Neel state in its two momentum sectors, product_state
against the projection of a one-hot vector, and the failures that must be loud.

Tolerance (derived, not measured): a sum of |G| products and one scaling on both sides of the comparison, with 1 / n(r) <= sqrt|G|:
    |got - want| <= 2 (|G| + 4) 2^-53 sqrt|G| max|Phi|"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
import fermion_entanglement_reference as R
import fermion_symm as F
from distributed_matvec_amd import SectorProjection  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd.diagonalize import LocalOperator
from oracle import model as M
from test_correlations_host import _torus_spin_config

pytestmark = pytest.mark.gpu
NEEL = 0b010101010101


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def bound(order, scale):
    return 2.0 * (order + 4) * 2.0 ** -53 * math.sqrt(order) * scale


def _free_ring(L, k):
    return {"basis": {"number_spins": L, "symmetries": [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]}}


def random_phi(torch, F_, K, cplx, seed):
    """a seeded random block over the full basis: (numpy (F, K), the same on the device, interleaved)"""
    rs = np.random.RandomState(seed)
    a = rs.rand(F_, K) - 0.5
    if cplx:
        a = a + 1j * (rs.rand(F_, K) - 0.5)
    return a, torch.from_numpy(a).cuda()


class Spin:
    """a spin-1/2 sector: the library's basis and representatives, and the reference's B+ (dense)"""

    def __init__(self, cfg):
        self.cfg = cfg
        self.model, self.full, self.want_reps = E.tables(cfg)[:3]
        self.order = len(self.model.group.perms) * (2 if self.model.spin_inversion else 1)
        self.basis = D.loadConfigFromDict({"basis": cfg["basis"]})
        self.reps = D.enumerateStates(self.basis, 1)[0][0]
        assert np.array_equal(_u64(self.reps), self.want_reps)
        self.F, self.n = len(self.full), len(self.want_reps)
        self.kernel = "k_project_pull"

    @functools.cached_property
    def B(self):
        B = E.projector_columns(self.cfg)[1]
        B.setflags(write=False)
        return B

    def adjoint(self, phi):
        return np.conj(np.conj(phi).T @ self.B).T  # B+ Phi without a conjugated copy of B

    def unproject(self, psi):
        return D.unproject(self.basis, self.reps, psi)


class Fermi:
    """a fermionic sector (fermion_entanglement_reference.Case): B is sparse"""

    def __init__(self, case):
        self.case = case
        self.order = len(case.group)
        self.basis = D.loadConfigFromDict(case.config())
        self.reps = D.enumerateStates(self.basis, 1)[0][0]
        assert np.array_equal(_u64(self.reps), case.reps)
        self.full = case.states
        self.F, self.n = len(case.states), len(case.reps)
        self.kernel = "k_project_pull_fermi"

    def adjoint(self, phi):
        return self.case.columns.conj().T @ phi

    def unproject(self, psi):
        return D.fermion_unproject(self.basis, self.reps, psi)


# name: (sector, dtype of Phi)
SPIN = {
    "ring12_k0_inversion_plus_stabilisers_f64": (lambda: E.ring(12, 6, 0, inv=1), "f64"),
    "ring12_k3_complex_characters_c128": (lambda: E.ring(12, 6, 3), "c128"),
    "ring12_k3_promoted_f64": (lambda: E.ring(12, 6, 3), "f64"),
    "ring12_k6_reflection_inversion_minus_zero_norms": (lambda: E.ring(12, 6, 6, inv=-1, reflect=1), "f64"),
    "ring10_every_weight_k1": (lambda: _free_ring(10, 1), "c128"),
    "ring10_weight5_unprojected_identity": (lambda: E.ring(10, 5, None), "f64"),
    "ring16_k0_810_rows": (lambda: E.ring(16, 8, 0), "f64"),
    "ring36_weight3_k5_64_bit_words": (lambda: E.ring(36, 3, 5), "c128"),
    "torus_4x3": (_torus_spin_config, "f64"),
}
FERMI = {
    "ring8_k0_f64": (lambda: R.Case(8, 4, gens=F.translations(8), secs=[0]), "f64"),
    "ring8_k1_c128": (lambda: R.Case(8, 4, gens=F.translations(8), secs=[1]), "c128"),
    "ring10_dihedral_reflection_odd": (lambda: R.Case(10, 5, gens=F.dihedral(10), secs=[0, 1]), "f64"),
    "ring10_every_number_k1": (lambda: R.Case(10, None, gens=F.translations(10), secs=[1]), "c128"),
    "ring16_k0_more_than_256_rows": (lambda: R.Case(16, 8, gens=F.translations(16), secs=[0]), "f64"),
    "ring34_two_particles_k5": (lambda: R.Case(34, 2, gens=F.translations(34), secs=[5]), "c128"),
    "spinful6_unprojected": (lambda: R.Case(6, up=(3, 3)), "f64"),
    "spinful6_k0": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0]), "f64"),
    "spinful6_k2": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2]), "c128"),
    "spinful6_k0_flip_plus": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[0], flip=1), "f64"),
    "spinful6_k1_flip_minus": (lambda: R.Case(6, up=(3, 3), gens=F.translations(6), secs=[1], flip=-1), "c128"),
    "spinful17_one_up_one_down_k3": (lambda: R.Case(17, up=(1, 1), gens=F.translations(17), secs=[3]), "c128"),
}


@functools.lru_cache(maxsize=None)
def sector(name):
    """the sector of a case of the tables: built once, shared, read-only"""
    if name in SPIN:
        return Spin(SPIN[name][0]())
    return Fermi(FERMI[name][0]())


def _case_checks(name, s):
    if name == "ring12_k0_inversion_plus_stabilisers_f64":
        assert s.order == 24 and s.F == 924
    if name == "ring12_k6_reflection_inversion_minus_zero_norms":
        dead = int((~E.tables(s.cfg)[5]).sum())
        print(f"{name}: {dead} of {s.F} states lie on orbits of zero norm")
        assert s.order == 48 and dead > 100  # many orbits of zero norm
    if name == "ring16_k0_810_rows":
        assert s.n == 810 and s.F == 12870  # more than one 256-row tile
    if name == "ring36_weight3_k5_64_bit_words":
        assert int(s.full.max()) >> 32
    if name == "ring10_every_weight_k1":
        assert s.F == 1024
    if name == "torus_4x3":
        assert s.order == 12
    if name == "ring16_k0_more_than_256_rows":
        assert s.n > 256 and s.n % 256 != 0
    if name == "ring34_two_particles_k5":
        assert int(s.full.max()) >> 32
    if name == "spinful17_one_up_one_down_k3":
        assert s.F == 289 and s.case.M == 34
    if name.startswith("spinful6"):
        assert s.F == 400


@pytest.mark.parametrize("name", sorted(SPIN) + sorted(FERMI))
def test_project_matches_the_adjoint_of_the_projector_columns(torch, name):
    s = sector(name)
    _case_checks(name, s)
    cplx = (SPIN.get(name) or FERMI[name])[1] == "c128"
    phi_np, phi = random_phi(torch, s.F, 1, cplx, 7)
    pj = D.SectorProjection(s.basis, s.reps)
    assert pj.full_size == s.F
    got_t = pj.project(phi[:, 0])
    assert pj.kernel == s.kernel
    assert got_t.shape == (s.n,)
    assert got_t.dtype == (torch.complex128 if cplx or pj.complex_characters else torch.float64)
    if name == "ring12_k3_promoted_f64":
        assert got_t.dtype == torch.complex128 and phi.dtype == torch.float64
    got = got_t.cpu().numpy()
    want = s.adjoint(phi_np[:, 0])
    tol = bound(s.order, float(np.abs(phi_np).max()))
    worst = float(np.abs(got - want).max())
    print(f"project {name}: {s.F} states -> {s.n} rows, |G| = {s.order}, max error {worst:.2e}, bound {tol:.2e}, ratio {worst / tol:.3f}")
    assert np.isfinite(got).all() and worst <= tol, (name, worst, tol)
    if name == "ring10_weight5_unprojected_identity":
        assert np.array_equal(got, phi_np[:, 0])  # B = 1
    # the one-shot form is the same call
    assert torch.equal(D.project(s.basis, s.reps, phi[:, 0]), got_t)
    pj.destroy()


ADJOINT = ["ring12_k0_inversion_plus_stabilisers_f64", "ring12_k3_complex_characters_c128", "ring10_every_weight_k1",
           "ring8_k1_c128", "spinful6_k0_flip_plus", "ring10_dihedral_reflection_odd"]


@pytest.mark.parametrize("name", ADJOINT)
def test_adjoint_and_isometry_against_the_expansion_kernels(torch, name):
    s = sector(name)
    cplx = (SPIN.get(name) or FERMI[name])[1] == "c128"
    dtype = torch.complex128 if cplx else torch.float64
    phi_np, phi = random_phi(torch, s.F, 1, cplx, 21)
    phi = phi[:, 0].contiguous()
    psi = D.fillRandom(s.reps, 5, dtype)
    max_phi, max_psi = float(np.abs(phi_np).max()), float(psi.abs().max())
    pj = D.SectorProjection(s.basis, s.reps)
    # <project(Phi), psi> = <Phi, unproject(psi)>
    lhs = complex(torch.vdot(pj.project(phi).to(torch.complex128), psi.to(torch.complex128)))
    rhs = complex(torch.vdot(phi.to(torch.complex128), s.unproject(psi).to(torch.complex128)))
    tol = bound(s.order, max_phi) * math.sqrt(s.F) * max_psi
    print(f"adjoint {name}: |lhs - rhs| = {abs(lhs - rhs):.2e}, tolerance {tol:.2e}")
    assert abs(lhs - rhs) <= tol
    # project(unproject(psi)) = psi
    back = pj.project(s.unproject(psi))
    tol = bound(s.order, max_psi) * math.sqrt(s.F) * max_psi
    dev = float((back - psi).abs().max())
    print(f"isometry {name}: max |B+ B psi - psi| = {dev:.2e}, tolerance {tol:.2e}")
    assert dev <= tol
    # unproject(project(.)) is idempotent
    once = s.unproject(pj.project(phi))
    twice = s.unproject(pj.project(once))
    tol = bound(s.order, max_phi) * math.sqrt(s.F) * max_phi
    dev = float((twice - once).abs().max())
    print(f"projector {name}: max |P P Phi - P Phi| = {dev:.2e}, tolerance {tol:.2e}")
    assert dev <= tol and float(once.abs().max()) > 1e-3
    pj.destroy()


def test_the_sectors_of_the_ring_are_complete(torch):
    phi_np, phi = random_phi(torch, 924, 1, True, 3)
    total, dims = 0.0, 0
    for k in range(12):
        for inv in (1, -1):
            basis = D.loadConfigFromDict(E.ring(12, 6, k, inv=inv))
            reps = D.enumerateStates(basis, 1)[0][0]
            dims += reps.numel()
            if reps.numel():
                total += float(torch.linalg.vector_norm(D.project(basis, reps, phi[:, 0])) ** 2)
    norm2 = float(np.linalg.norm(phi_np) ** 2)
    print(f"completeness: sum of the sector weights / |Phi|^2 - 1 = {total / norm2 - 1.0:.2e}")
    assert dims == 924  # an abelian group: the sector dimensions add up to the full basis
    assert abs(total - norm2) <= 1e-12 * norm2


@pytest.mark.parametrize("name", ["ring12_k3_complex_characters_c128", "spinful6_k0_flip_plus", "ring16_k0_810_rows"])
@pytest.mark.parametrize("K", [3, 8, 11])
def test_blocks_of_columns_in_every_layout(torch, name, K):
    s = sector(name)
    cplx = (SPIN.get(name) or FERMI[name])[1] == "c128"
    phi_np, phi = random_phi(torch, s.F, K, cplx, 100 + K)
    tol = bound(s.order, float(np.abs(phi_np).max()))
    pj = D.SectorProjection(s.basis, s.reps)
    single = torch.stack([pj.project(phi[:, c].contiguous()) for c in range(K)], dim=1)
    transposed = phi.T.contiguous().T  # column-major
    wide = torch.zeros(s.F, 2 * K + 1, dtype=phi.dtype, device=phi.device)
    wide[:, 1::2] = phi
    layouts = {"interleaved": phi, "transposed": transposed, "strided view": wide[:, 1::2]}
    assert transposed.stride() == (1, s.F) and layouts["strided view"].stride() == (2 * K + 1, 2)
    for what, block in layouts.items():
        got = pj.project(block)
        assert got.shape == (s.n, K) and got.is_contiguous()
        dev = float((got - single).abs().max())
        print(f"block {name} K = {K} {what}: max deviation from the columns one by one {dev:.2e}, bound {tol:.2e}")
        assert dev <= tol, (name, K, what)
    # out= with strides is honoured, and nothing outside it is touched
    sentinel = 12345.0
    big = torch.full((s.n + 2, 2 * K), sentinel, dtype=single.dtype, device=phi.device)
    out = big[1:-1, 1::2]
    ret = pj.project(phi, out=out)
    assert ret.data_ptr() == out.data_ptr() and float((out - single).abs().max()) <= tol
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[1:-1, 1::2] = False
    assert bool((big[keep] == sentinel).all())
    colmajor = torch.empty(K, s.n, dtype=single.dtype, device=phi.device).T
    assert float((pj.project(phi, out=colmajor) - single).abs().max()) <= tol
    pj.destroy()


def test_out_must_fit_exactly(torch):
    s = sector("ring12_k3_complex_characters_c128")
    _, phi = random_phi(torch, s.F, 3, True, 1)
    pj = D.SectorProjection(s.basis, s.reps)
    for bad in (torch.empty(s.n, 4, dtype=torch.complex128, device="cuda"), torch.empty(s.n, 3, dtype=torch.float64, device="cuda"),
                torch.empty(s.n, dtype=torch.complex128, device="cuda"), torch.empty(s.n, 3, dtype=torch.complex128),
                torch.empty(s.n, 1, dtype=torch.complex128, device="cuda").expand(s.n, 3)):
        with pytest.raises(D.LsAmdError, match="out must be"):
            pj.project(phi, out=bad)
    pj.destroy()


@pytest.mark.parametrize("K", [1, 8])
def test_two_calls_return_the_same_bytes(torch, K):
    for name in ("ring16_k0_810_rows", "spinful6_k1_flip_minus"):
        s = sector(name)
        cplx = (SPIN.get(name) or FERMI[name])[1] == "c128"
        _, phi = random_phi(torch, s.F, K, cplx, 9)
        block = phi[:, 0].contiguous() if K == 1 else phi
        pj = D.SectorProjection(s.basis, s.reps)
        a, b = pj.project(block), pj.project(block)
        assert a.data_ptr() != b.data_ptr()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
        pj.destroy()


@functools.lru_cache(maxsize=None)
def heisenberg_ring_12():
    """(config, states, dense H, eigenvalues, eigenvectors) of the 12-site Heisenberg ring at weight 6 without symmetries"""
    cfg = M.heisenberg_chain_config(12)
    states, H = M.dense_sector_matrix(cfg)
    H = np.asarray(H)
    assert np.abs(H.imag).max() == 0.0 and len(states) == 924
    H = np.ascontiguousarray(H.real)
    w, v = np.linalg.eigh(H)
    for a in (H, w, v):
        a.setflags(write=False)
    return cfg, np.asarray(states, dtype=np.uint64), H, w, v


def _sector_of_the_ring(k, inv):
    cfg = {"basis": E.ring(12, 6, k, inv=inv)["basis"], "hamiltonian": heisenberg_ring_12()[0]["hamiltonian"]}
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    return basis, h, reps


def test_symmetry_resolution_of_an_eigenvector(torch):
    _, states, _, w, v = heisenberg_ring_12()
    assert w[1] - w[0] > 1e-6  # the ground state is not degenerate
    e0 = float(w[0])
    phi = torch.from_numpy(np.ascontiguousarray(v[:, 0])).cuda()
    plain = D.loadConfigFromDict({"basis": E.ring(12, 6, None)["basis"]})
    assert np.array_equal(_u64(D.enumerateStates(plain, 1)[0][0]), states)  # the order project reads Phi in
    weights, home = {}, None
    for k in range(12):
        for inv in (1, -1):
            basis, h, reps = _sector_of_the_ring(k, inv)
            psi = D.project(basis, reps[0], phi)
            weights[k, inv] = float(torch.linalg.vector_norm(psi) ** 2)
            if abs(weights[k, inv] - 1.0) <= 1e-12:
                assert home is None
                home = (k, inv)
                # in its sector the projected state is the eigenvector of the sector Hamiltonian: the projected matvec kernels
                plan = D.MatvecPlan(h, reps, psi.dtype)
                y = torch.zeros_like(psi)
                plan.matvec([psi], [y])
                res = float(torch.linalg.vector_norm(y - e0 * psi))
                print(f"ground state: sector (k = {k}, inv = {inv:+d}), |H psi - E0 psi| = {res:.2e} ({plan.kernel})")
                assert res <= 1e-11
                plan.destroy()
    print("weights:", {key: f"{val:.1e}" for key, val in weights.items() if val > 1e-20})
    assert home is not None
    assert all(val <= 1e-12 for key, val in weights.items() if key != home)


def test_quench_from_the_neel_state_in_its_momentum_sectors(torch):
    _, states, _, w, v = heisenberg_ring_12()
    t = 1.0
    row = v[int(np.searchsorted(states, np.uint64(NEEL)))]
    want = complex(np.sum(np.abs(row) ** 2 * np.exp(-1j * w * t)))  # <N|e^{-iHt}|N>
    width = float(w[-1] - w[0])
    bounds = (float(w[0]) - 0.01 * width, float(w[-1]) + 0.01 * width)  # the sectors' spectra lie inside the full one
    got, total = 0j, 0.0
    for k, inv in ((0, 1), (6, -1)):
        basis, h, reps = _sector_of_the_ring(k, inv)
        psi, weight = D.product_state(basis, reps[0], NEEL)
        assert psi.dtype == torch.float64 and psi.device.type == "cuda" and abs(weight - 0.5) <= 1e-14
        op = LocalOperator(h, reps, torch.float64)
        out = D.propagate(op, psi, t, bounds=bounds, eps=1e-12)
        got += weight * complex(torch.vdot(psi.to(torch.complex128), out))
        total += weight
    print(f"quench: sum_s w_s <phi_s|e^(-i H_s t)|phi_s> = {got:.12f}, dense {want:.12f}, difference {abs(got - want):.2e}")
    assert abs(total - 1.0) <= 1e-14
    assert abs(got - want) <= 1e-10
    assert 0.01 < abs(want) < 0.99  # the state has moved: the comparison is not of constants


@pytest.mark.parametrize("name", ["ring12_k6_reflection_inversion_minus_zero_norms", "ring12_k3_complex_characters_c128", "ring8_k1_c128",
                                  "ring10_dihedral_reflection_odd", "spinful6_k1_flip_minus", "spinful6_k0_flip_plus"])
def test_product_state_is_the_projection_of_a_one_hot_vector(torch, name):
    s = sector(name)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    pj = D.SectorProjection(s.basis, s.reps)
    tol = bound(s.order, 1.0)
    live = 0
    for state in s.full[:: max(1, s.F // 25)]:
        at = int(L.ls_amd_test_project_state_index(s.basis.payload, C.c_uint64(int(state))))
        assert s.full[at] == state
        phi = torch.zeros(s.F, dtype=torch.complex128, device="cuda")
        phi[at] = 1.0
        want = pj.project(phi)
        n2 = float(torch.linalg.vector_norm(want) ** 2)
        if n2 <= 1e-20:
            with pytest.raises(D.LsAmdError, match="zero weight"):
                D.product_state(s.basis, s.reps, int(state))
            continue
        live += 1
        psi, weight = D.product_state(s.basis, s.reps, int(state), dtype=torch.complex128)
        assert abs(weight - n2) <= 4 * tol
        assert float((psi * math.sqrt(weight) - want).abs().max()) <= tol, (name, hex(int(state)))
    assert live >= 5
    pj.destroy()


def test_errors_are_flags_and_messages(torch):
    from distributed_matvec_amd import _lib

    L = _lib.load()
    s = sector("ring12_k3_complex_characters_c128")
    # representatives of another weight: the flag, zero rows, no fault
    wrong = torch.from_numpy(np.array([0b11111, 0b101111, 0b1011101], dtype=np.int64)).cuda()
    pj = D.SectorProjection(s.basis, wrong)
    _, phi = random_phi(torch, s.F, 8, True, 2)
    with pytest.raises(D.LsAmdError, match="not in the basis"):
        pj.project(phi[:, 0].contiguous())
    out = pj.project(phi, check=False)
    with pytest.raises(D.LsAmdError, match="not in the basis"):
        pj.check()
    pj.check()  # the flag is cleared once reported
    assert float(out.abs().max()) == 0.0
    pj.destroy()
    # f64 with complex characters is refused at the C level; so is a K outside [1, 64]
    pj = D.SectorProjection(s.basis, s.reps)
    real = torch.zeros(s.F, dtype=torch.float64, device="cuda")
    out = torch.zeros(s.n, 65, dtype=torch.complex128, device="cuda")
    assert L.ls_amd_project_apply(pj._plan(), 0, 1, C.c_void_p(real.data_ptr()), 1, 0, C.c_void_p(out.data_ptr()), 65, 1, None) == -1
    assert "f64 needs +-1 characters" in L.ls_amd_last_error().decode()
    for K in (0, 65):
        assert L.ls_amd_project_apply(pj._plan(), 1, K, C.c_void_p(phi.data_ptr()), 8, 1, C.c_void_p(out.data_ptr()), 65, 1, None) == -1
        assert "outside [1, 64]" in L.ls_amd_last_error().decode()
    assert L.ls_amd_project_apply(pj._plan(), 7, 1, C.c_void_p(phi.data_ptr()), 8, 1, C.c_void_p(out.data_ptr()), 65, 1, None) == -1
    assert L.ls_amd_project_full_size(pj._plan()) == 924
    assert pj.kernel == "k_project_pull"
    pj.destroy()
    f = sector("spinful6_k1_flip_minus")
    fp = D.SectorProjection(f.basis, f.reps)
    assert fp.kernel == "k_project_pull_fermi"
    # a word with another number of up particles among the representatives of the product basis
    fp.destroy()
    bad = f.reps.clone()
    bad[0] = 0b000011_001111
    fp = D.SectorProjection(f.basis, bad)
    with pytest.raises(D.LsAmdError, match="not in the basis"):
        fp.project(torch.zeros(f.F, dtype=torch.complex128, device="cuda"))
    fp.destroy()
