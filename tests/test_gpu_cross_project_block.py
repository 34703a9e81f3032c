"""The block form of the projecting cross-sector kernel on the GPU: CrossSectorPlan.apply_block(method="kernel") on groups="project"
plans (k_cross_project_blk, k_cross_project_blk_fermi) against the dense B2^+ A B1 of tests/cross_groups_reference.py and
tests/fermion_cross_reference.py (nothing of this library), for partial, full and several chunks of columns, in every layout, with
several tiles per workgroup, with 64-bit words against the single-vector kernel; the knob (method=, LS_AMD_CROSS_PROJECT_BLOCK), the
error flag, and evolve.thermal_correlation(groups="project", block_method=...) against eigendecompositions of the dense sectors.

No tolerance of its own.  A (row, column) of Y is the row of tests/test_gpu_cross_groups.py applied to one column: the bound is
cross_groups_reference.compare with S = monomials x |G2| and the row scale that _against_dense / _fermi_case derive there, taken
column by column with that column's max|x|.  The thermal test uses the derived bound of tests/test_gpu_cross_block.py,
|N_k(t) - exact| <= 1e-10 ||A||_2^2 Z_k and |Z_k - exact| <= 1e-11 Z_k (at most 2 T + 1 = 9 propagate calls, T = 4 times, enter a
value).  Every comparison prints its worst error / tolerance."""
import numpy as np
import pytest

import cross_groups_reference as G
import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_symm as F
from distributed_matvec_amd import config
from distributed_matvec_amd.evolve import thermal_correlation

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 9, 64)  # a partial chunk, a full chunk, a chunk and a tail, the maximum
KERNEL, KERNEL_FERMI = "k_cross_project_blk", "k_cross_project_blk_fermi"


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _dtype(torch, name):
    return torch.complex128 if name == "c128" else torch.float64


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _setup(src_cfg, dst_cfg, op_cfg):
    """(Operator on the source basis, source reps, target Basis, target reps): device tensors of the representatives"""
    sbasis = D.loadConfigFromDict(src_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    tbasis = D.loadConfigFromDict(dst_cfg)
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    return A, sreps[0], tbasis, treps[0]


def _random_block(torch, n, K, dtype, seed):
    """(n, K) interleaved (strides (K, 1)), entries uniform in [-1, 1) (+ i [-1, 1))"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.0, 1.0, (n, K))
    if dtype == torch.complex128:
        a = a + 1j * rng.uniform(-1.0, 1.0, (n, K))
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _nan_block(torch, n, K, dtype):
    return torch.full((n, K), float("nan"), dtype=dtype, device="cuda")


def _scale(unit, x):
    """per (row, column): unit = the row's bound on its sum of |coefficient| (array or number), times the column's max|x|"""
    return np.reshape(np.asarray(unit, dtype=float), (-1, 1)) * x.abs().amax(dim=0).cpu().numpy()[None, :]


def _check_blocks(torch, plan, mat, S, unit, dtype, what, Ks=KS, real=False, seed=7):
    """apply_block(method="kernel") on interleaved blocks of every K in Ks against mat @ X, Y pre-filled with NaN"""
    n_dst, n_src = mat.shape
    xs = _random_block(torch, n_src, max(Ks), dtype, seed)
    for K in Ks:
        x = xs[:, :K].contiguous()
        y = _nan_block(torch, n_dst, K, dtype)
        plan.apply_block(x, y, method="kernel")
        want = mat @ x.cpu().numpy()
        if real:
            want = want.real
        G.compare(y.cpu().numpy(), want, S, _scale(unit, x), f"project block {what} K = {K}")


def _spin_case(torch, src, dst, op, dt):
    """(plan, reference, S, unit) of one spin pair; the representatives and the names of both paths are checked"""
    ref = G.dense(src, dst, op)
    A, sreps, tbasis, treps = _setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3  # nothing passes vacuously
    if dt == "f64":
        assert np.abs(ref["matrix"].imag).max() <= 1e-14
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, _dtype(torch, dt), groups="project")
    for K in KS:
        assert plan.block_kernel(K, "kernel") == KERNEL
        assert plan.block_kernel(K) == "columns" and plan.block_kernel(K, "columns") == "columns"
    S = G.monomials(op) * G.group_order(dst)
    return plan, ref, S, G.row_scale(X.coefficient_sum(op), ref["n2"], 1.0)


FREE12 = G.ring(12, None, 0, 0, 1)
DIHEDRAL12 = G.ring(12, 6, 0, 0, 1)
HOP = (DIHEDRAL12, G.ring(12, 6, 2), G.hop_q_plus_sz0(12, 1))


# ---- 1: a local operator, two tiles and a seam -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 5])
def test_local_sz_at_free_weight(torch, k):
    """12-site ring without a fixed weight, sigma^z_0 from (k = 0, refl, inv) into k: ~350 target rows, two tiles and a seam"""
    plan, ref, S, unit = _spin_case(torch, FREE12, G.ring(12, None, k), G.sz_site(0), "c128")
    assert 256 < len(ref["dst"]) < 512 and ref["leak"] > 0.1
    _check_blocks(torch, plan, ref["matrix"], S, unit, torch.complex128, f"sigma^z_0 k = {k}")
    plan.destroy()


# ---- 2: four passes, complex terms and characters ------------------------------------------------------------------------------------
def test_many_flip_groups_and_complex_coefficients(torch):
    """sum_j e^{-iqj} sigma^+_j sigma^-_{j+1} + sigma^z_0 on 12 sites: 13 groups (4 per pass); against the dense matrix and, column by
    column, against plan.apply under the same bound"""
    src, dst, op = HOP
    plan, ref, S, unit = _spin_case(torch, src, dst, op, "c128")
    c128 = torch.complex128
    _check_blocks(torch, plan, ref["matrix"], S, unit, c128, "13 groups")
    K = 9
    x = _random_block(torch, len(ref["src"]), K, c128, 13)
    y = _nan_block(torch, len(ref["dst"]), K, c128)
    plan.apply_block(x, y, method="kernel")
    single = _nan_block(torch, len(ref["dst"]), K, c128)
    for k in range(K):
        yk = torch.full((len(ref["dst"]),), float("nan"), dtype=c128, device="cuda")
        plan.apply(x[:, k].contiguous(), yk)
        single[:, k] = yk
    assert float(single.abs().max()) > 1e-3
    G.compare(y.cpu().numpy(), single.cpu().numpy(), S, _scale(unit, x), "13 groups, kernel vs apply per column")
    plan.destroy()


# ---- 3: the inversion image and the real-coefficient kinds -----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f64", "c128"])
@pytest.mark.parametrize("inv", [1, -1])
def test_the_identity_upwards(torch, dt, inv):
    """A = 1 from translations-only k = 0 into the dihedral (0, 0) sector with inversion +-1: n_img = 2, a real coefficient"""
    plan, ref, S, unit = _spin_case(torch, G.ring(12, 6, 0), G.ring(12, 6, 0, 0, inv), G.identity(12), dt)
    assert len(ref["dst"]) < len(ref["src"])
    _check_blocks(torch, plan, ref["matrix"], S, unit, _dtype(torch, dt), f"identity upwards inv {inv} {dt}", real=dt == "f64")
    plan.destroy()


# ---- 4: fermions ----------------------------------------------------------------------------------------------------------------------
def _fermi_case(torch, src, dst, model, dt, what):
    spinful = src["n_up"] is not None
    ref = R.reference(src, dst, model)
    A, sreps, tbasis, treps = _setup(R.basis_config(src), R.basis_config(dst), R.operator_section(model, spinful))
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3
    if dt == "f64":
        assert np.abs(ref["matrix"].imag).max() <= 1e-14
    dtype = _dtype(torch, dt)
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype, groups="project")
    for K in KS:
        assert plan.block_kernel(K, "kernel") == KERNEL_FERMI and plan.block_kernel(K) == "columns"
    if spinful:
        import fermion_spinful_symm as FS

        order = len(FS.group(dst["L"], dst["gens"], dst["secs"], dst["flip"]))
    else:
        order = len(F.closure(dst["L"], dst["gens"], dst["secs"]))
    # n2(r') >= |G2|^-1/2: the row's sum of |coefficient| is at most sum |c_j| sqrt(|G2|)
    _check_blocks(torch, plan, ref["matrix"], len(model) * order, R.coefficient_sum(model) * np.sqrt(order), dtype, what, real=dt == "f64", seed=5)
    plan.destroy()
    return ref


FD10 = R.sector(10, 4, F.dihedral(10), [0, 0])


def test_fermions_local_c_dagger(torch):
    ref = _fermi_case(torch, FD10, R.sector(10, 5, F.translations(10), [3]), [(1.0, [("+", 0, 0)])], "c128", "c+_0 into k = 3")
    assert ref["leak"] > 0.1 * ref["norm"]


@pytest.mark.parametrize("dt", ["f64", "c128"])
def test_fermions_into_a_dihedral_target_drop_zero_norm_orbits(torch, dt):
    """translations-only k = 5 (characters +-1) -> dihedral (0, 0), sum_j w_j c+_j with uneven weights: images of the adjoint whose
    orbit has no norm in the source sector must contribute nothing"""
    src, dst = R.sector(10, 4, F.translations(10), [5]), R.sector(10, 5, F.dihedral(10), [0, 0])
    model = [(1.0 + 0.25 * j, [("+", j, 0)]) for j in range(10)]
    ref = _fermi_case(torch, src, dst, model, dt, f"dihedral target {dt}")
    assert ref["pull_dropped"] > 0


def test_spinful_fermions_with_spin_flip_on_the_source_only(torch):
    src = R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1)
    dst = R.sector(4, 4, F.translations(4), [1], n_up=2)
    _fermi_case(torch, src, dst, [(1.0, [("n", 0, 0)]), (0.5, [("+", 0, 0), ("-", 1, 0)])], "c128", "spinful, flip on the source")


# ---- 5: 64-bit words ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 9])
def test_64_bit_words_against_the_single_vector_kernel(torch, K):
    """34-site ring at weight 2 (561 states): dihedral (0, 0) -> (k = 5), a local bond plus sigma^z_0, column by column against
    plan.apply under the bound of test_64_bit_words_against_the_library_composition"""
    L = 34
    src, dst = G.ring(L, 2, 0, 0), G.ring(L, 2, 5)
    op = {"terms": [{"expression": "σᶻ₀", "sites": [[0]]}, {"expression": "σ⁺₀ σ⁻₁", "sites": [[0, 1], [1, 0]]}]}
    A, sreps, tbasis, treps = _setup(src, dst, op)
    assert (sreps.numel(), treps.numel()) == (17, 16)
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128, groups="project")
    assert plan.block_kernel(K, "kernel") == KERNEL
    x = _random_block(torch, 17, K, c128, 3)
    y = _nan_block(torch, 16, K, c128)
    plan.apply_block(x, y, method="kernel")
    want = _nan_block(torch, 16, K, c128)
    for k in range(K):
        yk = torch.full((16,), float("nan"), dtype=c128, device="cuda")
        plan.apply(x[:, k].contiguous(), yk)
        want[:, k] = yk
    assert float(want.abs().max()) > 1e-3
    # n2(r') >= |G2|^-1/2: the row's sum of |coefficient| is at most sum |c_j| sqrt(|G2|)
    G.compare(y.cpu().numpy(), want.cpu().numpy(), G.monomials(op) * L, _scale(X.coefficient_sum(op) * np.sqrt(L), x), f"34 sites K = {K}")
    plan.destroy()


# ---- 6: layouts -----------------------------------------------------------------------------------------------------------------------
def test_block_layouts(torch):
    """column-major X and Y (transposed (K, n) tensors), a row stride padded beyond K (the padding must survive in Y), and an
    interleaved X with a column-major Y"""
    src, dst, op = HOP
    plan, ref, S, unit = _spin_case(torch, src, dst, op, "c128")
    c128, K = torch.complex128, 9
    n_dst, n_src = ref["matrix"].shape
    x = _random_block(torch, n_src, K, c128, 11)
    want = ref["matrix"] @ x.cpu().numpy()
    scale = _scale(unit, x)
    # column-major
    xc = x.t().contiguous().t()
    yc = torch.full((K, n_dst), float("nan"), dtype=c128, device="cuda").t()
    assert xc.stride() == (1, n_src) and yc.stride() == (1, n_dst)
    plan.apply_block(xc, yc, method="kernel")
    G.compare(yc.cpu().numpy(), want, S, scale, "layout column-major")
    # rows padded to K + 3
    sentinel = -7.25
    wide_x = torch.full((n_src, K + 3), sentinel, dtype=c128, device="cuda")
    wide_y = torch.full((n_dst, K + 3), sentinel, dtype=c128, device="cuda")
    wide_x[:, :K] = x
    wide_y[:, :K] = float("nan")
    assert wide_x[:, :K].stride() == (K + 3, 1)
    plan.apply_block(wide_x[:, :K], wide_y[:, :K], method="kernel")
    G.compare(wide_y[:, :K].cpu().numpy(), want, S, scale, "layout padded rows")
    assert bool((wide_y[:, K:] == sentinel).all()) and bool((wide_x[:, K:] == sentinel).all())
    # interleaved in, column-major out
    yc = torch.full((K, n_dst), float("nan"), dtype=c128, device="cuda").t()
    plan.apply_block(x, yc, method="kernel")
    G.compare(yc.cpu().numpy(), want, S, scale, "layout interleaved X, column-major Y")
    plan.destroy()


# ---- 7: several tiles per workgroup ------------------------------------------------------------------------------------------------
def test_one_workgroup_walks_both_tiles(torch, monkeypatch):
    """LS_AMD_CROSS_BLOCKS=1: one row block per chunk of columns walks both tiles, so the register accumulators must be cleared at
    the head of the second"""
    monkeypatch.setenv("LS_AMD_CROSS_BLOCKS", "1")
    plan, ref, S, unit = _spin_case(torch, FREE12, G.ring(12, None, 5), G.sz_site(0), "c128")
    assert len(ref["dst"]) > 256
    _check_blocks(torch, plan, ref["matrix"], S, unit, torch.complex128, "one workgroup", Ks=(3, 9))
    plan.destroy()


# ---- 8: equal bytes, and who decides the path ---------------------------------------------------------------------------------------
def test_equal_bytes_and_the_knob(torch, monkeypatch):
    src, dst, op = HOP
    monkeypatch.delenv("LS_AMD_CROSS_PROJECT_BLOCK", raising=False)
    plan, ref, S, unit = _spin_case(torch, src, dst, op, "c128")
    c128, K = torch.complex128, 9
    n_dst, n_src = ref["matrix"].shape
    x = _random_block(torch, n_src, K, c128, 17)
    f64 = torch.float64

    def run(method):
        y = _nan_block(torch, n_dst, K, c128)
        plan.apply_block(x, y, method=method)
        return y

    y1, y2 = run("kernel"), run("kernel")
    assert float(y1.abs().max()) > 1e-3 and torch.equal(y1.view(f64), y2.view(f64))
    single = _nan_block(torch, n_dst, K, c128)
    for k in range(K):
        yk = torch.full((n_dst,), float("nan"), dtype=c128, device="cuda")
        plan.apply(x[:, k].contiguous(), yk)
        single[:, k] = yk
    assert torch.equal(run(None).view(f64), single.view(f64))  # unset: the column loop, byte for byte the K applies
    monkeypatch.setenv("LS_AMD_CROSS_PROJECT_BLOCK", "kernel")
    assert plan.block_kernel(K) == KERNEL and plan.block_kernel(K, "columns") == "columns"
    assert torch.equal(run(None).view(f64), y1.view(f64))  # the environment chooses the kernel ...
    assert torch.equal(run("columns").view(f64), single.view(f64))  # ... and the argument wins over it
    monkeypatch.setenv("LS_AMD_CROSS_PROJECT_BLOCK", "columns")
    assert plan.block_kernel(K) == "columns" and plan.block_kernel(K, "kernel") == KERNEL
    assert torch.equal(run("kernel").view(f64), y1.view(f64))
    monkeypatch.setenv("LS_AMD_CROSS_PROJECT_BLOCK", "rows")
    with pytest.raises(D.LsAmdError, match="LS_AMD_CROSS_PROJECT_BLOCK=rows"):
        run(None)
    with pytest.raises(ValueError, match="'columns', 'kernel'"):
        run("rows")
    monkeypatch.delenv("LS_AMD_CROSS_PROJECT_BLOCK")
    # the other plans have one block kernel whatever the method says
    A, sreps, tbasis, treps = _setup(DIHEDRAL12, G.ring(12, 6, 5), X.sz_q(12, 5))
    restrict = D.CrossSectorPlan(A, sreps, tbasis, treps, c128, groups="restrict")
    assert restrict.block_kernel(K, "kernel") == restrict.block_kernel(K, "columns") == restrict.block_kernel(K) == "k_cross_pull_blk"
    restrict.destroy()
    plan.destroy()


# ---- 9: the error flag ----------------------------------------------------------------------------------------------------------------
def test_an_image_outside_the_source_basis_raises_from_check(torch):
    """sigma^+_0 between two bases of the SAME weight: nothing checks covariance here, the kernel's flag does"""
    src, dst = G.ring(12, 6, 0, 0, 1), G.ring(12, 6, 3)
    A, sreps, tbasis, treps = _setup(src, dst, {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}]})
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128, groups="project")
    x = _random_block(torch, sreps.numel(), 3, c128, 1)
    y = torch.zeros((treps.numel(), 3), dtype=c128, device="cuda")
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.apply_block(x, y, method="kernel")
    plan.check()  # reported once
    plan.destroy()


# ---- 10: thermal_correlation ------------------------------------------------------------------------------------------------------
TIMES = [0.0, 0.5, 1.0, 2.5]
BETAS = [0.0, 0.7]


def _heisenberg_section(L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"name": "Heisenberg", "terms": [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds},
                                            {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}


def _sector_hamiltonian(basis_cfg, L):
    """(reps, B^+ H B) from the isometry and the full matrix of tests/cross_sector_reference.py"""
    reps, B = X.isometry(basis_cfg)
    H = X.full_matrix(basis_cfg, _heisenberg_section(L))
    H = np.asarray(H.todense() if hasattr(H, "todense") else H)
    Hs = B.conj().T @ H @ B
    assert np.abs(Hs - Hs.conj().T).max() <= 1e-12
    return reps, 0.5 * (Hs + Hs.conj().T)


def test_thermal_correlation_of_a_local_operator(torch, monkeypatch):
    """8-site ring at weight 4, sigma^z_0 from k = 0 into k = 3, the identity block as vectors: N_k(t) and Z_k of every basis vector
    and the sector's exact C(t) against the eigendecompositions of the dense sector Hamiltonians and the dense B2^+ A B1 (numpy
    only), on the kernel path and once more on the column loop under the same bound"""
    L = 8
    src, dst, op = X.ring(L, 4, 0), X.ring(L, 4, 3), G.sz_site(0)
    ref = G.dense(src, dst, op)
    r1, Hs = _sector_hamiltonian(src, L)
    r2, Ht = _sector_hamiltonian(dst, L)
    assert np.array_equal(r1, ref["src"]) and np.array_equal(r2, ref["dst"]) and ref["leak"] > 0.1
    Es, Us = np.linalg.eigh(Hs)
    Et, Ut = np.linalg.eigh(Ht)
    lo, hi = min(Es[0], Et[0]), max(Es[-1], Et[-1])
    bounds = (float(lo - 0.01 * (hi - lo)), float(hi + 0.01 * (hi - lo)))
    Amat = ref["matrix"]
    norm = float(np.linalg.norm(Amat, 2))
    assert norm > 0.1
    n = len(Es)
    cfg = {"basis": src["basis"], "hamiltonian": _heisenberg_section(L), "observables": [op]}
    eye = torch.eye(n, dtype=torch.complex128, device="cuda")
    for beta in BETAS:
        e_ref = bounds[0]
        b = Us @ (np.exp(-0.5 * beta * (Es - e_ref))[:, None] * Us.conj().T)
        Z = (np.abs(b) ** 2).sum(axis=0)
        phi = Amat @ b
        N = np.empty((len(TIMES), n), dtype=complex)
        for j, t in enumerate(TIMES):
            bt = Us @ (np.exp(-1j * Es * t)[:, None] * (Us.conj().T @ b))
            pt = Ut @ (np.exp(-1j * Et * t)[:, None] * (Ut.conj().T @ phi))
            N[j] = ((Amat @ bt).conj() * pt).sum(axis=0)
        assert Z.min() > 1e-6 and np.abs(N).max() > 1e-6
        exact = N.sum(axis=1) / Z.sum()
        assert abs(exact[0]) > 1e-3 and abs(exact[0].imag) <= 1e-13 * abs(exact[0])  # C(0) = <A^+ A> is real and positive
        for method, name in (("kernel", KERNEL), ("columns", "columns")):
            res = thermal_correlation(cfg, 0, beta, TIMES, vectors=eye, target=dst, groups="project", bounds=bounds, block_method=method)
            assert res.kernel == name and res.dimension == n and res.reference_energy == e_ref
            rn = float((np.abs(res.numerator - N) / (1e-10 * norm ** 2 * Z[None, :])).max())
            rz = float((np.abs(res.partition - Z) / (1e-11 * Z)).max())
            rc = float((np.abs(res.correlation - exact) / (1e-10 * norm ** 2)).max())
            print(f"thermal_correlation project {method} beta = {beta}: orders {res.orders.tolist()}, numerator error / bound {rn:.3g}, "
                  f"partition error / bound {rz:.3g}, C(t) error / bound {rc:.3g}")
            assert rn <= 1.0 and rz <= 1.0 and rc <= 1.0, (method, beta, rn, rz, rc)
    # who decides when block_method is None: the environment where it is set, else the driver's measured default
    run = dict(vectors=eye, target=dst, groups="project", bounds=bounds)
    monkeypatch.delenv("LS_AMD_CROSS_PROJECT_BLOCK", raising=False)
    assert thermal_correlation(cfg, 0, 0.0, [0.0], **run).kernel == KERNEL
    monkeypatch.setenv("LS_AMD_CROSS_PROJECT_BLOCK", "columns")
    assert thermal_correlation(cfg, 0, 0.0, [0.0], **run).kernel == "columns"
    assert thermal_correlation(cfg, 0, 0.0, [0.0], block_method="kernel", **run).kernel == KERNEL
