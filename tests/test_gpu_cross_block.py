"""Cross-sector operators on blocks of vectors and finite-temperature correlations on the GPU: CrossSectorPlan.apply_block
(k_cross_pull_blk, k_cross_pull_blk_fermi) against the reference matrices of tests/cross_sector_reference.py,
tests/fermion_cross_reference.py and tests/cross_groups_reference.py (nothing of this library) for partial, full and several chunks
of columns, in every layout, with several tiles per workgroup, on a medium size against the single-vector kernel, and the failures
that must be loud; evolve.thermal_correlation and evolve.combine_sectors against eigendecompositions of the dense sector matrices.

The bound of the thermal tests is derived, not measured: |N_k(t) - exact| <= 1e-10 ||A||_2^2 Z_k and |Z_k - exact| <= 1e-11 Z_k.
At most 2 T + 1 = 9 propagate calls enter a value, each good to eps = 1e-12 relative to the norm of its vector (propagate's
contract in real time; the cooling step shrinks its vector and is cut relative to the norm that comes out), bilinearly: <A b(t)|p(t)> with |b| = sqrt(Z_k), |p| <= ||A|| sqrt(Z_k) moves by at most ~9e-12 ||A||^2 Z_k, and the cross
apply adds ~1e-13 sum|c| on top.  Every test prints its worst error / bound."""
import numpy as np
import pytest

import cross_groups_reference as G
import cross_sector_reference as X
import distributed_matvec_amd as D
import fermion_cross_reference as R
import fermion_symm as F
from distributed_matvec_amd import config
from distributed_matvec_amd.api import CrossSectorPlan
from distributed_matvec_amd.evolve import combine_sectors, thermal_correlation

apply_block = CrossSectorPlan.apply_block  # the feature under test: without it nothing here can run

pytestmark = pytest.mark.gpu

KS = (1, 3, 8, 9, 64)  # a partial chunk, a full chunk, a chunk and a tail, the maximum


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
    """(source Basis, Operator on it, source reps, target Basis, target reps): device tensors of the representatives"""
    sbasis = D.loadConfigFromDict(src_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    tbasis = D.loadConfigFromDict(dst_cfg)
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    return sbasis, A, sreps[0], tbasis, treps[0]


def _fermi_setup(src, dst, model):
    return _setup(R.basis_config(src), R.basis_config(dst), R.operator_section(model, src["n_up"] is not None))


def _random_block(torch, n, K, dtype, seed):
    """(n, K) interleaved (strides (K, 1)), entries uniform in [-1, 1) (+ i [-1, 1))"""
    rng = np.random.RandomState(seed)
    a = rng.uniform(-1.0, 1.0, (n, K))
    if dtype == torch.complex128:
        a = a + 1j * rng.uniform(-1.0, 1.0, (n, K))
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _nan_block(torch, n, K, dtype):
    return torch.full((n, K), float("nan"), dtype=dtype, device="cuda")


def _spin_rule(got, want, scale, what):
    """_compare of tests/test_gpu_cross_sector.py, column by column: |got - want| <= max(1e-13 sum_j |c_j| max|x|, 1e-12 max(|got|, |want|))"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for k in range(want.shape[1]):
        g, w = got[:, k], want[:, k]
        tol = np.maximum(1e-13 * scale[k], 1e-12 * np.maximum(np.abs(g), np.abs(w)))
        err = np.abs(g - w)
        assert np.isfinite(g).all() and (err <= tol).all(), (what, k, float(err.max()), float(tol.min()))
        worst = max(worst, float((err / tol).max()))
    print(f"block cross-sector {what}: {want.shape[0]} rows x {want.shape[1]} columns, max |y| {np.abs(want).max():.3e}, worst error / tolerance {worst:.3g}")
    return worst


def _check_spin_like(torch, plan, mat, csum, dtype, what, Ks=KS, real=False):
    """apply_block on interleaved blocks of every K in Ks against mat @ X, Y pre-filled with NaN"""
    n_dst, n_src = mat.shape
    xs = _random_block(torch, n_src, max(Ks), dtype, 7)
    for K in Ks:
        x = xs[:, :K].contiguous()
        y = _nan_block(torch, n_dst, K, dtype)
        plan.apply_block(x, y)
        want = mat @ x.cpu().numpy()
        if real:
            want = want.real
        scale = csum * x.abs().amax(dim=0).cpu().numpy()
        _spin_rule(y.cpu().numpy(), want, scale, f"{what} K = {K}")


# ---- block apply against reference matrices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(X.ALL_CASES))
def test_block_apply_matches_the_reference_matrix(torch, name):
    src, dst, op, dt = X.ALL_CASES[name]
    ref = X.case_formula(name)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    mat = ref["matrix"]
    assert np.count_nonzero(np.abs(mat) > 1e-9) > 0  # nothing passes vacuously
    if dt == "f64":
        assert np.abs(mat.imag).max() <= 1e-14
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    for K in KS:
        assert plan.block_kernel(K) == "k_cross_pull_blk"
    _check_spin_like(torch, plan, mat, X.coefficient_sum(op), dtype, name, real=dt == "f64")
    plan.destroy()


FERMI_RUNS = [(name, dt) for name in sorted(R.CASES) for dt in R.CASES[name][4]]


@pytest.mark.parametrize("name,dt", FERMI_RUNS)
def test_block_apply_matches_the_signed_projectors(torch, name, dt):
    src, dst, model, _, _, _ = R.CASES[name]
    ref = R.case_reference(name)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _fermi_setup(src, dst, model)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    mat = ref["matrix"]
    assert np.count_nonzero(np.abs(mat) > 1e-9) > 0 and (mat.real < -1e-9).any() and (mat.real > 1e-9).any()
    if dt == "f64":
        assert np.abs(mat.imag).max() <= 1e-14
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    for K in KS:
        assert plan.block_kernel(K) == "k_cross_pull_blk_fermi"
    _check_spin_like(torch, plan, mat, R.coefficient_sum(model), dtype, f"{name} {dt}", real=dt == "f64")
    plan.destroy()


DIHEDRAL12 = G.ring(12, 6, 0, 0, 1)
RESTRICT_SPIN = {
    "dihedral12_sz_q1": (DIHEDRAL12, G.ring(12, 6, 1), X.sz_q(12, 1), "c128"),
    "dihedral12_sz_q5": (DIHEDRAL12, G.ring(12, 6, 5), X.sz_q(12, 5), "c128"),
    "dihedral8_staggered_into_reflection": (G.ring(8, 4, 0, 0, 1), G.with_generators(8, 4, [(G.reflection(8), 1)]), X.staggered_z(8), "f64"),
}


@pytest.mark.parametrize("name", sorted(RESTRICT_SPIN))
def test_block_apply_on_restrict_plans(torch, name):
    """the groups="restrict" cases of tests/test_gpu_cross_groups.py with their own rule (cross_groups_reference.compare), column by column"""
    src, dst, op, dt = RESTRICT_SPIN[name]
    ref = G.dense(src, dst, op)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3 and ref["leak"] < 1e-12
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype, groups="restrict")
    xs = _random_block(torch, len(ref["src"]), max(KS), dtype, 7)
    for K in KS:
        assert plan.block_kernel(K) == "k_cross_pull_blk"
        x = xs[:, :K].contiguous()
        y = _nan_block(torch, len(ref["dst"]), K, dtype)
        plan.apply_block(x, y)
        want = ref["matrix"] @ x.cpu().numpy()
        got = y.cpu().numpy()
        for k in range(K):
            G.compare(got[:, k], want[:, k].real if dt == "f64" else want[:, k], G.monomials(op),
                      G.row_scale(X.coefficient_sum(op), ref["n2"], x[:, k].abs().max()), f"restrict block {name} K = {K} column {k}")
    plan.destroy()


FD10 = R.sector(10, 4, F.dihedral(10), [0, 0])
RESTRICT_FERMI = {
    "fd10_n_q3": (FD10, R.sector(10, 4, F.translations(10), [3]), R.n_q(10, 3)),
    "fd10_cdag_q2": (FD10, R.sector(10, 5, F.translations(10), [2]), R.c_dag(10, 2)),
    "spinful_flip_source_n_q1": (R.sector(4, 4, F.translations(4), [0], n_up=2, flip=1), R.sector(4, 4, F.translations(4), [1], n_up=2), R.n_q(4, 1, True)),
}


@pytest.mark.parametrize("name", sorted(RESTRICT_FERMI))
def test_block_apply_on_restrict_plans_of_fermions(torch, name):
    src, dst, model = RESTRICT_FERMI[name]
    ref = R.reference(src, dst, model)
    sbasis, A, sreps, tbasis, treps = _fermi_setup(src, dst, model)
    assert np.array_equal(_u64(sreps), ref["src"]) and np.array_equal(_u64(treps), ref["dst"])
    assert np.abs(ref["matrix"]).max() > 1e-3 and ref["leak"] <= 4e-14
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.complex128, groups="restrict")
    if src["n_up"] is None:
        order = len(F.closure(dst["L"], dst["gens"], dst["secs"]))
    else:
        import fermion_spinful_symm as FS

        order = len(FS.group(dst["L"], dst["gens"], dst["secs"], dst["flip"]))
    xs = _random_block(torch, len(ref["src"]), max(KS), torch.complex128, 5)
    for K in KS:
        assert plan.block_kernel(K) == "k_cross_pull_blk_fermi"
        x = xs[:, :K].contiguous()
        y = _nan_block(torch, len(ref["dst"]), K, torch.complex128)
        plan.apply_block(x, y)
        want, got = ref["matrix"] @ x.cpu().numpy(), y.cpu().numpy()
        for k in range(K):  # n2(r') >= |G2|^-1/2, as in tests/test_gpu_cross_groups.py
            G.compare(got[:, k], want[:, k], len(model), R.coefficient_sum(model) * float(x[:, k].abs().max()) * np.sqrt(order),
                      f"restrict block {name} K = {K} column {k}")
    plan.destroy()


# ---- layouts -------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.25


def _layout_case(torch, which):
    if which == "spin":
        name = "L16_splus_w8_w7_k0_k5"
        src, dst, op, dt = X.ALL_CASES[name]
        sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
        return name, A, sreps, tbasis, treps, X.case_formula(name)["matrix"], X.coefficient_sum(op), "k_cross_pull_blk"
    name = "L12_cdag_q5"
    src, dst, model, _, _, _ = R.CASES[name]
    sbasis, A, sreps, tbasis, treps = _fermi_setup(src, dst, model)
    return name, A, sreps, tbasis, treps, R.case_reference(name)["matrix"], R.coefficient_sum(model), "k_cross_pull_blk_fermi"


@pytest.mark.parametrize("which", ["spin", "fermion"])
@pytest.mark.parametrize("K", [3, 9])
def test_block_layouts(torch, which, K):
    """interleaved, column-major (a transposed (K, n) tensor), and [:, 1::2] views of blocks twice as wide whose other columns hold a
    sentinel that must survive in Y"""
    name, A, sreps, tbasis, treps, mat, csum, kernel = _layout_case(torch, which)
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128)
    assert plan.block_kernel(K) == kernel
    n_dst, n_src = mat.shape
    x = _random_block(torch, n_src, K, c128, 11)
    want = mat @ x.cpu().numpy()
    scale = csum * x.abs().amax(dim=0).cpu().numpy()
    # interleaved
    y = _nan_block(torch, n_dst, K, c128)
    assert x.stride() == (K, 1) and y.stride() == (K, 1)
    plan.apply_block(x, y)
    _spin_rule(y.cpu().numpy(), want, scale, f"{name} interleaved K = {K}")
    # column-major
    xc = x.t().contiguous().t()
    yc = torch.full((K, n_dst), float("nan"), dtype=c128, device="cuda").t()
    assert xc.stride() == (1, n_src) and yc.stride() == (1, n_dst)
    plan.apply_block(xc, yc)
    _spin_rule(yc.cpu().numpy(), want, scale, f"{name} column-major K = {K}")
    # every other column of a block twice as wide
    wide_x = torch.full((n_src, 2 * K), SENTINEL, dtype=c128, device="cuda")
    wide_y = torch.full((n_dst, 2 * K), SENTINEL, dtype=c128, device="cuda")
    wide_x[:, 1::2] = x
    wide_y[:, 1::2] = float("nan")
    plan.apply_block(wide_x[:, 1::2], wide_y[:, 1::2])
    _spin_rule(wide_y[:, 1::2].cpu().numpy(), want, scale, f"{name} [:, 1::2] K = {K}")
    assert bool((wide_y[:, 0::2] == SENTINEL).all()) and bool((wide_x[:, 0::2] == SENTINEL).all())
    plan.destroy()


# ---- several tiles per workgroup -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L16_sz_k0_k5", "L16_splus_w8_w7_k0_k5", "L12_identity_index"])
def test_one_workgroup_walks_every_tile(torch, monkeypatch, name):
    """LS_AMD_CROSS_BLOCKS=1: one row block per chunk of columns walks 4, 3 and 16 tiles, so the accumulators of a tile must not
    leak into the next"""
    monkeypatch.setenv("LS_AMD_CROSS_BLOCKS", "1")
    src, dst, op, dt = X.ALL_CASES[name]
    ref = X.case_formula(name)
    dtype = _dtype(torch, dt)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    assert treps.numel() > 2 * 256
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, dtype)
    _check_spin_like(torch, plan, ref["matrix"], X.coefficient_sum(op), dtype, name + " one workgroup", Ks=(3, 9), real=dt == "f64")
    plan.destroy()


# ---- project plans take the column loop ------------------------------------------------------------------------------------------
def test_project_plans_loop_over_the_columns(torch):
    src, dst, op = DIHEDRAL12, G.ring(12, 6, 2), G.hop_q_plus_sz0(12, 1)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128, groups="project")
    K = 5
    assert plan.block_kernel(K) == "columns" and plan.block_kernel(64) == "columns"
    x = _random_block(torch, sreps.numel(), K, c128, 3)
    y = _nan_block(torch, treps.numel(), K, c128)
    plan.apply_block(x, y)
    yt = torch.full((K, treps.numel()), float("nan"), dtype=c128, device="cuda").t()  # column-major: no scratch column on the way out
    plan.apply_block(x.t().contiguous().t(), yt)
    for k in range(K):
        yk = _nan_block(torch, treps.numel(), 1, c128)[:, 0]
        plan.apply(x[:, k].contiguous(), yk)
        assert float(yk.abs().max()) > 1e-3
        # k_cross_project adds a row's packets in registers in a fixed order: the same kernel on the same column returns the same bytes
        assert torch.equal(y[:, k].contiguous().view(torch.float64), yk.view(torch.float64)), k
        assert torch.equal(yt[:, k].contiguous().view(torch.float64), yk.view(torch.float64)), k
    plan.destroy()


# ---- failures that must be loud --------------------------------------------------------------------------------------------------
def test_block_refusals(torch):
    sbasis, A, sreps, tbasis, treps = _setup(X.ring(8, 4, 0), X.ring(8, 4, 3), X.sz_q(8, 3))
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128)
    n1, n2 = sreps.numel(), treps.numel()
    assert (n1, n2) == (10, 8)
    mk = lambda n, K, dt=c128, dev="cuda": torch.zeros((n, K), dtype=dt, device=dev)  # noqa: E731
    with pytest.raises(D.LsAmdError, match=r"K = 0 is outside \[1, 64\]"):
        plan.apply_block(mk(n1, 0), mk(n2, 0))
    with pytest.raises(D.LsAmdError, match=r"K = 65 is outside \[1, 64\]"):
        plan.apply_block(mk(n1, 65), mk(n2, 65))
    with pytest.raises(D.LsAmdError, match=r"K = 65 is outside \[1, 64\]"):
        plan.block_kernel(65)
    with pytest.raises(D.LsAmdError, match="x is torch.float64"):
        plan.apply_block(mk(n1, 2, torch.float64), mk(n2, 2))
    with pytest.raises(D.LsAmdError, match="y is torch.float64"):
        plan.apply_block(mk(n1, 2), mk(n2, 2, torch.float64))
    with pytest.raises(D.LsAmdError, match=r"x \(8, 2\) must be \(10, K\)"):
        plan.apply_block(mk(n2, 2), mk(n2, 2))
    with pytest.raises(D.LsAmdError, match=r"y \(10, 2\) \(8, K\)"):
        plan.apply_block(mk(n1, 2), mk(n1, 2))
    with pytest.raises(D.LsAmdError, match="x must be a device tensor"):
        plan.apply_block(mk(n1, 2, dev="cpu"), mk(n2, 2))
    with pytest.raises(D.LsAmdError, match="y must be a device tensor"):
        plan.apply_block(mk(n1, 2), mk(n2, 2, dev="cpu"))
    with pytest.raises(D.LsAmdError, match="2-D"):
        plan.apply_block(mk(n1, 2)[:, 0], mk(n2, 2)[:, 0])
    with pytest.raises(D.LsAmdError, match=r"x \(10, 2\) must be \(10, K\) and y \(8, 3\)"):
        plan.apply_block(mk(n1, 2), mk(n2, 3))
    buf = torch.zeros(64, dtype=c128, device="cuda")
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        plan.apply_block(buf[:20].view(n1, 2), buf[10:26].view(n2, 2))
    with pytest.raises(D.LsAmdError, match="share storage"):
        plan.apply_block(mk(n1, 2), buf[:2].view(1, 2).expand(n2, 2))
    # the two layouts every block entry refuses (tests/test_kpm_abi.py): row stride 1, column stride 1 at K = 4, of X and of Y ...
    with pytest.raises(D.LsAmdError, match=r"share storage"):
        plan.apply_block(torch.as_strided(buf, (n1, 4), (1, 1)), mk(n2, 4))
    with pytest.raises(D.LsAmdError, match=r"strides \(row 1, column 1\) of Y make two elements of the 8 x 4 block share storage"):
        plan.apply_block(mk(n1, 4), torch.as_strided(buf, (n2, 4), (1, 1)))
    # ... and the interleaved halves of one buffer, whose address ranges overlap (n_src and n_dst rows: 10 and 8)
    big = torch.zeros((n1, 8), dtype=c128, device="cuda")
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        plan.apply_block(big[:, :4], big[:n2, 4:])
    with pytest.raises(D.LsAmdError, match="X and Y overlap"):
        plan.apply_block(big[:, 4:], big[:n2, :4])
    # ... and nothing of that left a flag or a broken plan behind
    x = _random_block(torch, n1, 2, c128, 1)
    y = _nan_block(torch, n2, 2, c128)
    plan.apply_block(x, y)
    assert bool(torch.isfinite(y.abs()).all())
    plan.destroy()


def test_an_operator_that_leaves_the_source_basis_raises_from_check(torch):
    """sigma^+_0 handed a target of the SAME weight (tests/test_gpu_cross_sector.py has the single-vector form): the block kernel
    raises the same flag, and check() reports it with the same message"""
    plain = {"basis": {"number_spins": 12, "hamming_weight": 6, "symmetries": []}}
    sbasis, A, sreps, tbasis, treps = _setup(plain, plain, {"terms": [{"expression": "σ⁺₀", "sites": [[0]]}]})
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, torch.float64)
    x = _random_block(torch, sreps.numel(), 3, torch.float64, 1)
    y = torch.zeros((treps.numel(), 3), dtype=torch.float64, device="cuda")
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.apply_block(x, y)
    plan.apply_block(x, y, check=False)  # the flag is read back by check(), whenever that is called
    with pytest.raises(D.LsAmdError, match="not in the source basis"):
        plan.check()
    plan.check()  # reported once


# ---- a medium size, against the single-vector kernel -----------------------------------------------------------------------------
def test_medium_ring_against_eight_single_applies(torch):
    """24-site ring with translations, weight 12 at k = 0 into weight 11 at k = 5 by S^+_q: 24 flip groups, 6 passes, ~10^5 rows,
    hundreds of tiles; the interleaved block of 8 against 8 calls of apply (k_cross_pull), by _compare's formula"""
    L, K = 24, 8
    src, dst, op = X.ring(L, 12, 0), X.ring(L, 11, 5), X.splus_q(L, 5)
    sbasis, A, sreps, tbasis, treps = _setup(src, dst, op)
    c128 = torch.complex128
    plan = D.CrossSectorPlan(A, sreps, tbasis, treps, c128)
    assert plan.kernel == "k_cross_pull" and plan.block_kernel(K) == "k_cross_pull_blk" and plan.nnz > treps.numel()
    assert sreps.numel() > 100000 and treps.numel() > 100000
    x = _random_block(torch, sreps.numel(), K, c128, 24)
    y = _nan_block(torch, treps.numel(), K, c128)
    plan.apply_block(x, y)
    want = torch.empty((K, treps.numel()), dtype=c128, device="cuda")
    for k in range(K):
        plan.apply(x[:, k].contiguous(), want[k])
    assert float(want.abs().max()) > 1e-3
    scale = X.coefficient_sum(op) * x.abs().amax(dim=0).cpu().numpy()
    _spin_rule(y.cpu().numpy(), want.t().cpu().numpy(), scale, "24-site ring S^+_q, block of 8 against 8 applies")
    plan.destroy()


# ---- thermal_correlation against dense matrices ----------------------------------------------------------------------------------
TIMES = [0.0, 0.5, 1.0, 2.5]
BETAS = [0.0, 0.7, 3.0]


def _heisenberg_section(L):
    bonds = [[i, (i + 1) % L] for i in range(L)]
    return {"name": "Heisenberg", "terms": [{"expression": "σˣ₀ σˣ₁", "sites": bonds}, {"expression": "σʸ₀ σʸ₁", "sites": bonds},
                                            {"expression": "σᶻ₀ σᶻ₁", "sites": bonds}]}


def _full(basis_cfg, op_cfg):
    A = X.full_matrix(basis_cfg, op_cfg)
    return np.asarray(A.todense() if hasattr(A, "todense") else A)


def _sector_hamiltonian(basis_cfg, L):
    """(reps, B^+ H B) from the isometry and the full matrix of tests/cross_sector_reference.py"""
    reps, B = X.isometry(basis_cfg)
    H = _full(basis_cfg, _heisenberg_section(L))
    Hs = B.conj().T @ H @ B
    assert np.abs(Hs - Hs.conj().T).max() <= 1e-12
    return reps, 0.5 * (Hs + Hs.conj().T)


_dense_cache = {}


def _dense_case(name):
    """{"Es", "Us", "Et", "Ut": eigendecompositions of H in the two sectors; "A": the reference matrix; "bounds": the dense extremes
    of both sectors widened by 1 %; "norm": ||A||_2}; computed once per case"""
    if name not in _dense_cache:
        src, dst, op, _ = X.ALL_CASES[name]
        ref = X.case_formula(name)
        r1, Hs = _sector_hamiltonian(src, 8)
        r2, Ht = _sector_hamiltonian(dst, 8)
        assert np.array_equal(r1, ref["src"]) and np.array_equal(r2, ref["dst"])
        Es, Us = np.linalg.eigh(Hs)
        Et, Ut = np.linalg.eigh(Ht)
        lo, hi = min(Es[0], Et[0]), max(Es[-1], Et[-1])
        w = hi - lo
        _dense_cache[name] = {"Es": Es, "Us": Us, "Et": Et, "Ut": Ut, "A": ref["matrix"], "bounds": (float(lo - 0.01 * w), float(hi + 0.01 * w)),
                              "norm": float(np.linalg.norm(ref["matrix"], 2))}
    return _dense_cache[name]


def _dense_typicality(d, Rv, beta, e_ref, times):
    """(N [T, K], Z [K]) of the module docstring by eigendecomposition"""
    Es, Us, Et, Ut, A = d["Es"], d["Us"], d["Et"], d["Ut"], d["A"]
    b = Us @ (np.exp(-0.5 * beta * (Es - e_ref))[:, None] * (Us.conj().T @ Rv))
    Z = (np.abs(b) ** 2).sum(axis=0)
    phi = A @ b
    N = np.empty((len(times), Rv.shape[1]), dtype=complex)
    for j, t in enumerate(times):
        bt = Us @ (np.exp(-1j * Es * t)[:, None] * (Us.conj().T @ b))
        pt = Ut @ (np.exp(-1j * Et * t)[:, None] * (Ut.conj().T @ phi))
        N[j] = ((A @ bt).conj() * pt).sum(axis=0)
    return N, Z


def _exact_sector_average(d, beta, times):
    """(1 / Z_s) sum_{n, m} e^{-beta E_n} e^{i (E_n - E_m) t} |<m|A|n>|^2"""
    Es, Et = d["Es"], d["Et"]
    w = np.abs(d["Ut"].conj().T @ d["A"] @ d["Us"]) ** 2  # [m, n]
    p = np.exp(-beta * (Es - Es.min()))
    out = np.array([(w * np.exp(1j * (Es[None, :] - Et[:, None]) * t) * p[None, :]).sum() for t in times])
    return out / p.sum()


def _thermal_config(name):
    src, dst, op, _ = X.ALL_CASES[name]
    cfg = {"basis": src["basis"], "hamiltonian": _heisenberg_section(8), "observables": [op]}
    return cfg, dst


@pytest.mark.parametrize("name", ["L8_sz_k0_k3", "L8_splus_w4_w3_k1_k4"])
def test_thermal_correlation_matches_the_eigendecomposition(torch, name):
    d = _dense_case(name)
    cfg, dst = _thermal_config(name)
    sbasis = D.loadConfigFromDict({"basis": cfg["basis"]})
    sreps, _ = D.enumerateStates(sbasis, 1)
    K = 3
    Rv = torch.stack([D.fillRandom(sreps[0], 21 + k, torch.complex128) for k in range(K)], dim=1)
    assert d["norm"] > 0.1
    worst_n = worst_z = 0.0
    for beta in BETAS:
        res = thermal_correlation(cfg, 0, beta, TIMES, vectors=Rv, target=dst, bounds=d["bounds"])
        assert res.kernel == "k_cross_pull_blk" and res.dimension == len(d["Es"]) and res.bounds == d["bounds"]
        assert res.reference_energy == d["bounds"][0]
        assert res.numerator.shape == (len(TIMES), K) and res.partition.shape == (K,) and res.correlation.shape == (len(TIMES),)
        assert res.orders.shape == (len(TIMES),) and res.orders[0] == 0 and (res.orders[1:] > 0).all()
        # every segment moves K columns through N orders in each of the two sectors; the cooling step comes on top
        moved = 2 * K * int(res.orders.sum())
        assert res.matvec_columns == moved if beta == 0.0 else res.matvec_columns > moved
        N, Z = _dense_typicality(d, Rv.cpu().numpy(), beta, res.reference_energy, TIMES)
        assert Z.min() > 1e-6 and np.abs(N).max() > 1e-6
        rn = float((np.abs(res.numerator - N) / (1e-10 * d["norm"] ** 2 * Z[None, :])).max())
        rz = float((np.abs(res.partition - Z) / (1e-11 * Z)).max())
        worst_n, worst_z = max(worst_n, rn), max(worst_z, rz)
        print(f"thermal_correlation {name} beta = {beta}: orders {res.orders.tolist()}, |N| up to {np.abs(N).max():.3e}, Z {Z.min():.3e}..{Z.max():.3e}, "
              f"numerator error / bound {rn:.3g}, partition error / bound {rz:.3g}")
        assert np.abs(res.correlation - res.numerator.sum(axis=1) / res.partition.sum()).max() <= 1e-15 * d["norm"] ** 2
        assert rn <= 1.0 and rz <= 1.0, (name, beta, rn, rz)
    print(f"thermal_correlation {name}: worst numerator error / bound {worst_n:.3g}, worst partition error / bound {worst_z:.3g}")


def test_thermal_correlation_over_a_whole_basis_is_the_exact_trace(torch):
    """vectors = the 10 x 10 identity: the typicality average IS the trace over the sector"""
    name = "L8_sz_k0_k3"
    d = _dense_case(name)
    cfg, dst = _thermal_config(name)
    eye = torch.eye(10, dtype=torch.complex128, device="cuda")
    for beta in BETAS:
        res = thermal_correlation(cfg, 0, beta, TIMES, vectors=eye, target=dst, bounds=d["bounds"])
        want = _exact_sector_average(d, beta, TIMES)
        assert abs(want[0]) > 1e-3 and abs(want[0].imag) <= 1e-13 * abs(want[0])  # C(0) = <A^+ A> is real and positive
        ratio = float((np.abs(res.correlation - want) / (1e-10 * d["norm"] ** 2)).max())
        print(f"exact trace beta = {beta}: C(t) = {np.array2string(res.correlation, precision=6)}, error / bound {ratio:.3g}")
        assert ratio <= 1.0, (beta, ratio)


def test_canonical_ensemble_over_all_momentum_sectors(torch):
    """8-site ring at weight 4, A = S^z_q with q = 3: the eight sectors k -> k + 3 with identity vectors, one E_ref and one pair of
    bounds, combined by combine_sectors, against the dense trace over the 70 states of the weight sector"""
    L, q = 8, 3
    plain = {"basis": {"number_spins": L, "hamming_weight": 4, "symmetries": []}}
    states = np.array([s for s in range(1 << L) if bin(s).count("1") == 4])
    assert len(states) == 70
    H = _full(plain, _heisenberg_section(L))[np.ix_(states, states)]
    A = _full(plain, X.sz_q(L, q))[np.ix_(states, states)]
    assert np.abs(H - H.conj().T).max() <= 1e-13
    E, U = np.linalg.eigh(0.5 * (H + H.conj().T))
    w = E[-1] - E[0]
    bounds = (float(E[0] - 0.01 * w), float(E[-1] + 0.01 * w))
    e_ref = bounds[0]
    norm = float(np.linalg.norm(A, 2))
    Ae = U.conj().T @ A @ U  # <m|A|n>
    worst = 0.0
    for beta in (0.0, 0.7):
        results, dims = [], []
        for k in range(L):
            cfg = {"basis": X.ring(L, 4, k)["basis"], "hamiltonian": _heisenberg_section(L), "observables": [X.sz_q(L, q)]}
            n = D.enumerateStates(D.loadConfigFromDict({"basis": cfg["basis"]}), 1)[0][0].numel()
            dims.append(n)
            eye = torch.eye(n, dtype=torch.complex128, device="cuda")
            results.append(thermal_correlation(cfg, 0, beta, TIMES, vectors=eye, target=X.ring(L, 4, (k + q) % L), bounds=bounds, reference_energy=e_ref))
            assert results[-1].dimension == n and results[-1].reference_energy == e_ref
        assert dims == [10, 8, 9, 8, 10, 8, 9, 8] and sum(dims) == 70
        got = combine_sectors(results)
        p = np.exp(-beta * (E - E[0]))
        want = np.array([((np.abs(Ae) ** 2) * np.exp(1j * (E[None, :] - E[:, None]) * t) * p[None, :]).sum() for t in TIMES]) / p.sum()
        assert abs(want[0]) > 1e-3
        ratio = float((np.abs(got - want) / (1e-10 * norm ** 2)).max())
        worst = max(worst, ratio)
        print(f"canonical ensemble beta = {beta}: C(t) = {np.array2string(got, precision=6)}, error / bound {ratio:.3g}")
        assert ratio <= 1.0, (beta, ratio)
    print(f"canonical ensemble: worst error / bound {worst:.3g}")


def test_thermal_correlation_inside_one_sector(torch):
    """target=None: A maps the sector into itself (the bond operator sum_j sigma^z_j sigma^z_{j+1} at k = 0), both vectors move under one
    operator, and the plan is a cross plan from the basis to itself; identity vectors against the dense trace over the sector"""
    L = 8
    src = X.ring(L, 4, 0)
    bond = {"terms": [{"expression": "σᶻ₀ σᶻ₁", "sites": [[i, (i + 1) % L] for i in range(L)]}]}
    reps, B = X.isometry(src)
    _, H = _sector_hamiltonian(src, L)
    A = B.conj().T @ _full(src, bond) @ B
    E, U = np.linalg.eigh(H)
    w = E[-1] - E[0]
    bounds = (float(E[0] - 0.01 * w), float(E[-1] + 0.01 * w))
    norm = float(np.linalg.norm(A, 2))
    d = {"Es": E, "Us": U, "Et": E, "Ut": U, "A": A}
    cfg = {"basis": src["basis"], "hamiltonian": _heisenberg_section(L), "observables": [bond]}
    eye = torch.eye(len(reps), dtype=torch.complex128, device="cuda")
    for beta in (0.0, 0.7):
        res = thermal_correlation(cfg, 0, beta, TIMES, vectors=eye, bounds=bounds)
        assert res.kernel == "k_cross_pull_blk" and res.dimension == 10
        want = _exact_sector_average(d, beta, TIMES)
        assert abs(want[0]) > 1e-3 and np.abs(want - want[0]).max() > 1e-3  # A does not commute with H: C(t) moves
        ratio = float((np.abs(res.correlation - want) / (1e-10 * norm ** 2)).max())
        print(f"one sector beta = {beta}: C(t) = {np.array2string(res.correlation, precision=6)}, error / bound {ratio:.3g}")
        assert ratio <= 1.0, (beta, ratio)
