"""Every symmetry-projected SPIN matvec path against operators that are not a real sum of exchange pairs of one amplitude: the fixed
table of tests/projected_cases.py (transverse fields, dimerised couplings, a complex scalar chirality, four-site plaquette terms,
directed hopping; 32- and 64-bit words; trivial, -1 and complex characters, with and without the global flip in the group).  Each
row asserts the dispatch kind of pull_kinds() (csrc/k_pull_t.hpp) it is there for -- (TRIVIAL, REAL), (TRIVIAL, CPLX), (PM1, CPLX),
which the Heisenberg models never reach, next to the three they do -- and every path is compared with tests/sector_reference.py, an
explicit sparse projector that shares no code with the library (validated without a GPU by tests/test_sector_reference.py).

Tolerance: the project's rule, max|got - want| <= 1e-12 max(1, max|want|), on every path.  Every comparison prints its error first
(pytest -s shows `ERR case path value`)."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from distributed_matvec_amd import _lib
from oracle import model as M
from projected_cases import CASES, HERMITIAN, NON_HERMITIAN, config_of, k4_mode_of, reference_of
from test_gpu_block_matvec import device_block, random_block
from test_gpu_kpm import assert_close, assert_dots, coefficient_sets

pytestmark = pytest.mark.gpu

COEF_NAME = {5: "UNI", 13: "REAL", 21: "CPLX"}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


class Case:
    """operator, basis, representatives and reference of one row of the table; built once per module"""

    def __init__(self, torch, name):
        self.name = name
        _, _, self.is_real, self.is_hermitian, self.k4, self.packet, _ = CASES[name]
        self.cfg = config_of(name)
        self.model = M.model_from_config(self.cfg)
        self.want_reps, self.H, leak = reference_of(name)
        assert leak <= 1e-12, (name, leak)
        self.n = len(self.want_reps)
        self.basis, self.h = D.loadConfigFromDict(self.cfg, hamiltonian=True)
        self.reps, _ = D.enumerateStates(self.basis, 1)
        # an f64 vector too where the operator is real and the characters are +-1
        self.dtypes = [torch.complex128] + ([torch.float64] if self.is_real and self.k4 != "GENERAL" else [])
        self.parts = {}

    def vector(self, torch, dtype, seed):
        rs = np.random.RandomState(seed)
        x = rs.rand(self.n) - 0.5
        if dtype == torch.complex128:
            x = x + 1j * (rs.rand(self.n) - 0.5)
        return x, self.H @ x

    def partitions(self, P):
        if P not in self.parts:
            self.parts[P] = D.enumerateStates(self.basis, P)
        return self.parts[P]


_cases = {}


def case_of(torch, name):
    if name not in _cases:
        _cases[name] = Case(torch, name)
    return _cases[name]


def tag(torch, dtype):
    return "c128" if dtype == torch.complex128 else "f64"


def close(got, want, case, path):
    err = np.abs(got - want).max()
    print(f"ERR {case} {path} {err:.2e} (max|want| {np.abs(want).max():.2f})")
    assert_close(got, want, (case, path))


def apply_plan(torch, pl, x):
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    yd = torch.full_like(xd, -7.0)  # (every operator of the table has diagonal terms: y is assigned)
    pl.matvec([xd], [yd])
    return yd.cpu().numpy()


def stage_a_packets(c):
    """packets the pull kernel's stage A makes: per row, the flip masks whose terms sum to a non-zero coefficient -- out of the
    oracle's term tables, not the library's"""
    rows = c.want_reps
    off = c.model.offdiag
    total = 0
    for x in sorted(set(int(v) for v in off.x)):
        coef = np.zeros(len(rows), dtype=complex)
        for v, m, r, s in zip(off.v[off.x == x], off.m[off.x == x], off.r[off.x == x], off.s[off.x == x]):
            assert int(s) == 0  # (matrix-element terms carry no sign mask)
            coef[(rows & m) == r] += v
        total += int((np.abs(coef) > 1e-12).sum())
    return total


# ---------------------------------------------------------------------------------------------
# the row of the table: representatives, flags, kernel, coefficient kind
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_what_the_table_says(torch, name):
    c = case_of(torch, name)
    assert np.array_equal(c.reps[0].cpu().numpy().view(np.uint64), c.want_reps)  # bit for bit
    assert c.n > 256  # more than one tile and window
    assert c.h.isReal == c.is_real and c.h.isHermitian == c.is_hermitian
    assert k4_mode_of(c.model) == c.k4
    assert c.basis.requiresProjection() and c.basis.hasPermutationSymmetries()
    if not c.is_hermitian:
        pl = D.MatvecPlan(c.h, c.reps, torch.complex128)
        assert pl.kernel == "tile"
        assert pl.cache_slots(0) == 0 and pl.slot_cache == (0, 0)  # nothing to cache on the push path
        pl.destroy()
        return
    pl = D.MatvecPlan(c.h, c.reps, torch.complex128, mode="pull")
    assert pl.kernel == "tile-pull+indexed"
    assert pl.cache_slots(0) == c.n and pl.kernel == "tile-pull+indexed+cached"
    rows, cbytes = pl.slot_cache
    pl.destroy()
    # host.c, slot cache: bytes = packets x (4 + 1 + 8 x doubles of coefficient) + 12 per stream of 64 rows + 8
    streams = (c.n + 63) // 64
    packets = stage_a_packets(c)
    per_packet = (cbytes - 12 * streams - 8) / packets
    print(f"KIND {name}: n = {c.n}, {packets} packets, {cbytes} bytes cached = {per_packet:.3f} per packet -> ({c.k4}, {COEF_NAME[c.packet]})")
    assert rows == c.n and cbytes == packets * c.packet + 12 * streams + 8, (name, per_packet, c.packet)


# ---------------------------------------------------------------------------------------------
# the one-partition pull forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", ["0", "37", "256"])
@pytest.mark.parametrize("name", HERMITIAN)
def test_fused_pull(torch, monkeypatch, name, halo):
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_PULL_INDEXED", "1")
    monkeypatch.setenv("LS_AMD_PULL_HALO", halo)
    monkeypatch.setenv("LS_AMD_PULL_SPLIT", "0")
    for dtype in c.dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
        assert pl.kernel == "tile-pull+indexed"
        assert _lib.load().ls_amd_internal_plan_split_active(pl.h) == 0  # one kernel
        x, want = c.vector(torch, dtype, 52)
        close(apply_plan(torch, pl, x), want, name, f"fused/halo={halo}/{tag(torch, dtype)}")
        pl.destroy()


@pytest.mark.parametrize("rounds", ["one-round", "tile-rounds"])
@pytest.mark.parametrize("name", HERMITIAN)
def test_split_pull(torch, monkeypatch, name, rounds):
    """resolve | gather over the rows a packet buffer holds: every row in one round, and one 256-row tile per round"""
    c = case_of(torch, name)
    # host.c ls_amd_internal_plan_split_enable: a stream of 64 rows reserves 64 x groups packets + 4 bytes; the buffer below holds
    # between four and seven such streams, i.e. one tile (also if the library keeps up to twice the oracle's flip masks as groups)
    per_stream = 64 * c.model.max_off_diag * c.packet + 4
    monkeypatch.setenv("LS_AMD_PULL_INDEXED", "1")
    monkeypatch.setenv("LS_AMD_PULL_HALO", "37")
    monkeypatch.setenv("LS_AMD_PULL_SPLIT", "1000000000" if rounds == "one-round" else str(8 * per_stream - 8))
    for dtype in c.dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
        assert pl.kernel == "tile-pull+indexed"
        split_rows = _lib.load().ls_amd_internal_plan_split_active(pl.h)
        if rounds == "one-round":
            assert split_rows == c.n
        else:
            assert 0 < split_rows < c.n and split_rows % 256 == 0, (split_rows, c.n)
        x, want = c.vector(torch, dtype, 53)
        close(apply_plan(torch, pl, x), want, name, f"split/{rounds}/{tag(torch, dtype)}")
        pl.destroy()


@pytest.mark.parametrize("name", HERMITIAN)
def test_slot_cache(torch, name):
    """the cached streams depend on operator and basis only: three different vectors after the resolving call, with every row
    cached and with a prefix of whole tiles (the others run the fused kernel)"""
    c = case_of(torch, name)
    for dtype in c.dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
        assert pl.cache_slots(0) == c.n and pl.kernel == "tile-pull+indexed+cached"
        full_bytes = pl.slot_cache[1]
        for trial in range(4):  # 0 resolves + gathers, 1..3 only gather
            x, want = c.vector(torch, dtype, 61 + trial)
            close(apply_plan(torch, pl, x), want, name, f"cached/full/{trial}/{tag(torch, dtype)}")
        pl.destroy()
        # a third of the bytes; where that admits no whole tile (two or three tiles in all), two thirds
        prefixes = []
        for ceiling in (full_bytes // 3, 2 * full_bytes // 3):
            pp = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
            prows = pp.cache_slots(ceiling)
            assert prows % 256 == 0 and prows < c.n and pp.slot_cache[1] <= ceiling, (prows, pp.slot_cache, ceiling)
            assert pp.kernel == ("tile-pull+indexed+cached" if prows else "tile-pull+indexed")
            prefixes.append(prows)
            for trial in range(4):
                x, want = c.vector(torch, dtype, 71 + trial)
                close(apply_plan(torch, pp, x), want, name, f"cached/prefix={prows}/{trial}/{tag(torch, dtype)}")
            pp.destroy()
            if prows:
                break
        # (four tiles or more of comparable length: a third of the bytes holds one; three: two thirds do)
        assert (prefixes[0] > 0 if c.n > 1024 else max(prefixes) > 0 if c.n > 512 else True), (name, prefixes)


@pytest.mark.parametrize("name", HERMITIAN)
def test_value_table_and_hash_table_forms(torch, monkeypatch, name):
    """LS_AMD_PULL_VALUES=1 (f64: the value table; c128: falls back to the index table) and LS_AMD_PULL_INDEXED=0 (k_tile_pull over
    the {representative -> x} hash table)"""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_PULL_INDEXED", "1")
    monkeypatch.setenv("LS_AMD_PULL_VALUES", "1")
    for dtype in c.dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
        assert pl.kernel == ("tile-pull+values" if dtype == torch.float64 else "tile-pull+indexed")  # the table holds f64 values
        for trial in range(2):  # another x: the refresh replaces every value
            x, want = c.vector(torch, dtype, 152 + trial)
            close(apply_plan(torch, pl, x), want, name, f"values/{trial}/{pl.kernel}/{tag(torch, dtype)}")
        pl.destroy()
    monkeypatch.setenv("LS_AMD_PULL_VALUES", "0")
    monkeypatch.setenv("LS_AMD_PULL_INDEXED", "0")
    for halo in ("512", "0"):
        monkeypatch.setenv("LS_AMD_PULL_HALO", halo)
        for dtype in c.dtypes:
            pl = D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
            assert pl.kernel == "tile-pull"
            for trial in range(2):
                x, want = c.vector(torch, dtype, 162 + trial)
                close(apply_plan(torch, pl, x), want, name, f"hash-table/halo={halo}/{trial}/{tag(torch, dtype)}")
            pl.destroy()


# ---------------------------------------------------------------------------------------------
# push, partitions, replicated x
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HERMITIAN)
def test_push_mode(torch, name):
    c = case_of(torch, name)
    for dtype in c.dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="push")
        assert pl.kernel == "tile"
        x, want = c.vector(torch, dtype, 81)
        close(apply_plan(torch, pl, x), want, name, f"push/{tag(torch, dtype)}")
        pl.destroy()


def partitioned(torch, c, P, dtype, seed, path):
    parts, masks = c.partitions(P)
    assert np.array_equal(D.arrFromHashedToBlock(parts, masks).cpu().numpy().view(np.uint64), c.want_reps)
    x, want = c.vector(torch, dtype, seed)
    xs = D.arrFromBlockToHashed(torch.from_numpy(x).cuda(), masks, P)
    ys = [torch.full_like(v, 3.0) for v in xs]
    pl = D.MatvecPlan(c.h, parts, dtype)
    pl.matvec(xs, ys)
    assert pl.kernel.startswith("tile") and "pull" not in pl.kernel, pl.kernel  # packets
    # 8-byte state + the value: what the VECTOR's type takes; an operator with complex coefficients only has c128 plans
    assert pl.packet_bytes == (24 if dtype == torch.complex128 else 16)
    assert c.is_real or pl.packet_bytes == 24
    close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, c.name, f"{path}/{tag(torch, dtype)}")
    pl.destroy()


@pytest.mark.parametrize("name", HERMITIAN)
def test_three_partitions(torch, name):
    c = case_of(torch, name)
    for dtype in c.dtypes:
        partitioned(torch, c, 3, dtype, 91, "P=3")


def replicated(torch, c, P, dtype):
    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    x, want = c.vector(torch, dtype, 60)
    xg = torch.from_numpy(x).cuda()
    ys = []
    for p in range(P):
        pl = D.ReplicatedPlan(c.h, parts[p], reps_global, dtype, P, p)
        assert pl.kernel == "replicated-tile-pull"  # (the entry of one rank alone: x through the {representative -> x} table)
        y = torch.full((parts[p].numel(),), 3.0, dtype=dtype, device="cuda")
        pl.matvec(xg, y)
        ys.append(y)
        pl.destroy()
    close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, c.name, f"replicated-x/P={P}/{tag(torch, dtype)}")


@pytest.mark.parametrize("name", HERMITIAN)
def test_replicated_x(torch, name):
    """one partition per process with the whole x replicated, every `rank` in turn on the one device (P = 3)"""
    c = case_of(torch, name)
    for dtype in c.dtypes:
        replicated(torch, c, 3, dtype)


@pytest.mark.parametrize("name", ["chiral_16_k3", "chiral_16_k3_x-1"])
def test_replicated_x_two_partitions(torch, name):
    """P = 2 on the two rows with complex characters AND complex coefficients"""
    c = case_of(torch, name)
    for dtype in c.dtypes:
        replicated(torch, c, 2, dtype)


@pytest.mark.parametrize("name", ["tfim_14_k0_r0_x1", "chiral_16_k0", "chiral_16_k8", "chiral_16_k3_x-1", "chiral_36_4_k5"])
def test_replicated_exchange_ranks_as_threads(torch, name):
    """the INDEXED replicated-x driver (ls_amd_repl_matvec: k_pull_t over the owner-major x as it arrives, owners prescale in the
    trivial sectors; resolve while the blocks travel, then gather) with three ranks as threads over the loop-back transport: the
    three kinds the Heisenberg models do not reach, complex characters with the flip, and 64-bit words"""
    from distributed_matvec_amd.distributed import RcclReplicatedOperator
    from test_gpu_loopback import _run_ranks

    c = case_of(torch, name)
    P, dtype = 3, torch.complex128
    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    x, want = c.vector(torch, dtype, 23)
    xs = D.arrFromBlockToHashed(torch.from_numpy(x).cuda(), masks, P)
    ys = [torch.full_like(v, -3.0) for v in xs]
    kernels = [None] * P

    def body(rank, comm):
        op = RcclReplicatedOperator(c.h, reps_global, masks, dtype, comm=comm)
        kernels[rank] = op.engine.plan.kernel
        for _ in range(2):
            op.matvec(xs[rank], ys[rank], check=True)
        op.rm.destroy()

    comms = _run_ranks(P, body)
    assert all(k == "replicated-tile-pull+indexed" for k in kernels), kernels
    close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, name, "replicated-x/indexed/3-ranks/c128")
    for comm in comms:
        comm.destroy()


# ---------------------------------------------------------------------------------------------
# block and fused steps (LS_AMD_BLOCK=kernel)
# ---------------------------------------------------------------------------------------------
_block_plans = {}


def block_plan(torch, c, dtype):
    key = (c.name, dtype)
    if key not in _block_plans:
        _block_plans[key] = D.MatvecPlan(c.h, c.reps, dtype)
    return _block_plans[key]


@pytest.mark.parametrize("layout", ["interleaved", "colmajor"])
@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("name", HERMITIAN)
def test_block_matvec(torch, monkeypatch, name, K, layout):
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    for dtype in c.dtypes:
        pl = block_plan(torch, c, dtype)
        assert pl.kernel == "tile-pull+indexed" and pl.block_kernel(K) == "k_pull_gather_blk"
        X = random_block(torch, c.n, K, dtype, 7 + K)
        x = device_block(torch, X, layout, dtype)
        y = device_block(torch, X, layout, dtype, fill=float("nan"))
        pl.matvec_block(x, y)
        close(y.cpu().numpy(), c.H @ X, name, f"k_pull_gather_blk/K={K}/{layout}/{tag(torch, dtype)}")


@pytest.mark.parametrize("name", HERMITIAN)
def test_chebyshev_and_accumulate_steps(torch, monkeypatch, name):
    """one matvec_block_axpby with the Chebyshev triple (k_pull_gather_cheb, dots as assert_dots checks them) and one
    matvec_block_axpby_acc with a complex c (k_pull_gather_evolve)"""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    monkeypatch.setenv("LS_AMD_ACC", "fused")
    K, cz = 5, -0.3 + 1.1j
    for dtype in c.dtypes:
        pl = block_plan(torch, c, dtype)
        assert pl.axpby_kernel(K) == "k_pull_gather_cheb" and pl.acc_kernel(K) == "k_pull_gather_evolve"
        X, Y0 = random_block(torch, c.n, K, dtype, 11), random_block(torch, c.n, K, dtype, 31)
        Z0 = random_block(torch, c.n, K, torch.complex128, 51)
        HX = c.H @ X
        al, be, ga = coefficient_sets(HX)[2]
        want = al * HX + be * X + ga * Y0
        x, y = device_block(torch, X, "interleaved", dtype), device_block(torch, Y0, "interleaved", dtype)
        dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
        pl.matvec_block_axpby(x, y, al, be, ga, dots=dots)
        got = y.cpu().numpy()
        close(got, want, name, f"k_pull_gather_cheb/{tag(torch, dtype)}")
        assert_dots(dots.cpu().numpy(), X, got, (name, "cheb"))
        x, y = device_block(torch, X, "colmajor", dtype), device_block(torch, Y0, "colmajor", dtype)
        z = device_block(torch, Z0, "interleaved", torch.complex128)
        dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
        pl.matvec_block_axpby_acc(x, y, al, be, ga, z, cz, dots=dots)
        got = y.cpu().numpy()
        close(got, want, name, f"k_pull_gather_evolve/y/{tag(torch, dtype)}")
        assert_dots(dots.cpu().numpy(), X, got, (name, "evolve"))
        zwant = Z0 + cz * want
        err = np.abs(z.cpu().numpy() - zwant).max()
        print(f"ERR {name} k_pull_gather_evolve/z/{tag(torch, dtype)} {err:.2e}")
        # Z0 + c want: the accumulate adds one rounding to the step's own (test_gpu_evolve.assert_acc)
        assert err <= 1e-12 * max(1.0, np.abs(Z0).max() + abs(cz) * np.abs(want).max()), (name, err)


# ---------------------------------------------------------------------------------------------
# what must be refused, and the operators only the push kernel applies
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NON_HERMITIAN)
def test_non_hermitian_operators_take_the_push_kernel(torch, name):
    c = case_of(torch, name)
    assert np.abs((c.H - c.H.conj().T)).max() > 0.5  # (the reference is not Hermitian either)
    dtypes = [torch.complex128] + ([torch.float64] if c.k4 != "GENERAL" else [])
    for dtype in dtypes:
        pl = D.MatvecPlan(c.h, c.reps, dtype)  # auto
        assert pl.kernel == "tile"
        x, want = c.vector(torch, dtype, 82)
        close(apply_plan(torch, pl, x), want, name, f"auto(tile)/{tag(torch, dtype)}")
        pl.destroy()
        partitioned(torch, c, 3, dtype, 92, "auto(tile)/P=3")
        with pytest.raises(D.LsAmdError, match="pull mode needs a Hermitian operator"):
            D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
        parts, masks = c.partitions(2)
        with pytest.raises(D.LsAmdError, match="replicated-x .pull. plans need a Hermitian operator"):
            D.ReplicatedPlan(c.h, parts[0], D.arrFromHashedToBlock(parts, masks), dtype, 2, 0)
    if c.k4 == "GENERAL":
        with pytest.raises(D.LsAmdError, match="complex characters need dtype c128"):
            D.MatvecPlan(c.h, c.reps, torch.float64)


def test_complex_coefficients_need_c128(torch):
    c = case_of(torch, "chiral_16_k0")  # every character is +1: it is the operator that needs the complex vector
    for mode in ("auto", "pull", "push"):
        with pytest.raises(D.LsAmdError, match="needs dtype c128"):
            D.MatvecPlan(c.h, c.reps, torch.float64, mode=mode)
    parts, masks = c.partitions(2)
    with pytest.raises(D.LsAmdError, match="needs dtype c128"):
        D.ReplicatedPlan(c.h, parts[0], D.arrFromHashedToBlock(parts, masks), torch.float64, 2, 0)
    with pytest.raises(D.LsAmdError, match="needs dtype c128"):
        D.MatvecPlan(c.h, c.partitions(3)[0], torch.float64)


@pytest.mark.parametrize("name", ["jq_16_k0_r1", "chiral_16_k3"])
def test_csr_export_applies_the_same_matrix(torch, name):
    """Operator.to_csr (k_csr.hip over the cross-sector plan) tied to the same reference, for a real and a complex row"""
    c = case_of(torch, name)
    csr = c.h.to_csr(c.reps)
    assert csr.dtype == (torch.float64 if c.is_real and c.k4 != "GENERAL" else torch.complex128)
    assert tuple(csr.shape) == (c.n, c.n) and csr.nnz > c.n
    x, want = c.vector(torch, csr.dtype, 95)
    got = (csr.to_dense() @ torch.from_numpy(x).cuda()).cpu().numpy()
    close(got, want, name, "to_csr")
