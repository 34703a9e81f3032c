"""Every matvec path of spin bases WITHOUT permutation symmetries -- the whole 2^L space, one weight, and their sectors of the global
flip alone -- against operators that are not a real sum of exchange pairs of one amplitude: the fixed table of
tests/unprojected_cases.py (transverse fields, XYZ couplings, a real non-Hermitian matrix with complex coefficients, a complex scalar
chirality, four-site plaquette terms, dimerised and two-domain exchange, directed hopping of a real and of a complex amplitude; 32-
and 64-bit words).  These bases run k_direct in all its instantiations, k_direct_blk / _cheb / _evolve, the packet producers and
consumers, and the replicated-x row kernel with its reach computation (csrc/k_rows.hip, csrc/k_packets.hip, csrc/k_plan.hip).  Every
path is compared with tests/sector_reference.py, an explicit sparse projector that shares no code with the library (validated
without a GPU by tests/test_unprojected_cases.py and tests/test_sector_reference.py).

Tolerance: the project's rule, max|got - want| <= 1e-12 max(1, max|want|), on every path.  Every comparison prints its error first
(pytest -s shows `ERR case path value`).  Every kernel name asserted below is what host.c (ls_amd_plan_create,
ls_amd_plan_kernel_name, block_kernel_of) decides for the row; the rule is quoted where it is asserted."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from test_gpu_block_matvec import device_block, random_block
from test_gpu_kpm import assert_close, assert_dots, coefficient_sets
from unprojected_cases import ALL, CASES, FIXED_WEIGHT, HERMITIAN, INVERSION, NON_HERMITIAN, config_of, reference_of

pytestmark = pytest.mark.gpu

COMPLEX = [name for name in ALL if not CASES[name][2]]
PACKET_ENVS = ("LS_AMD_PACKETS", "LS_AMD_SCATTER_HASH", "LS_AMD_PACKET_INDEX", "LS_AMD_PACKET_STREAMS", "LS_AMD_STREAM_KEYS",
               "LS_AMD_STREAM_PRODUCER", "LS_AMD_PACKET_INDEX_MAX")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


@pytest.fixture(autouse=True)
def default_row_kernel(monkeypatch):
    """the kernel names asserted below are those of the default settings"""
    for k in PACKET_ENVS + ("LS_AMD_ROW_KERNEL", "LS_AMD_MODE", "LS_AMD_REPL_REACH"):
        monkeypatch.delenv(k, raising=False)


class Case:
    """operator, basis, states and reference of one row of the table; built once per module"""

    def __init__(self, torch, name):
        self.name = name
        _, self.args, self.is_real, self.is_hermitian, self.n = CASES[name]
        self.inversion = "X" in self.args
        self.cfg = config_of(name)
        self.want_reps, self.H, leak = reference_of(name)
        assert leak <= 1e-12, (name, leak)
        assert len(self.want_reps) == self.n
        self.basis, self.h = D.loadConfigFromDict(self.cfg, hamiltonian=True)
        self.reps, _ = D.enumerateStates(self.basis, 1)
        # an f64 vector too where the MATRIX is real (twist: complex coefficients, real matrix)
        self.dtypes = [torch.complex128] + ([torch.float64] if self.is_real else [])
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


def pull_kernel_of(name):
    """what ls_amd_plan_create gives a one-partition pull plan of the row under the default LS_AMD_ROW_KERNEL:
      * direct-pull+pairs: setup_pairs -- the full fixed-weight basis without the flip, a real Hermitian operator whose off-diagonal
        groups are all exchange pairs and whose diagonal terms are zz terms on them, no exchange run (dimer_14_7: the amplitudes
        alternate), and 11 w >= 4 L and 11 (L - w) >= 4 L (else the one-row-per-lane variants);
      * direct-pull+staged: chain_eligible -- a real Hermitian operator of exchange runs + at most two other exchange pairs; with the
        flip, L even at weight L / 2.  two_domain_14_7_x1: detect_runs keeps the bond (12, 13) out of the runs of a flip sector, so
        the runs are bonds 0..6 (J = 1) and 7..11 (J = 0.6) and the other pairs are (12, 13) and the closing (0, 13): two;
      * direct-pull: k_direct, everything else (generic groups, complex coefficients, no fixed weight, a non-Hermitian operator)."""
    return {"dimer_14_7": "direct-pull+pairs", "two_domain_14_7_x1": "direct-pull+staged"}.get(name, "direct-pull")


# ---------------------------------------------------------------------------------------------
# a. the row of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_case_is_what_the_table_says(torch, name):
    c = case_of(torch, name)
    assert np.array_equal(c.reps[0].cpu().numpy().view(np.uint64), c.want_reps)  # bit for bit
    assert c.n > 1024  # several tiles and windows
    assert c.h.isReal == c.is_real and c.h.isHermitian == c.is_hermitian
    assert c.basis.requiresProjection() == c.inversion
    assert not c.basis.hasPermutationSymmetries()


# ---------------------------------------------------------------------------------------------
# b. one partition, every mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_one_partition_modes(torch, name):
    c = case_of(torch, name)
    # ls_amd_plan_create: `auto` pulls when the operator is Hermitian OR the basis is unprojected (row i takes <i|H|i ^ x> from the
    # partner's expansion); a flip sector pulls through the Hermiticity of the projected matrix, so a non-Hermitian operator is
    # pushed there and mode="pull" is refused
    pulls = c.is_hermitian or not c.inversion
    for dtype in c.dtypes:
        for mode in ("auto", "pull"):
            if not pulls and mode == "pull":
                with pytest.raises(D.LsAmdError, match="pull mode needs a Hermitian operator"):
                    D.MatvecPlan(c.h, c.reps, dtype, mode="pull")
                continue
            pl = D.MatvecPlan(c.h, c.reps, dtype, mode=mode)
            assert pl.kernel == (pull_kernel_of(name) if pulls else "direct-push"), (mode, pl.kernel)
            x, want = c.vector(torch, dtype, 41)
            close(apply_plan(torch, pl, x), want, name, f"{mode}({pl.kernel})/{tag(torch, dtype)}")
            pl.destroy()
        pl = D.MatvecPlan(c.h, c.reps, dtype, mode="push")
        # push_staged_eligible: no flip, a fixed weight, a real operator with at least one UNDIRECTED exchange run.  No row of the table
        # has one: the runs of hop / phase_hop are directed, dimer's amplitudes alternate, two_domain is a flip sector, and the
        # adjacent pairs of chiral and jq share their flip mask with other terms (generic groups) -- k_direct pushes everywhere
        assert pl.kernel == "direct-push"
        for trial in range(2):  # twice through the same plan
            x, want = c.vector(torch, dtype, 42 + trial)
            close(apply_plan(torch, pl, x), want, name, f"push/{trial}/{tag(torch, dtype)}")
        pl.destroy()


ROW_KERNELS = [("dimer_14_7", "generic", "direct-pull"), ("dimer_14_7", "pairs", "direct-pull+pairs"),
               ("dimer_14_7", "pairrows", "direct-pull+pairrows"), ("dimer_14_7", "pairsites", "direct-pull+pairsites"),
               ("two_domain_14_7_x1", "generic", "direct-pull"), ("phase_hop_14_7", "generic", "direct-pull"),
               ("phase_hop_34_3", "generic", "direct-pull"), ("hop_14_7", "generic", "direct-pull")]


@pytest.mark.parametrize("name,setting,kernel", ROW_KERNELS, ids=[f"{n}-{s}" for n, s, _ in ROW_KERNELS])
def test_row_kernel_settings(torch, monkeypatch, name, setting, kernel):
    """LS_AMD_ROW_KERNEL (setup_pairs, chain_eligible): generic keeps k_direct; pairs / pairrows / pairsites force k_pairs_t, k_pairs_row
    (one row per lane) and k_pairs_site (the degree-2 ring and its two amplitude classes fit the site table); the default setting
    is what test_one_partition_modes runs.  Pull and push, for the directed rows too (no staged kernel takes them either way)."""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", setting)
    for dtype in c.dtypes:
        for mode, want_kernel in (("auto", kernel), ("push", "direct-push")):
            pl = D.MatvecPlan(c.h, c.reps, dtype, mode=mode)
            assert pl.kernel == want_kernel, (mode, pl.kernel)
            for trial in range(2):
                x, want = c.vector(torch, dtype, 44 + trial)
                close(apply_plan(torch, pl, x), want, name, f"ROW_KERNEL={setting}/{mode}({pl.kernel})/{trial}/{tag(torch, dtype)}")
            pl.destroy()


@pytest.mark.parametrize("name", COMPLEX)
def test_complex_coefficients_need_c128(torch, name):
    c = case_of(torch, name)
    assert c.dtypes == [torch.complex128]
    for mode in ("auto", "pull", "push"):
        with pytest.raises(D.LsAmdError, match="needs dtype c128"):
            D.MatvecPlan(c.h, c.reps, torch.float64, mode=mode)
    with pytest.raises(D.LsAmdError, match="needs dtype c128"):
        D.MatvecPlan(c.h, c.partitions(3)[0], torch.float64)


# ---------------------------------------------------------------------------------------------
# c. block and fused steps (LS_AMD_BLOCK=kernel, LS_AMD_ACC=fused)
# ---------------------------------------------------------------------------------------------
_block_plans = {}


def block_plan(torch, c, dtype):
    key = (c.name, dtype)
    if key not in _block_plans:
        _block_plans[key] = D.MatvecPlan(c.h, c.reps, dtype)
    return _block_plans[key]


def block_names(c):
    """block_kernel_of: k_direct_blk (and the fused steps k_direct_cheb / k_direct_evolve) serve pull plans of UNPROJECTED bases,
    Hermitian or not; flip sectors (and their push plans) loop over the columns and finish with the epilogue"""
    return ("columns", "epilogue", "epilogue") if c.inversion else ("k_direct_blk", "k_direct_cheb", "k_direct_evolve")


@pytest.mark.parametrize("layout", ["interleaved", "colmajor"])
@pytest.mark.parametrize("columns", ["3", "chunk+1"])
@pytest.mark.parametrize("name", ALL)
def test_block_matvec(torch, monkeypatch, name, columns, layout):
    """K = 3, and the K around the chunk of columns k_direct_blk keeps in registers (8 of f64, 4 of c128): K = 8 for f64, K = 5 for
    c128.  Y starts as NaN.  Non-Hermitian rows pass the error word nobody reads (host.c ls_amd_matvec_block)."""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    monkeypatch.setenv("LS_AMD_ACC", "fused")
    for dtype in c.dtypes:
        K = 3 if columns == "3" else (8 if dtype == torch.float64 else 5)
        pl = block_plan(torch, c, dtype)
        assert pl.block_kernel(K) == block_names(c)[0]
        X = random_block(torch, c.n, K, dtype, 7 + K)
        x = device_block(torch, X, layout, dtype)
        y = device_block(torch, X, layout, dtype, fill=float("nan"))
        pl.matvec_block(x, y)
        close(y.cpu().numpy(), c.H @ X, name, f"{pl.block_kernel(K)}/K={K}/{layout}/{tag(torch, dtype)}")


@pytest.mark.parametrize("name", ALL)
def test_chebyshev_and_accumulate_steps(torch, monkeypatch, name):
    """one matvec_block_axpby with the Chebyshev triple (k_direct_cheb, dots as assert_dots checks them) and one
    matvec_block_axpby_acc with a complex c (k_direct_evolve); non-Hermitian rows pass the second error word in both
    (host.c ls_amd_matvec_block_axpby, ls_amd_matvec_block_axpby_acc)"""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_BLOCK", "kernel")
    monkeypatch.setenv("LS_AMD_ACC", "fused")
    K, cz = 5, -0.3 + 1.1j
    for dtype in c.dtypes:
        pl = block_plan(torch, c, dtype)
        assert (pl.axpby_kernel(K), pl.acc_kernel(K)) == block_names(c)[1:]
        X, Y0 = random_block(torch, c.n, K, dtype, 11), random_block(torch, c.n, K, dtype, 31)
        Z0 = random_block(torch, c.n, K, torch.complex128, 51)
        HX = c.H @ X
        al, be, ga = coefficient_sets(HX)[2]
        want = al * HX + be * X + ga * Y0
        x, y = device_block(torch, X, "interleaved", dtype), device_block(torch, Y0, "interleaved", dtype)
        dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
        pl.matvec_block_axpby(x, y, al, be, ga, dots=dots)
        got = y.cpu().numpy()
        close(got, want, name, f"{pl.axpby_kernel(K)}/{tag(torch, dtype)}")
        assert_dots(dots.cpu().numpy(), X, got, (name, "cheb"))
        x, y = device_block(torch, X, "colmajor", dtype), device_block(torch, Y0, "colmajor", dtype)
        z = device_block(torch, Z0, "interleaved", torch.complex128)
        dots = torch.full((2 * K,), float("nan"), dtype=torch.float64, device="cuda")
        pl.matvec_block_axpby_acc(x, y, al, be, ga, z, cz, dots=dots)
        got = y.cpu().numpy()
        close(got, want, name, f"{pl.acc_kernel(K)}/y/{tag(torch, dtype)}")
        assert_dots(dots.cpu().numpy(), X, got, (name, "evolve"))
        zwant = Z0 + cz * want
        err = np.abs(z.cpu().numpy() - zwant).max()
        print(f"ERR {name} {pl.acc_kernel(K)}/z/{tag(torch, dtype)} {err:.2e}")
        # Z0 + c want: the accumulate adds one rounding to the step's own (test_gpu_evolve.assert_acc)
        assert err <= 1e-12 * max(1.0, np.abs(Z0).max() + abs(cz) * np.abs(want).max()), (name, err)


# ---------------------------------------------------------------------------------------------
# d. partitions in one process
# ---------------------------------------------------------------------------------------------
def partitioned(torch, c, P, dtype, seed, path, kernel="tile", key_bytes=8, trials=1):
    parts, masks = c.partitions(P)
    assert np.array_equal(D.arrFromHashedToBlock(parts, masks).cpu().numpy().view(np.uint64), c.want_reps)
    pl = D.MatvecPlan(c.h, parts, dtype)
    assert pl.kernel == kernel, (path, pl.kernel)
    # the key (8-byte state, or the u32 index / rank of pre-indexed packets) + the value: what the VECTOR's type takes
    assert pl.key_bytes == key_bytes and pl.packet_bytes == key_bytes + (16 if dtype == torch.complex128 else 8), path
    got = None
    for trial in range(trials):
        x, want = c.vector(torch, dtype, seed + trial)
        xs = D.arrFromBlockToHashed(torch.from_numpy(x).cuda(), masks, P)
        ys = [torch.full_like(v, 3.0) for v in xs]
        pl.matvec(xs, ys)
        got = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
        close(got, want, c.name, f"{path}/{trial}/{tag(torch, dtype)}")
    pl.destroy()
    return got, want


def streams(c):
    """ls_amd_internal_streams_eligible: partitions of one process take the sorted streams (u32 global-rank keys, window consumers)
    when the basis has one weight and no flip and EVERY off-diagonal group is an exchange pair -- of any amplitude: dimer_14_7"""
    return c.name == "dimer_14_7"


@pytest.mark.parametrize("env", ["default", "LS_AMD_PACKETS=block", "LS_AMD_SCATTER_HASH=0"])
@pytest.mark.parametrize("name", ALL)
def test_three_partitions(torch, monkeypatch, name, env):
    """the per-wave packet rings (default), the block-wide packet lists, and the consumers' search without the hash table; packets
    carry the state (8-byte keys) unless the plan takes the streams, which setup_packet_index builds on the wave rings only"""
    c = case_of(torch, name)
    if env != "default":
        monkeypatch.setenv(*env.split("="))
    st = streams(c) and env != "LS_AMD_PACKETS=block"
    for dtype in c.dtypes:
        partitioned(torch, c, 3, dtype, 91, f"P=3/{env}", "tile+streams" if st else "tile", 4 if st else 8, trials=2)


@pytest.mark.parametrize("name", [n for n in FIXED_WEIGHT if n not in INVERSION])
def test_three_partitions_pre_indexed_packets(torch, monkeypatch, name):
    """LS_AMD_PACKET_INDEX=1: the producers read the u32 index at the destination off the all-destinations rank directory
    (setup_packet_index: one weight, <= 64 sites) -- for three- and four-bit flip masks and directed pairs too"""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_PACKET_INDEX", "1")
    monkeypatch.setenv("LS_AMD_PACKET_STREAMS", "0")
    for dtype in c.dtypes:
        partitioned(torch, c, 3, dtype, 93, "P=3/pre-indexed", "tile", 4, trials=2)


def test_sorted_streams_of_two_amplitudes(torch, monkeypatch):
    """dimer_14_7: exchange pairs of TWO amplitudes through the sorted streams -- both key forms, the three producers -- against
    the reference and against the atomic consumers"""
    c = case_of(torch, "dimer_14_7")
    settings = {"streams": {}, "atomics": {"LS_AMD_PACKET_STREAMS": "0"}, "index-keys": {"LS_AMD_STREAM_KEYS": "index"},
                "direct-producer": {"LS_AMD_STREAM_PRODUCER": "direct"}, "ring-producer": {"LS_AMD_STREAM_PRODUCER": "ring"},
                "direct-producer/index-keys": {"LS_AMD_STREAM_PRODUCER": "direct", "LS_AMD_STREAM_KEYS": "index"}}
    for dtype in c.dtypes:
        got = {}
        for label, env in settings.items():
            for k in PACKET_ENVS:
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            atomics = label == "atomics"
            got[label], want = partitioned(torch, c, 3, dtype, 95, f"P=3/{label}", "tile" if atomics else "tile+streams", 8 if atomics else 4,
                                           trials=2)
        for label in settings:  # (the bound of tests/test_gpu_matvec.py::test_sorted_packet_streams)
            assert np.abs(got[label] - got["atomics"]).max() <= 1e-13 * max(1.0, np.abs(want).max()), label


@pytest.mark.parametrize("name", ["tfim_12_x-1", "chiral_14_7_x-1", "jq_40_3"])
def test_eight_partitions(torch, name):
    c = case_of(torch, name)
    for dtype in c.dtypes:
        partitioned(torch, c, 8, dtype, 97, "P=8", trials=2)


# ---------------------------------------------------------------------------------------------
# e. replicated x
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HERMITIAN)
def test_replicated_x(torch, name):
    """one partition per process with the whole x replicated, every `rank` in turn on the one device (P = 3): k_direct over the
    global index, its partners looked up in the global x (plan_create_replicated_impl: FAMILY_REPL_DIRECT for every basis without
    permutations; hash partitions are not contiguous rows, so no staged kernel)"""
    c = case_of(torch, name)
    P = 3
    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    for dtype in c.dtypes:
        x, want = c.vector(torch, dtype, 60)
        xg = torch.from_numpy(x).cuda()
        ys = []
        for p in range(P):
            pl = D.ReplicatedPlan(c.h, parts[p], reps_global, dtype, P, p)
            assert pl.kernel.startswith("replicated-direct-pull"), pl.kernel
            y = torch.full((parts[p].numel(),), 3.0, dtype=dtype, device="cuda")
            pl.matvec(xg, y)
            ys.append(y)
            pl.destroy()
        close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, name, f"replicated-x/P={P}/{tag(torch, dtype)}")


@pytest.mark.parametrize("name", NON_HERMITIAN)
def test_replicated_x_needs_a_hermitian_operator(torch, name):
    c = case_of(torch, name)
    parts, masks = c.partitions(3)
    for dtype in c.dtypes:
        with pytest.raises(D.LsAmdError, match="replicated-x .pull. plans need a Hermitian operator"):
            D.ReplicatedPlan(c.h, parts[0], D.arrFromHashedToBlock(parts, masks), dtype, 3, 0)


def replicated_ranks(torch, c, dtype, path, P=3):
    """P ranks as threads over the loop-back transport, two matvecs (the first on another vector: stale blocks of the global buffer
    would show); returns the bytes of x every rank receives per matvec"""
    from distributed_matvec_amd.distributed import RcclReplicatedOperator
    from test_gpu_loopback import _run_ranks

    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    x, want = c.vector(torch, dtype, 23)
    other, _ = c.vector(torch, dtype, 24)
    xs = D.arrFromBlockToHashed(torch.from_numpy(x).cuda(), masks, P)
    others = D.arrFromBlockToHashed(torch.from_numpy(other).cuda(), masks, P)
    ys = [torch.full_like(v, -3.0) for v in xs]
    kernels, x_in = [None] * P, [None] * P

    def body(rank, comm):
        op = RcclReplicatedOperator(c.h, reps_global, masks, dtype, comm=comm)
        kernels[rank], x_in[rank] = op.engine.plan.kernel, op.x_bytes_in
        op.matvec(others[rank], ys[rank], check=True)
        op.matvec(xs[rank], ys[rank], check=True)
        op.rm.destroy()

    comms = _run_ranks(P, body)
    for comm in comms:
        comm.destroy()
    assert all(k.startswith("replicated-direct-pull") for k in kernels), kernels
    close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, c.name, f"{path}/{tag(torch, dtype)}")
    return x_in


def reach_of(c, P, shift=5, halo=1024):
    """what the sub-range exchange has to deliver, out of the REFERENCE matrix (csrc/dist.c setup_reach, host.c
    ls_amd_internal_plan_reach): rank p computes the global rows [n p / P, n (p + 1) / P) and reads the blocks of 2^shift rows that
    hold a column of a non-zero entry of those rows, and its own rows with `halo` = 1024 rows either side (REACH_HALO); it receives
    the elements of those blocks that other ranks own (x is owned by hash partition).  Per rank: (elements received, elements of the
    other ranks in all, runs of marked blocks)"""
    owner = c.partitions(P)[1].cpu().numpy()
    H, n = c.H.tocsr(), c.n
    out = []
    for p in range(P):
        n0, n1 = n * p // P, n * (p + 1) // P
        rows = H[n0:n1]
        marked = np.zeros(((n - 1) >> shift) + 1, dtype=bool)
        marked[np.unique(rows.indices[np.abs(rows.data) > 1e-12] >> shift)] = True  # (a rounding residue is no entry)
        marked[max(0, n0 - halo) >> shift : ((min(n, n1 + halo) - 1) >> shift) + 1] = True
        reached = np.repeat(marked, 1 << shift)[:n]
        runs = int((np.diff(np.concatenate([[0], marked.astype(int)])) == 1).sum())
        out.append((int((reached & (owner != p)).sum()), int((owner != p).sum()), runs))
    return out


# (the last: eight ranks, where the rows of a rank and their halo no longer span the 4096 states of xyz_12)
REACH_CASES = [("chiral_14_7", 3), ("jq_14_5", 3), ("jq_40_3", 3), ("xyz_12", 3), ("xyz_12", 8)]


@pytest.mark.parametrize("reach", ["-5", "0"])
@pytest.mark.parametrize("name,P", REACH_CASES, ids=[f"{n}-P{P}" for n, P in REACH_CASES])
def test_replicated_exchange_reach_blocks(torch, monkeypatch, name, P, reach):
    """lsk_reach_blocks marks the blocks of 32 rows (LS_AMD_REPL_REACH=-5) a rank's rows read from the ROW's coefficients while the
    kernel gathers by the partner's: three- and four-bit masks, complex coefficients, the identity index (xyz_12).  A block that is
    not marked never arrives, so a partner outside the reach reads the other vector's value; a block marked without need shows in
    the byte count, which is compared with reach_of(): equal where the marked blocks form at most 16 runs (dist.c keeps 16 intervals
    and closes the smallest gaps beyond that: then no less than the reach and no more than the vector).  Fewer bytes than the whole
    vector wherever the reach leaves something out -- every case but xyz_12 at three ranks: there the 1365 rows of a rank, 1024 rows
    either side and the partners across the top bonds cover all 128 blocks for EVERY rank (reach_of() says so from the reference
    matrix alone), the forced layout delivers the whole vector, and eight ranks take that part.  0: the whole vector travels."""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_REPL_REACH", reach)
    want = reach_of(c, P)
    assert (sum(r for r, _, _ in want) < sum(f for _, f, _ in want)) == ((name, P) != ("xyz_12", 3))
    for dtype in c.dtypes:
        x_in = replicated_ranks(torch, c, dtype, f"replicated-x/{P}-ranks/reach={reach}", P)
        es = 16 if dtype == torch.complex128 else 8
        full = [f * es for _, f, _ in want]
        print(f"REACH {name} P={P} {reach} {tag(torch, dtype)}: {x_in} of {full} bytes, reach_of {[r * es for r, _, _ in want]}")
        if reach == "0":
            assert x_in == full
            continue
        for got, (r, f, runs) in zip(x_in, want):
            assert (got == r * es) if runs <= 16 else (r * es <= got <= f * es), (x_in, want)
        if (name, P) != ("xyz_12", 3):  # (what tests/test_gpu_loopback.py asserts of a forced reach)
            assert all(a <= b for a, b in zip(x_in, full)) and sum(x_in) < sum(full), (x_in, full)


@pytest.mark.parametrize("name", ["tfim_12_x-1", "chiral_14_7_x-1"])
def test_replicated_exchange_flip_sectors(torch, name):
    """flip sectors canonicalise the partner first: no reach (ls_amd_internal_plan_reach does not apply), the same driver"""
    c = case_of(torch, name)
    for dtype in c.dtypes:
        replicated_ranks(torch, c, dtype, "replicated-x/3-ranks")


# ---------------------------------------------------------------------------------------------
# f. the CSR export applies the same matrix
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chiral_14_7", "twist_12"])
def test_csr_export_applies_the_same_matrix(torch, name):
    """Operator.to_csr (k_csr.hip over the cross-sector plan) tied to the same reference: a complex row, and a real non-Hermitian
    one -- its own matrix, not the transpose (max|H - H^T| of twist is 0.8)"""
    c = case_of(torch, name)
    csr = c.h.to_csr(c.reps)
    assert csr.dtype == (torch.float64 if c.is_real else torch.complex128)
    assert tuple(csr.shape) == (c.n, c.n) and csr.nnz > c.n
    x, want = c.vector(torch, csr.dtype, 95)
    got = (csr.to_dense() @ torch.from_numpy(x).cuda()).cpu().numpy()
    close(got, want, name, "to_csr")
    if not c.is_hermitian:
        assert np.abs(c.H.T @ x - want).max() > 1e-3  # (the transpose would not have passed)
