"""Unprojected fermionic bases -- spinless at fixed N, spinful at fixed N, the spinful (N_up, N_down) product basis -- on every
matvec path beyond one partition: hash partitions in one process (packets), replicated-x plans, and the two multi-rank drivers of
csrc/dist.c (packet exchange, replicated-x exchange with its sub-range reach) over the loop-back communicator.  The table is
tests/fermion_partition_cases.py (validated without a GPU by tests/test_fermion_partition_cases.py); every y is compared with
fermion_jw.sector_matrix, which shares no code with the library.

Tolerance: the project's rule, max|got - want| <= 1e-12 max(1, max|want|), on every path.  Every comparison prints its error first
(pytest -s shows `ERR case path value`).  Every plan asserts the kernel name -- and, where it makes packets, the key width -- that
host.c / dist.c decide for the row; the rule is quoted where it is asserted.  Replicated-x plans make no packets: no key width.

What would turn which assertion red:
  * a dropped Jordan-Wigner sign (a string mask off by one mode, the closing bond of a ring): every `close` of a row with strings
    -- all but the two open chains -- since the reference applies the signs mode by mode;
  * a wrong global index for the product basis (a searched index over 2 L-bit words of two weights): `close` in
    test_replicated_x and test_replicated_exchange for the PRODUCT rows, and the byte counts of test_replicated_exchange_reach
    (a block marked at a wrong index shows in x_bytes_in == reach_of());
  * an unmarked reach block: `close` in test_replicated_exchange_reach -- the block never arrives and the row reads the value of
    the OTHER vector sent first -- and x_bytes_in falls below reach_of();
  * y assigned where it must be accumulated: `close` of the NO_DIAGONAL rows, whose `want` is H x + y0 with a non-trivial y0."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from fermion_partition_cases import (ALL, COMPLEX, EXCHANGE_ONLY, FIXED_WEIGHT, HERMITIAN, NON_HERMITIAN, PRODUCT, ROWS, reach_of,
                                     reference_of, vectors)
from test_gpu_loopback import _run_ranks

pytestmark = pytest.mark.gpu

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
def default_settings(monkeypatch):
    """the kernel names and key widths asserted below are those of the default settings"""
    for k in PACKET_ENVS + ("LS_AMD_ROW_KERNEL", "LS_AMD_MODE", "LS_AMD_REPL_REACH", "LS_AMD_ROWS_PER_ROUND", "LS_AMD_CHAIN_WIDE",
                            "LS_AMD_CHAIN_RECORDS"):
        monkeypatch.delenv(k, raising=False)


class Case:
    """operator, basis, states and reference of one row of the table; built once per module"""

    def __init__(self, torch, name):
        self.name = name
        self.row = ROWS[name]
        self.n = self.row.n
        self.states, self.H = reference_of(name)
        self.basis, self.h = D.loadConfigFromDict(self.row.case.config(), hamiltonian=True)
        # an f64 vector too where the matrix is real
        self.dtypes = [torch.complex128] + ([torch.float64] if self.row.is_real else [])
        self.parts = {}

    def vector(self, torch, dtype, seed):
        """(x, y0, want): rows with a diagonal are ASSIGNED (y0 is garbage); rows without one accumulate: want = H x + y0"""
        x, y0 = vectors(self.name, dtype == torch.complex128, seed)
        return x, y0, self.H @ x + (0 if self.row.has_diagonal else y0)

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
    assert err <= 1e-12 * max(1.0, np.abs(want).max()), (case, path, err)


def hashed(torch, v, masks, P):
    return D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(v)).cuda(), masks, P)


def streams(name):
    """ls_amd_internal_streams_eligible: the sorted streams (u32 global-rank keys, window consumers) need one weight
    (hamming_weight >= 0: not the product basis) and EVERY off-diagonal group an exchange pair (classify_groups: a truth table on
    the two flipped bits alone, the same amplitude both ways).  A hop between adjacent modes has no string and is one; any other
    hop carries its string in the sign mask (support > 2 bits: generic), conjugate amplitudes differ both ways (generic) and a
    directed hop is LSK_GROUP_HOP_*.  Only the two open spinless chains are made of adjacent real hops alone."""
    return name in EXCHANGE_ONLY


def pre_indexable(name):
    """setup_packet_index: pre-indexed 4-byte packets need one weight h with 0 <= h < LSK_BINOM_K - 1 = 33 on <= 64 bits.  The
    product basis has none (hamming_weight == -1: h < 0) and spinless_ring_36_33 has h = 33: both carry 8-byte states."""
    return name in FIXED_WEIGHT and ROWS[name].case.N < 33


def test_the_rules_split_the_table_as_the_rows_are_meant_to():
    assert [n for n in ALL if streams(n)] == ["spinless_open_33_3", "spinless_open_16_8"]
    assert [n for n in ALL if not pre_indexable(n)] == ["spinless_ring_36_33"] + PRODUCT


# ---------------------------------------------------------------------------------------------
# the row of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_case_is_what_the_table_says(torch, name):
    c = case_of(torch, name)
    assert c.h.isReal == c.row.is_real and c.h.isHermitian == c.row.is_hermitian
    assert (c.h.numberDiagTerms() > 0) == c.row.has_diagonal
    assert not c.basis.requiresProjection() and not c.basis.hasPermutationSymmetries()
    for P in (1, 3, 8):  # bit for bit
        parts, masks = c.partitions(P)
        assert len(parts) == P and sum(int(p.numel()) for p in parts) == c.n
        assert np.array_equal(D.arrFromHashedToBlock(parts, masks).cpu().numpy().view(np.uint64), c.states), (name, P)


# ---------------------------------------------------------------------------------------------
# a. partitions in one process
# ---------------------------------------------------------------------------------------------
def partitioned(torch, c, P, dtype, seed, path, kernel, key_bytes, trials=2):
    parts, masks = c.partitions(P)
    pl = D.MatvecPlan(c.h, parts, dtype)
    assert pl.kernel == kernel, (c.name, path, pl.kernel)
    # the key (8-byte state, or the u32 index / rank of pre-indexed packets) + the value: what the VECTOR's type takes
    assert pl.key_bytes == key_bytes and pl.packet_bytes == key_bytes + (16 if dtype == torch.complex128 else 8), (c.name, path, pl.key_bytes)
    got = want = None
    for trial in range(trials):  # twice through the same plan
        x, y0, want = c.vector(torch, dtype, seed + trial)
        xs, ys = hashed(torch, x, masks, P), hashed(torch, y0, masks, P)
        pl.matvec(xs, ys)
        got = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
        close(got, want, c.name, f"{path}/{trial}/{tag(torch, dtype)}")
    pl.destroy()
    return got, want


@pytest.mark.parametrize("env", ["default", "LS_AMD_PACKETS=block", "LS_AMD_SCATTER_HASH=0"])
@pytest.mark.parametrize("name", ALL)
def test_three_partitions(torch, monkeypatch, name, env):
    """the per-wave packet rings (default), the block-wide packet lists, and the consumers' search without the hash table.
    setup_packet_index: with all partitions in one process (pl->me < 0) the packets carry the 8-byte state unless the plan takes
    the streams (streams_wanted), which it builds on the wave rings only (packets_wave_rings: not under LS_AMD_PACKETS=block);
    ls_amd_plan_kernel_name: `tile+streams` with them, `tile` without"""
    c = case_of(torch, name)
    if env != "default":
        monkeypatch.setenv(*env.split("="))
    st = streams(name) and env != "LS_AMD_PACKETS=block"
    for dtype in c.dtypes:
        partitioned(torch, c, 3, dtype, 91, f"P=3/{env}", "tile+streams" if st else "tile", 4 if st else 8)


@pytest.mark.parametrize("name", ALL)
def test_three_partitions_pre_indexed_packets(torch, monkeypatch, name):
    """LS_AMD_PACKET_INDEX=1 (LS_AMD_PACKET_STREAMS=0: streams_wanted says no): setup_packet_index builds the all-destinations rank
    directory for the fixed-weight rows (u32 index at the destination: 4-byte keys) and returns early for the product rows (h < 0)
    and for weight 33 (h >= LSK_BINOM_K - 1) -- those stay at 8-byte states, on the same wave rings, and must still be right"""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_PACKET_INDEX", "1")
    monkeypatch.setenv("LS_AMD_PACKET_STREAMS", "0")
    for dtype in c.dtypes:
        partitioned(torch, c, 3, dtype, 93, "P=3/pre-indexed", "tile", 4 if pre_indexable(name) else 8)


@pytest.mark.parametrize("name", ["spinless_long_40_3_complex", "hubbard_ring_8_4_4", "spinful_17_n3_flips"])
def test_eight_partitions(torch, name):
    """(none of the three is made of exchange pairs alone: streams_wanted says no, pl->me < 0: 8-byte states)"""
    c = case_of(torch, name)
    assert not streams(name)
    for dtype in c.dtypes:
        partitioned(torch, c, 8, dtype, 97, "P=8", "tile", 8)


@pytest.mark.parametrize("name", EXCHANGE_ONLY)
def test_sorted_streams_of_fermionic_chains(torch, monkeypatch, name):
    """the two open chains through the sorted streams -- both key forms (setup_packet_index: global-rank keys by default, the index
    at the destination under LS_AMD_STREAM_KEYS=index; 4 bytes either way), the three producers -- against the reference and
    against the atomic consumers (LS_AMD_PACKET_STREAMS=0: `tile`, 8-byte states)"""
    c = case_of(torch, name)
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
            got[label], want = partitioned(torch, c, 3, dtype, 95, f"P=3/{label}", "tile" if atomics else "tile+streams", 8 if atomics else 4)
        for label in settings:  # (the bound of tests/test_gpu_matvec.py::test_sorted_packet_streams)
            err = np.abs(got[label] - got["atomics"]).max()
            print(f"ERR {name} P=3/{label}-atomics/{tag(torch, dtype)} {err:.2e}")
            assert err <= 1e-13 * max(1.0, np.abs(want).max()), (name, label, err)


@pytest.mark.parametrize("name", COMPLEX)
def test_complex_coefficients_need_c128(torch, name):
    c = case_of(torch, name)
    assert c.dtypes == [torch.complex128]
    with pytest.raises(D.LsAmdError, match="needs dtype c128"):
        D.MatvecPlan(c.h, c.partitions(3)[0], torch.float64)


# ---------------------------------------------------------------------------------------------
# b. replicated-x plans, every rank in turn on the one device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HERMITIAN)
def test_replicated_x(torch, name):
    """one partition per process with the whole x replicated, every `rank` in turn (P = 3): k_direct over the global index
    (plan_create_replicated_impl: FAMILY_REPL_DIRECT for every basis without permutations).  The global index comes from
    plan_setup_part with global_index set: combinadic for one weight; for the product basis NOT the product index (`!pl->global_index`)
    but the searched one, and the rows find their global index through d_row_gidx.  A hash partition is not a contiguous block of
    the global rows, so chain_eligible is not even asked: never `+staged`."""
    c = case_of(torch, name)
    P = 3
    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    for dtype in c.dtypes:
        x, y0, want = c.vector(torch, dtype, 60)
        xg = torch.from_numpy(x).cuda()
        ys = hashed(torch, y0, masks, P)
        for p in range(P):
            pl = D.ReplicatedPlan(c.h, parts[p], reps_global, dtype, P, p)
            assert pl.kernel == "replicated-direct-pull", (name, p, pl.kernel)
            pl.matvec(xg, ys[p])
            pl.destroy()
        close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, name, f"replicated-x/P={P}/{tag(torch, dtype)}")


@pytest.mark.parametrize("name", NON_HERMITIAN)
def test_replicated_x_needs_a_hermitian_operator(torch, name):
    c = case_of(torch, name)
    parts, masks = c.partitions(3)
    for dtype in c.dtypes:
        with pytest.raises(D.LsAmdError, match="replicated-x .pull. plans need a Hermitian operator"):
            D.ReplicatedPlan(c.h, parts[0], D.arrFromHashedToBlock(parts, masks), dtype, 3, 0)


@pytest.mark.parametrize("name", COMPLEX)
def test_replicated_x_complex_coefficients_need_c128(torch, name):
    c = case_of(torch, name)
    parts, masks = c.partitions(3)
    with pytest.raises(D.LsAmdError, match="needs dtype c128"):
        D.ReplicatedPlan(c.h, parts[0], D.arrFromHashedToBlock(parts, masks), torch.float64, 3, 0)


# ---------------------------------------------------------------------------------------------
# c. multi-rank packet exchange over the loop-back communicator
# ---------------------------------------------------------------------------------------------
def packet_ranks(torch, c, P, dtype, rounds, path, kernel, key_bytes):
    """P ranks as threads, two checked matvecs through the same operator; returns (y in block order, want, bytes on the wire per
    matvec summed over the ranks)"""
    from distributed_matvec_amd.distributed import RcclDistributedOperator

    parts, masks = c.partitions(P)
    x, y0, want = c.vector(torch, dtype, 17)
    other, _, _ = c.vector(torch, dtype, 18)
    xs, others = hashed(torch, x, masks, P), hashed(torch, other, masks, P)
    ys, scratch = hashed(torch, y0, masks, P), hashed(torch, y0, masks, P)
    info, dots = [None] * P, [None] * P

    def body(rank, comm):
        op = RcclDistributedOperator(c.h, parts[rank], dtype, comm=comm, num_rounds=rounds)
        info[rank] = (op.engine.plan.kernel, op.engine.plan.key_bytes, op.num_rounds, op.exchange_bytes_per_matvec)
        op.matvec(others[rank], scratch[rank], check=True)  # double-buffered slots, cursors, staging buffers: used once already
        op.matvec(xs[rank], ys[rank], check=True)
        dots[rank] = complex(op.dot(xs[rank], xs[rank]).cpu().item())
        op.dm.destroy()

    for comm in _run_ranks(P, body):
        comm.destroy()
    assert all(k == kernel for k, _, _, _ in info), (c.name, path, info)
    assert all(b == key_bytes for _, b, _, _ in info), (c.name, path, info)
    # every rank runs the same number of rounds (dist_create_impl: what was asked for, or the all-reduced maximum of the local row
    # counts over the 2^24 rows of a round: one)
    assert len({r for _, _, r, _ in info}) == 1 and info[0][2] == (rounds if rounds else 1), (c.name, path, info)
    got = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
    close(got, want, c.name, f"{path}/{tag(torch, dtype)}")
    for d in dots:  # globalSumReal over the ranks
        assert abs(d - np.vdot(x, x)) < 1e-9, (c.name, path, d)
    return got, want, sum(b for _, _, _, b in info)


PACKET_CASES = [(name, 3) for name in ALL] + [("spinless_open_33_3", 8), ("hubbard_ring_8_4_4", 8)]


@pytest.mark.parametrize("rounds", [3, 0])
@pytest.mark.parametrize("name,P", PACKET_CASES, ids=[f"{n}-P{P}" for n, P in PACKET_CASES])
def test_packet_exchange(torch, monkeypatch, name, P, rounds):
    """ls_amd_dist_matvec, one partition per rank (pl->me >= 0): setup_packet_index builds the 4-byte pre-indexed packets by default
    where a closed form ranks the basis (pre_indexable) and leaves 8-byte states to the product basis and weight 33; dist.c asks for
    the streams (g_want_streams) and ls_amd_internal_streams_eligible grants them to the two open chains: `tile+streams`, `tile`
    elsewhere -- the non-Hermitian row included (packets push: no Hermiticity needed).  For the stream rows the same again with the
    atomic consumers (LS_AMD_PACKET_STREAMS=0: `tile`, still pre-indexed): the same y to 1e-13 and the same bytes on the wire."""
    c = case_of(torch, name)
    key = 4 if pre_indexable(name) else 8
    for dtype in c.dtypes:
        path = f"packets/{P}-ranks/rounds={rounds}"
        got, want, volume = packet_ranks(torch, c, P, dtype, rounds, path, "tile+streams" if streams(name) else "tile", key)
        assert volume > 0
        if streams(name):
            monkeypatch.setenv("LS_AMD_PACKET_STREAMS", "0")
            got0, _, volume0 = packet_ranks(torch, c, P, dtype, rounds, path + "/atomics", "tile", 4)
            monkeypatch.delenv("LS_AMD_PACKET_STREAMS")
            err = np.abs(got - got0).max()
            print(f"ERR {name} {path}/streams-atomics/{tag(torch, dtype)} {err:.2e}")
            assert err <= 1e-13 * max(1.0, np.abs(want).max()), (name, err)
            assert volume == volume0 > 0  # pre-indexed 12 / 20-byte packets either way; the own segment never travels


# ---------------------------------------------------------------------------------------------
# d. multi-rank replicated-x exchange over the loop-back communicator; e. its reach
# ---------------------------------------------------------------------------------------------
def replicated_kernel_of(name):
    """plan_create_replicated_impl: a rank's rows are a contiguous block of the global rows, so the staged chain kernel applies (with
    chain_row0 = the block's first row) where the global index is combinadic and chain_eligible holds: a real Hermitian operator
    with a diagonal, made of exchange runs plus at most two other EXCHANGE pairs.  The two open chains are one run and nothing
    else.  Every other spinless row has a generic group (a string, conjugate amplitudes), spinless_ring_64_2 has no diagonal
    either; the product rows have a searched index; the spinful fixed-N rows close their rings with strings."""
    return "replicated-direct-pull+staged" if name in EXCHANGE_ONLY else "replicated-direct-pull"


def replicated_ranks(torch, c, dtype, path, P=3, kernel=None):
    """P ranks as threads, two matvecs (the first on ANOTHER vector: stale blocks of the global buffer would show); returns the bytes
    of x every rank receives per matvec"""
    from distributed_matvec_amd.distributed import RcclReplicatedOperator

    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    x, y0, want = c.vector(torch, dtype, 23)
    other, _, _ = c.vector(torch, dtype, 24)
    xs, others = hashed(torch, x, masks, P), hashed(torch, other, masks, P)
    ys, scratch = hashed(torch, y0, masks, P), hashed(torch, y0, masks, P)
    kernels, x_in = [None] * P, [None] * P

    def body(rank, comm):
        op = RcclReplicatedOperator(c.h, reps_global, masks, dtype, comm=comm)
        kernels[rank], x_in[rank] = op.engine.plan.kernel, op.x_bytes_in
        op.matvec(others[rank], scratch[rank], check=True)
        op.matvec(xs[rank], ys[rank], check=True)
        op.rm.destroy()

    for comm in _run_ranks(P, body):
        comm.destroy()
    assert all(k == (kernel or replicated_kernel_of(c.name)) for k in kernels), (c.name, path, kernels)
    close(D.arrFromHashedToBlock(ys, masks).cpu().numpy(), want, c.name, f"{path}/{tag(torch, dtype)}")
    return x_in


@pytest.mark.parametrize("reach", ["default", "0"])
@pytest.mark.parametrize("name", HERMITIAN)
def test_replicated_exchange(torch, monkeypatch, name, reach):
    """ls_amd_repl_matvec on three ranks under the default LS_AMD_REPL_REACH (blocks of 2^14 rows: setup_reach applies its 80 % rule,
    the same for all ranks) and with 0 (the whole vector travels: exactly (n - n_local) elements arrive)"""
    c = case_of(torch, name)
    if reach != "default":
        monkeypatch.setenv("LS_AMD_REPL_REACH", reach)
    parts, _ = c.partitions(3)
    for dtype in c.dtypes:
        x_in = replicated_ranks(torch, c, dtype, f"replicated-x/3-ranks/reach={reach}")
        es = 16 if dtype == torch.complex128 else 8
        full = [(c.n - int(p.numel())) * es for p in parts]
        if reach == "0":
            assert x_in == full, (x_in, full)
        else:  # the 80 % rule decides, for all ranks alike (tests/test_gpu_loopback.py)
            assert x_in == full or all(a < b for a, b in zip(x_in, full)), (x_in, full)


ROW_KERNELS = [("spinless_open_33_3", "LS_AMD_CHAIN_WIDE=1", "replicated-direct-pull+staged"),
               ("spinless_open_33_3", "LS_AMD_ROW_KERNEL=generic", "replicated-direct-pull"),
               ("spinless_open_16_8", "LS_AMD_CHAIN_RECORDS=1", "replicated-direct-pull+staged"),
               ("spinless_open_16_8", "LS_AMD_ROW_KERNEL=generic", "replicated-direct-pull")]


@pytest.mark.parametrize("name,env,kernel", ROW_KERNELS, ids=[f"{n}-{e}" for n, e, _ in ROW_KERNELS])
def test_replicated_exchange_row_kernel_settings(torch, monkeypatch, name, env, kernel):
    """the staged rows of a rank (chain_row0 != 0) in their other forms: 64-bit ranks over 64-bit states (setup_chain:
    LS_AMD_CHAIN_WIDE=1 where the basis has more than 32 bits), per-row records instead of wave headers (setup_chain_headers -- which
    a block with chain_row0 != 0 takes anyway: the setting must change nothing), and k_direct on the same rows (chain_eligible:
    LS_AMD_ROW_KERNEL=generic)"""
    c = case_of(torch, name)
    monkeypatch.setenv(*env.split("="))
    for dtype in c.dtypes:
        replicated_ranks(torch, c, dtype, f"replicated-x/3-ranks/{env}", kernel=kernel)


@pytest.mark.parametrize("name", NON_HERMITIAN)
def test_replicated_exchange_refuses_a_non_hermitian_operator_on_every_rank(torch, name):
    """ls_amd_repl_create: the plan of every rank is refused (plan_create_replicated_impl) and the set-up's agreements let all of
    them return -- no rank waits in a collective (_run_ranks would say so)"""
    from distributed_matvec_amd.distributed import RcclReplicatedOperator

    c = case_of(torch, name)
    P = 3
    parts, masks = c.partitions(P)
    reps_global = D.arrFromHashedToBlock(parts, masks)
    for dtype in c.dtypes:
        messages = [None] * P

        def body(rank, comm):
            try:
                RcclReplicatedOperator(c.h, reps_global, masks, dtype, comm=comm)
            except D.LsAmdError as e:
                messages[rank] = str(e)

        for comm in _run_ranks(P, body):
            comm.destroy()
        for r, m in enumerate(messages):
            assert m is not None, f"rank {r} built a replicated-x operator of a non-Hermitian matrix"
            assert "replicated-x (pull) plans need a Hermitian operator" in m, (r, m)


REACH_CASES = [(name, 3) for name in HERMITIAN] + [("spinless_open_33_3", 8), ("hubbard_ring_17_2_2", 8),
                                                   ("hubbard_32_1_2_pair_hop", 8), ("spinless_open_16_8", 8)]


@pytest.mark.parametrize("name,P", REACH_CASES, ids=[f"{n}-P{P}" for n, P in REACH_CASES])
def test_replicated_exchange_reach(torch, monkeypatch, name, P):
    """LS_AMD_REPL_REACH=-5: lsk_reach_blocks marks the blocks of 32 rows a rank's rows read -- through the combinadic global index,
    or (product basis) its search_index branch -- and setup_reach forces the sub-range layout.  A block that is not marked never
    arrives, so a partner outside the reach reads the other vector's value; a block marked without need shows in the byte count,
    which is compared with reach_of() built from the REFERENCE matrix and the ownership masks: equal where the marked blocks form at
    most 16 runs (REACH_K; dist.c closes the smallest gaps beyond that: then no less than the reach and no more than the vector --
    hubbard_32_1_2_pair_hop's last rank, 24 and 28 runs).  Fewer bytes than the whole vector in every case
    (tests/test_fermion_partition_cases.py checks that from the reference alone)."""
    c = case_of(torch, name)
    monkeypatch.setenv("LS_AMD_REPL_REACH", "-5")
    want = reach_of(c.H, c.partitions(P)[1].cpu().numpy(), P)
    assert sum(r for r, _, _ in want) < sum(f for _, f, _ in want)
    assert (max(runs for _, _, runs in want) > 16) == (name == "hubbard_32_1_2_pair_hop")
    for dtype in c.dtypes:
        x_in = replicated_ranks(torch, c, dtype, f"replicated-x/{P}-ranks/reach=-5", P)
        es = 16 if dtype == torch.complex128 else 8
        full = [f * es for _, f, _ in want]
        print(f"REACH {name} P={P} {tag(torch, dtype)}: {x_in} of {full} bytes, reach_of {[r * es for r, _, _ in want]}")
        for got, (r, f, runs) in zip(x_in, want):
            assert (got == r * es) if runs <= 16 else (r * es <= got <= f * es), (x_in, want)
        assert all(a <= b for a, b in zip(x_in, full)) and sum(x_in) < sum(full), (x_in, full)
