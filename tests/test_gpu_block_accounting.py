"""What one call of a block step on a matvec plan records: the matvec counter and the call count of every stage
(MatvecPlan.stage_times), for matvec_block, matvec_block_axpby and matvec_block_axpby_acc (fused and split) on the three host
paths -- the direct kernel, the cached-then-chunked pull loop, the column loop.  The value tests of test_gpu_block_matvec.py,
test_gpu_kpm.py and test_gpu_evolve.py do not see these numbers.

The table below is read off csrc/host.c, not off a run:
  direct   one launch under ST_ROWS ("rowKernel"), counted as one matvec;
  pull     one gather launch under ST_ROWS over the rows a valid slot cache covers (if any), then per chunk of blk_rows rows one
           resolve under ST_GENERATE ("producers") and one gather under ST_ROWS; counted as one matvec;
  columns  K calls of ls_amd_matvec, which counts and records its stages itself: K times what one single-vector matvec records.
The split accumulate step is the Chebyshev step and one k_axpby_acc pass outside every stage: it records what the Chebyshev step does.

blk_rows is what block_pbuf() fixes at the plan's first projected block call: the whole 256-row tiles LS_AMD_BLOCK_RESOLVE_BYTES
leave room for, at 64 rows per stream and cap * (4 + 1 + 8 * coefficient doubles) + 4 bytes per stream, cap = 64 x the number of
flip masks of the operator.  Neither cap nor the coefficient kind can be asked of a plan from Python, so the chunk count of the
Heisenberg chain below is written down (24 bonds, 24 flip masks; one uniform coefficient, no doubles: 7684 bytes per stream, 32
streams in 256 KiB, blk_rows = 2048) and the test asks, besides, that it is the same for the three steps and at least three."""
import numpy as np
import pytest

import distributed_matvec_amd as D
from helpers import model_config

pytestmark = pytest.mark.gpu

STAGES = ("localDiagonal", "hashRefresh", "rowKernel", "producers", "exchangeWait", "consumers", "resultsToOwners")
RESOLVE_BYTES = 1 << 18
BLK_ROWS = ((RESOLVE_BYTES // (64 * 24 * (4 + 1) + 4)) & ~3) * 64
STEPS = ["plain", "cheb", "acc_fused", "acc_split"]
PATHS = {"direct": ("heisenberg_chain_16", "kernel"), "pull": ("heisenberg_chain_24_symm", "kernel"),
         "columns": ("heisenberg_chain_24_symm", "columns")}
KERNELS = {"direct": ("k_direct_blk", "k_direct_cheb", "k_direct_evolve", "k_direct_cheb+k_axpby_acc"),
           "pull": ("k_pull_gather_blk", "k_pull_gather_cheb", "k_pull_gather_evolve", "k_pull_gather_cheb+k_axpby_acc"),
           "columns": ("columns", "epilogue", "epilogue", "epilogue")}


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


_plans = {}


def plan_of(torch, model):
    """(plan, n, rows of the slot cache, what one single-vector matvec records); heisenberg_chain_24_symm with half its packet
    streams cached and the cache valid"""
    if model not in _plans:
        basis, h = D.loadConfigFromDict(model_config(model), hamiltonian=True)
        reps, _ = D.enumerateStates(basis, 1)
        n = reps[0].numel()
        pl = D.MatvecPlan(h, reps, torch.float64)
        cached = 0
        x = torch.ones(n, dtype=torch.float64, device="cuda")
        if model == "heisenberg_chain_24_symm":
            probe = D.MatvecPlan(h, reps, torch.float64)
            assert probe.cache_slots(0) == n
            cached = pl.cache_slots(probe.slot_cache[1] // 2)
            probe.destroy()
            assert 0 < cached < n and cached % 256 == 0, (cached, n)
            pl.matvec([x], [torch.zeros_like(x)])  # the first matvec resolves the cached streams
            assert pl.slot_cache[0] == cached
        pl.enable_stage_timing(1024)
        pl.matvec([x], [torch.zeros_like(x)])
        single = pl.stage_times()
        assert single[1] == 1 and single[0]["rowKernel"][1] == 1 and single[0]["producers"][1] == 0, single
        _plans[model] = (pl, n, cached, {s: single[0][s][1] for s in STAGES})
    return _plans[model]


def expected(path, K, n, cached, single):
    """(matvecs, {stage: calls}) of one call"""
    calls = dict.fromkeys(STAGES, 0)
    if path == "direct":
        calls["rowKernel"] = 1
        return 1, calls
    if path == "pull":
        chunks = -(-(n - cached) // BLK_ROWS)
        assert chunks >= 3, (n, cached, BLK_ROWS)
        calls["rowKernel"] = (cached > 0) + chunks
        calls["producers"] = chunks
        return 1, calls
    return K, {s: K * single[s] for s in STAGES}


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_one_call_records_what_the_host_path_launches(torch, monkeypatch, path, step, K):
    model, mode = PATHS[path]
    monkeypatch.setenv("LS_AMD_BLOCK", mode)
    monkeypatch.setenv("LS_AMD_BLOCK_RESOLVE_BYTES", str(RESOLVE_BYTES))
    monkeypatch.setenv("LS_AMD_ACC", "split" if step == "acc_split" else "fused")
    pl, n, cached, single = plan_of(torch, model)
    names = (pl.block_kernel(K), pl.axpby_kernel(K), pl.acc_kernel(K))
    assert names == KERNELS[path][:2] + (KERNELS[path][3 if step == "acc_split" else 2],), names
    rs = np.random.RandomState(7 + K)
    x = torch.from_numpy(rs.rand(n, K) - 0.5).cuda()
    y = torch.from_numpy(rs.rand(n, K) - 0.5).cuda()
    z = torch.zeros((n, K), dtype=torch.float64, device="cuda")
    dots = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
    kernel, cache = pl.kernel, pl.slot_cache
    before, mv0 = pl.stage_times()
    if step == "plain":
        pl.matvec_block(x, y)
    elif step == "cheb":
        pl.matvec_block_axpby(x, y, 0.5, -0.25, -1.0, dots=dots)
    else:
        pl.matvec_block_axpby_acc(x, y, 0.5, -0.25, -1.0, z, 0.75, dots=dots)
    after, mv1 = pl.stage_times()
    got = {s: after[s][1] - before[s][1] for s in STAGES}
    want_mv, want = expected(path, K, n, cached, single)
    print(f"accounting {path}/{step}/K={K}: n={n} cached={cached} matvecs={mv1 - mv0} calls={got}")
    assert mv1 - mv0 == want_mv, (path, step, K, mv1 - mv0, want_mv)
    assert got == want, (path, step, K, got, want)
    assert pl.kernel == kernel and pl.slot_cache == cache
