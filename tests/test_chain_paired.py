"""Paired tiles of the staged chain kernel (k_chain_pair_t): a block works on 512 rows whose two top site bits are 01 and on their
512 partners across the top bond (bits 10), and reads that bond's term from its own LDS window.  Every shape is run three times --
the default plan, the same plan under LS_AMD_CHAIN_PAIRED=0 (k_chain_t alone) and the generic row kernel (k_direct, which shares no
tile code).  The tile maps of the two launches are checked on the host: every row exactly once."""
import ctypes as C
import os
from math import comb

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("LS_AMD_CHAIN_PAIRED", "LS_AMD_CHAIN_RECORDS", "LS_AMD_ROW_KERNEL", "LS_AMD_TILE_CHUNK")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    if not t.cuda.is_available():
        pytest.fail("GPU tests need a HIP device (the product has no CPU fallback)")
    t.cuda.set_device(0)
    return t


def _lib():
    from distributed_matvec_amd import _lib as L

    lib = L.load()
    lib.ls_amd_plan_chain_paired_rows.restype = C.c_int64
    lib.ls_amd_plan_chain_paired_rows.argtypes = [C.c_void_p]
    lib.ls_amd_test_tilemap_paired.restype = C.c_int
    lib.ls_amd_test_tilemap_paired.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.POINTER(C.c_uint64)),
                                               C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_int64)]
    return lib


def _pair_range(L, k):
    """[a0, a1) = the whole 512-row segments of R01 = [C(L-2, k), C(L-1, k)), d = C(L-2, k-1) rows to the partner"""
    r01, r10 = comb(L - 2, k), comb(L - 1, k)
    a0, a1 = -(-r01 // 512) * 512, r10 // 512 * 512
    return a0, a1, r10 - r01


def _config(L, weight, kind="ring", jz=1.0):
    from distributed_matvec_amd import config

    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["hamming_weight"] = weight
    lattice = [[i, i + 1] for i in range(L - 1)] if kind == "open" else [[i, (i + 1) % L] for i in range(L)]
    for t in cfg["hamiltonian"]["terms"]:
        t["sites"] = lattice
        if jz != 1.0 and "σᶻ" in t["expression"]:
            t["expression"] = f"{jz} × " + t["expression"]
    return cfg


def _matvec(torch, cfg, x):
    import distributed_matvec_amd as D

    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    xs = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(x)).cuda(), masks, 1)
    ys = [torch.zeros_like(v) for v in xs]
    pl = D.matrixVectorProduct(h, xs, ys, reps, mode="pull")
    y = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
    return y, pl.kernel, int(_lib().ls_amd_plan_chain_paired_rows(pl.h))


def _matvec_two_partitions(torch, cfg, x):
    """the two halves of the rows as replicated-x plans: the staged kernel on a slice of the global rows (row0 != 0 in the second)"""
    import distributed_matvec_amd as D

    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    xg = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    n = len(x)
    pieces, kernels, paired = [], set(), 0
    for p in range(2):
        n0, n1 = n * p // 2, n * (p + 1) // 2
        pl = D.ReplicatedPlan(h, reps[0][n0:n1], reps[0], xg.dtype, 2, p)
        y = torch.zeros(n1 - n0, dtype=xg.dtype, device="cuda")
        pl.matvec(xg, y)
        pieces.append(y)
        kernels.add(pl.kernel)
        paired += int(_lib().ls_amd_plan_chain_paired_rows(pl.h))
    assert len(kernels) == 1, kernels
    return torch.cat(pieces).cpu().numpy(), kernels.pop(), paired


# name: (sites, weight, ring / open, Jz)
SHAPES = {
    "ring16-w8": (16, 8, "ring", 1.0),    # 12 870 rows, R01 = R10 = 3 432: whole segments, both ragged ends of R01, both off-grid pieces of R10
    "ring16-w5": (16, 5, "ring", 1.0),    # R01 = 2002, d = 1001: other residues mod 64 and mod 512
    "ring16-w11": (16, 11, "ring", 1.0),  # R01 = 364, d = 1001: the second segment's window starts at an odd row
    "ring14-w7": (14, 7, "ring", 1.0),    # d = 924: one paired tile plus edges
    "ring13-w6": (13, 6, "ring", 1.0),    # d = 462: no whole segment, the plan stays unpaired
    "ring20-w10": (20, 10, "ring", 1.0),  # 184 756 rows: many paired tiles per XCD list
    "open16-w8": (16, 8, "open", 1.0),    # no cached pair
    "xxz16-w8": (16, 8, "ring", 0.35),    # Jz != J: another diagonal
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_paired_matches_unpaired_and_generic_kernel(torch, monkeypatch, shape):
    L, weight, kind, jz = SHAPES[shape]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(L, weight, kind, jz)
    n = comb(L, weight)
    x = np.random.RandomState(1000 * L + weight).rand(n) - 0.5
    a0, a1, d = _pair_range(L, weight)
    want_rows = 2 * (a1 - a0) if L >= 14 and a1 > a0 else 0
    assert (want_rows == 0) == (shape == "ring13-w6")

    y, kernel, paired = _matvec(torch, cfg, x)
    assert kernel == "direct-pull+staged" and paired == want_rows, (kernel, paired, want_rows)

    monkeypatch.setenv("LS_AMD_CHAIN_PAIRED", "0")
    y_un, kernel_un, paired_un = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_CHAIN_PAIRED")
    assert kernel_un == "direct-pull+staged" and paired_un == 0, (kernel_un, paired_un)

    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, kernel_gen, paired_gen = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_ROW_KERNEL")
    assert kernel_gen == "direct-pull" and paired_gen == 0, (kernel_gen, paired_gen)

    scale = np.abs(y_gen).max()
    e_un, e_gen = np.abs(y - y_un).max(), np.abs(y - y_gen).max()
    print(f"{shape}: paired rows {paired} of {n}, max|y - y_unpaired| = {e_un:.3e}, max|y - y_generic| = {e_gen:.3e}, max|y| = {scale:.3e}")
    # the tolerance of the chain kernel's parity tests (test_gpu_chain_wave_headers.py), element by element
    assert e_un <= 1e-12 * scale, (shape, e_un, int(np.abs(y - y_un).argmax()))
    assert e_gen <= 1e-12 * scale, (shape, e_gen, int(np.abs(y - y_gen).argmax()))
    if want_rows == 0:
        assert y.tobytes() == y_un.tobytes()
    # the records switch leaves the pairing alone (the second segments' headers then say "records" too): the same y to the bit
    monkeypatch.setenv("LS_AMD_CHAIN_RECORDS", "1")
    y_rec, kernel_rec, paired_rec = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_CHAIN_RECORDS")
    assert kernel_rec == "direct-pull+staged" and paired_rec == want_rows, (kernel_rec, paired_rec)
    assert y.tobytes() == y_rec.tobytes(), (shape, np.abs(y - y_rec).max())


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["0", "3"])
def test_paired_under_other_tile_orders(torch, monkeypatch, chunk):
    """LS_AMD_TILE_CHUNK deals both tile maps: contiguous eighths and chunks of three tiles"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(16, 8)
    n = comb(16, 8)
    x = np.random.RandomState(5).rand(n) - 0.5
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, _, _ = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_ROW_KERNEL")
    monkeypatch.setenv("LS_AMD_TILE_CHUNK", chunk)
    y, kernel, paired = _matvec(torch, cfg, x)
    assert kernel == "direct-pull+staged" and paired == 2 * 6 * 512, (kernel, paired)
    assert np.abs(y - y_gen).max() <= 1e-12 * np.abs(y_gen).max()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["inversion", "c128", "two-partitions"])
def test_plans_the_pairing_does_not_serve_stay_as_they_are(torch, monkeypatch, case):
    """an inversion sector (two cached pairs), complex vectors and a partitioned plan run without the paired launch, and y is bit for bit what LS_AMD_CHAIN_PAIRED=0 gives.  The partitioned plans are the two halves of the rows as
    replicated-x plans: those run the chain kernel (on a slice of the rows, row0 != 0 in the second) and add in a fixed order; hash
    partitions go through packets and atomics, where two runs of one build already differ in the last bit."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(16, 8)
    P = 1
    n = comb(16, 8)
    if case == "inversion":
        cfg["basis"]["spin_inversion"] = 1
        n = comb(15, 8)
    if case == "two-partitions":
        P = 2
    rs = np.random.RandomState(11)
    x = rs.rand(n) - 0.5
    if case == "c128":
        x = x + 1j * (rs.rand(n) - 0.5)
    run = _matvec_two_partitions if P == 2 else _matvec
    y, kernel, paired = run(torch, cfg, x)
    assert paired == 0, (case, kernel, paired)
    assert kernel == ("replicated-direct-pull+staged" if P == 2 else "direct-pull+staged"), kernel
    monkeypatch.setenv("LS_AMD_CHAIN_PAIRED", "0")
    y_un, kernel_un, paired_un = run(torch, cfg, x)
    assert kernel_un == kernel and paired_un == 0
    assert y.tobytes() == y_un.tobytes(), (case, np.abs(y - y_un).max())


def _tilemaps(lib, L, k, tile, chunk):
    rest, pairs = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    out = (C.c_int64 * 6)()
    rc = lib.ls_amd_test_tilemap_paired(L, k, tile, chunk, C.byref(rest), C.byref(pairs), out)
    assert rc >= 0
    if rc == 0:
        return None
    n, a0, a1, d, rest_slots, pair_slots = (int(v) for v in out)
    r = np.ctypeslib.as_array(rest, shape=(8 * max(rest_slots, 1),)).copy()
    p = np.ctypeslib.as_array(pairs, shape=(8 * max(pair_slots, 1),)).copy()
    lib.ls_amd_test_free(rest)
    lib.ls_amd_test_free(pairs)
    return n, a0, a1, d, r.reshape(8, -1), p.reshape(8, -1)


@pytest.mark.parametrize("chunk", [256, 3, 0])
def test_paired_tile_maps_write_every_row_exactly_once(chunk):
    """host only: over L = 13..24 and every weight, the tiles of the two launches cover [0, n) exactly once; paired tiles are whole
    and 512-aligned; a tile of the other map is flagged (bit 63: run on the records) exactly when it starts or ends off the 64-row
    grid of the wave headers, and one that starts off it ends on it"""
    lib = _lib()
    MASK48 = np.uint64(0xFFFFFFFFFFFF)
    seen_paired = 0
    for L in range(13, 25):
        for k in range(1, L):
            got = _tilemaps(lib, L, k, 1024, chunk)
            a0, a1, d = _pair_range(L, k)
            if got is None:
                assert L < 14 or a1 <= a0, (L, k)
                continue
            seen_paired += 1
            n, g0, g1, gd, rest, pairs = got
            assert (n, g0, g1, gd) == (comb(L, k), a0, a1, d) and L >= 14 and a1 > a0 and a0 % 512 == 0 and a1 % 512 == 0
            assert comb(L - 2, k) <= a0 and a1 + d <= comb(L - 1, k) + d <= n
            cover = np.zeros(n + 1, dtype=np.int32)  # difference array
            r = rest.ravel()
            r = r[(r >> np.uint64(48)) != 0]
            start = (r & MASK48).astype(np.int64)
            cnt = ((r >> np.uint64(48)) & np.uint64(0x7FF)).astype(np.int64)
            plain = (r >> np.uint64(63)).astype(bool)
            assert ((r >> np.uint64(59)) & np.uint64(0xF)).max() == 0  # no other flag
            assert cnt.min() >= 1 and cnt.max() <= 1024
            end = start + cnt
            assert np.array_equal(plain, (start % 64 != 0) | ((end % 64 != 0) & (end != n))), (L, k)
            off = start % 64 != 0
            assert np.all((end[off] % 64 == 0) | (end[off] == n)), (L, k)
            assert np.all(start // 1024 == (end - 1) // 1024)  # no tile crosses a multiple of the tile size
            np.add.at(cover, start, 1)
            np.add.at(cover, end, -1)
            p = pairs.ravel()
            p = p[(p >> np.uint64(48)) != 0]
            i0 = (p & MASK48).astype(np.int64)
            assert np.all((p >> np.uint64(48)) == 1024) and np.all(i0 % 512 == 0)
            assert np.array_equal(np.sort(i0), np.arange(a0, a1, 512))
            for s in (i0, i0 + d):
                np.add.at(cover, s, 1)
                np.add.at(cover, s + 512, -1)
            assert np.all(np.cumsum(cover)[:n] == 1), (L, k)
            if chunk > 0:  # chunks of consecutive tiles go round the XCD lists
                order = np.sort(i0)
                for q, row in enumerate(order):
                    xcd, slot = divmod(int(np.flatnonzero((pairs.ravel() & MASK48) == row)[0]), pairs.shape[1])
                    assert xcd == (q // chunk) % 8
                    if q >= 64:
                        break
    assert seen_paired > 100


def test_paired_kernel_keeps_seven_blocks_per_cu():
    """k_chain_pair_t next to the headline instantiation of k_chain_t: <= 72 VGPRs, the SGPR file admits 7 blocks, no scratch, and the
    window + the launch-time image (binomials of 32 sites at half filling + the near-pair table) stay within 22.5 KB"""
    import shutil
    import sys

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    stats = kernel_resources.resources(source="k_rows.hip")
    pair = [v for k, v in stats.items() if k.startswith("_Z14k_chain_pair_t")]
    assert len(pair) == 1, sorted(stats)
    v = pair[0]
    image = 32 * 18 * 4 + 3840
    assert v["scratch"] == 0 and v["vgpr"] <= 72 and v["occ"] >= 7, v
    assert 800 // (-(-v["sgpr"] // 16) * 16 + 16) >= 7, v
    assert v["lds"] + image <= 22.5 * 1024 and (160 * 1024) // (v["lds"] + image) >= 7, v
