"""Tile prologue of the staged chain kernels (k_chain_t, k_chain_pair_t; k_rows.hip: chain_rows).  A tile's LDS window is exactly four
16-byte loads per thread (2048 f64 rows, 1024 c128 elements, two windows of 1024 rows for a paired tile); an interior tile -- every row of
its windows inside x, x 16-byte aligned -- has them written straight into LDS with no bounds check, all requested before the one wait;
a tile at either end of x, or an unaligned x, keeps the checked loads.

Host: the windows as the kernels place them (ls_amd_test_chain_tile_windows calls the kernels' own function) over every tile of the
tile maps of small rings, on one and three partitions: "interior" means inside x, and every partner a row finds in LDS lies in the
window.  GPU: the default plan against the generic row kernel (k_direct shares no tile code), against per-row records (to the bit)
and against the unpaired plan, on shapes with nothing but edge tiles, odd window starts, several exchange runs, 64-bit states and
complex vectors; rows of a partition (first row != 0 in a longer x); an x that starts 8 bytes off the 16-byte grid."""
import ctypes as C
import os
from math import comb

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("LS_AMD_CHAIN_PAIRED", "LS_AMD_CHAIN_RECORDS", "LS_AMD_ROW_KERNEL", "LS_AMD_TILE_CHUNK", "LS_AMD_PAIR_TILE_CHUNK",
       "LS_AMD_CHAIN_PAIR_LEVELS")
MAX_LEVELS = 6
F64, C128, PAIRED = 0, 1, 2  # kinds of ls_amd_test_chain_tile_windows


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
    u64pp = C.POINTER(C.POINTER(C.c_uint64))
    lib.ls_amd_test_chain_tile_windows.restype = C.c_int
    lib.ls_amd_test_chain_tile_windows.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
    lib.ls_amd_test_tilemap_pair_levels.restype = C.c_int
    lib.ls_amd_test_tilemap_pair_levels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, u64pp, u64pp,
                                                    C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_int64)]
    lib.ls_amd_plan_chain_paired_rows.restype = C.c_int64
    lib.ls_amd_plan_chain_paired_rows.argtypes = [C.c_void_p]
    return lib


# ---------------------------------------------------------------------------------------------
# host: where the windows lie
# ---------------------------------------------------------------------------------------------
def _plain_tiles(lib, n, tile_rows):
    """(first row, rows) of every tile of the map of n rows"""
    ptr = C.POINTER(C.c_uint64)()
    slots = lib.ls_amd_test_tilemap(n, tile_rows, 256, C.byref(ptr))
    assert slots >= 0
    e = np.ctypeslib.as_array(ptr, shape=(8 * max(slots, 1),)).copy()
    lib.ls_amd_test_free(ptr)
    cnt = ((e >> np.uint64(48)) & np.uint64(0x7FF)).astype(np.int64)
    start = (e & np.uint64((1 << 48) - 1)).astype(np.int64)
    return [(int(s), int(c)) for s, c in zip(start[cnt > 0], cnt[cnt > 0])]


def _paired_tiles(lib, L, k, levels):
    """the two maps of the paired plan: (first row, rows) of the tiles of the one, (first row, rows between the segments) of the
    other; None when the basis has no whole paired segment"""
    rest, pairs, ranges = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int64)()
    out = (C.c_int64 * 4)()
    nr = lib.ls_amd_test_tilemap_pair_levels(L, k, 1024, 256, 256, levels, C.byref(rest), C.byref(pairs), C.byref(ranges), out)
    assert nr >= 0
    if nr == 0:
        return None
    r = np.ctypeslib.as_array(rest, shape=(8 * max(int(out[1]), 1),)).copy()
    p = np.ctypeslib.as_array(pairs, shape=(8 * max(int(out[2]), 1),)).copy()
    d = np.ctypeslib.as_array(ranges, shape=(nr, 6)).copy()[:, 4]
    for q in (rest, pairs, ranges):
        lib.ls_amd_test_free(q)
    r, p = r[(r >> np.uint64(48)) != 0], p[(p >> np.uint64(48)) != 0]
    plain = [(int(e & np.uint64((1 << 48) - 1)), int((e >> np.uint64(48)) & np.uint64(0x7FF))) for e in r]
    paired = [(int(e & np.uint64(0xFFFFFFFF)), int(d[int((e >> np.uint64(32)) & np.uint64(0xFFFF))])) for e in p]
    return plain, paired


def _windows(lib, kind, first, first_b, n_x):
    out = (C.c_int64 * 7)()
    interior = lib.ls_amd_test_chain_tile_windows(kind, first, first_b, n_x, out)
    assert interior in (0, 1)
    w0, w0b, rows, windows, core, halo, ldsp = (int(v) for v in out)
    return bool(interior), w0, w0b, rows, windows, core, halo, ldsp


def _partners(L, k):
    """partner[p][i] = row of state i with sites p, p + 1 exchanged (i itself where they hold the same bit), p = 0..11"""
    words = np.arange(1 << L, dtype=np.uint32)
    ones = np.zeros(1 << L, dtype=np.uint8)
    for b in range(L):
        ones += ((words >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    states = words[ones == k].astype(np.int64)  # ascending = the combinadic order
    assert len(states) == comb(L, k)
    out = []
    for p in range(12):
        anti = ((states >> p) ^ (states >> (p + 1))) & 1
        out.append(np.searchsorted(states, states ^ (anti * (3 << p))))
    return out


@pytest.mark.parametrize("L", [13, 14, 15, 16, 17])
def test_windows_of_every_tile(L):
    """every tile of both maps (and of the 512-row map of complex vectors), the whole basis and the rows of each of three partitions
    in the whole x: a window is four 16-byte loads per thread; "interior" is exactly "every row of every window lies in [0, n_x)";
    the tile's rows lie in the window, and so does every partner that a pair served from LDS leads to"""
    lib = _lib()
    k = L // 2
    n = comb(L, k)
    partner = _partners(L, k)
    seen = {"interior": 0, "edge": 0, "odd": 0, "paired": 0}

    def check(kind, first, first_b, rows_of_tile, n_x):
        interior, w0, w0b, rows, windows, core, halo, ldsp = _windows(lib, kind, first, first_b, n_x)
        elem = 16 if kind == C128 else 8
        assert windows * rows * elem == 4 * 256 * 16 and windows == (2 if kind == PAIRED else 1)
        assert ldsp == (12 if kind == F64 else 11) and halo > comb(ldsp - 1, (ldsp - 1) // 2) and rows == core + 2 * halo
        segments = [(first, w0)] + ([(first_b, w0b)] if kind == PAIRED else [])
        inside = True
        for f, w in segments:
            assert w % 2 == 0 and w in (f - halo, f - halo - 1)
            inside &= 0 <= w and w + rows <= n_x
            assert rows_of_tile <= core and w <= f and f + rows_of_tile <= w + rows
            for p in range(ldsp):
                reach = partner[p][f:f + rows_of_tile]
                assert w <= reach.min() and reach.max() < w + rows, (kind, f, p, int(reach.min()), int(reach.max()), w)
            seen["odd"] += (f - halo) % 2
        assert interior == inside, (kind, first, first_b, n_x, w0, w0b)
        if interior:  # what the unchecked loads read: [w, w + rows) of x, in 16-byte pieces from an even row on
            for _, w in segments:
                assert 0 <= w and w + rows <= n_x
        seen["interior" if interior else "edge"] += 1

    for P in (1, 3):
        for part in range(P):
            n0, n1 = n * part // P, n * (part + 1) // P
            for kind, tile_rows in ((F64, 1024), (C128, 512)):
                for start, cnt in _plain_tiles(lib, n1 - n0, tile_rows):
                    check(kind, n0 + start, 0, cnt, n)
    for levels in (1, MAX_LEVELS):
        maps = _paired_tiles(lib, L, k, levels)
        assert (maps is None) == (L < 14)
        if maps is None:
            continue
        for start, cnt in maps[0]:
            check(F64, start, 0, cnt, n)
        for start, d in maps[1]:
            check(PAIRED, start, start + d, 512, n)
            seen["paired"] += 1
    assert seen["edge"] > 0 and (seen["interior"] > 0 or n < 4096) and (seen["paired"] > 0 or L < 14), seen
    if L == 17:
        assert seen["odd"] > 0, seen


def test_a_basis_shorter_than_a_window_has_no_interior_tile():
    lib = _lib()
    n = comb(13, 6)
    assert n < 2048
    for start, cnt in _plain_tiles(lib, n, 1024):
        assert not _windows(lib, F64, start, 0, n)[0]
    assert lib.ls_amd_test_chain_tile_windows(3, 0, 0, n, (C.c_int64 * 7)()) == -1


def test_chain_kernels_keep_their_blocks_per_cu():
    """the staged kernels after the prologue: no scratch anywhere; the two of the headline <= 72 VGPRs with an SGPR count that admits 7
    blocks; static LDS = the window + its zero slot, 16 400 bytes at the most (it was 16 424 with the 2052-row windows), and with the launch-time
    image of 32 sites at half filling within 22.5 KB"""
    import shutil
    import sys

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    stats = kernel_resources.resources(source="k_rows.hip")
    chain = {k: v for k, v in stats.items() if k.startswith("_Z14k_chain_pair_t") or k.startswith("_Z9k_chain_tI")}
    assert len(chain) == 7, sorted(chain)
    image = 32 * 18 * 4 + 3840
    for name, v in chain.items():
        assert v["scratch"] == 0 and v["lds"] <= 16400, (name, v)
    headline = [v for k, v in chain.items() if k.startswith("_Z14k_chain_pair_t") or k.startswith("_Z9k_chain_tIjjLb0ELi1024ELb1E")]
    assert len(headline) == 2, sorted(chain)
    for v in headline:
        assert v["vgpr"] <= 72 and v["occ"] >= 7 and 800 // (-(-v["sgpr"] // 16) * 16 + 16) >= 7, v
        assert v["lds"] + image <= 22.5 * 1024 and (160 * 1024) // (v["lds"] + image) >= 7, v


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _config(L, weight, kind="ring", jz=1.0, drop=()):
    from distributed_matvec_amd import config

    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["hamming_weight"] = weight
    lattice = [[i, i + 1] for i in range(L - 1)] if kind == "open" else [[i, (i + 1) % L] for i in range(L)]
    lattice = [s for s in lattice if s[0] not in drop]
    for t in cfg["hamiltonian"]["terms"]:
        t["sites"] = lattice
        if jz != 1.0 and "σᶻ" in t["expression"]:
            t["expression"] = f"{jz} × " + t["expression"]
    return cfg


def _matvec(torch, cfg, x, offset=0):
    """y = H x on one partition; offset: x is handed over as a view `offset` elements into a larger tensor"""
    import distributed_matvec_amd as D

    lib = _lib()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    xs = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(x)).cuda(), masks, 1)
    if offset:
        big = torch.zeros(xs[0].numel() + offset, dtype=xs[0].dtype, device="cuda")
        big[offset:].copy_(xs[0])
        xs = [big[offset:]]
        assert xs[0].data_ptr() % 16 == (offset * xs[0].element_size()) % 16 and xs[0].is_contiguous()
    ys = [torch.zeros_like(v) for v in xs]
    pl = D.matrixVectorProduct(h, xs, ys, reps, mode="pull")
    y = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
    return y, pl.kernel, int(lib.ls_amd_plan_chain_paired_rows(pl.h))


# name: (sites, weight, ring / open, Jz, dropped bonds, complex x, rows on paired tiles expected)
SHAPES = {
    "ring13-w6": (13, 6, "ring", 1.0, (), False, False),        # 1716 rows: less than one window, every tile an edge tile
    "ring14-w7": (14, 7, "ring", 1.0, (), False, True),         # 3432 rows: the smallest paired plan
    "ring16-w8": (16, 8, "ring", 1.0, (), False, True),         # 12 870 rows
    "ring17-w8": (17, 8, "ring", 1.0, (), False, True),         # 24 310 rows: odd window starts; second windows near the end of x
    "ring20-w10": (20, 10, "ring", 1.0, (), False, True),       # 184 756 rows: four pairing levels
    "open20-w10": (20, 10, "open", 1.0, (), False, True),       # no cached pair
    "xxz20-w10": (20, 10, "ring", 0.35, (), False, True),       # Jz = 0.35: another diagonal
    "ring20-w10-drop7": (20, 10, "ring", 1.0, (7,), False, True),  # bond (7, 8) missing: several exchange runs, the generic run loop
    "open33-w3": (33, 3, "open", 1.0, (), False, False),        # 5456 rows: 64-bit states, 32-bit ranks
    "ring16-w8-c128": (16, 8, "ring", 1.0, (), True, False),    # complex x: 512-row tiles, windows of 1024 elements
}


def _vector(n, seed, cplx):
    rs = np.random.RandomState(seed)
    x = rs.rand(n) - 0.5
    return x + 1j * (rs.rand(n) - 0.5) if cplx else x


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_default_plan_matches_generic_records_and_unpaired(torch, monkeypatch, shape):
    """the default plan, element by element: against the generic row kernel and against the unpaired plan at 1e-12 max|y| (the
    tolerance of test_chain_paired.py), against the plan on per-row records to the bit"""
    L, weight, kind, jz, drop, cplx, paired = SHAPES[shape]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(L, weight, kind, jz, drop)
    n = comb(L, weight)
    x = _vector(n, 1000 * L + weight, cplx)

    def run(**env):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        out = _matvec(torch, cfg, x)
        for key in env:
            monkeypatch.delenv(key)
        return out

    y, kernel, rows = run()
    assert kernel == "direct-pull+staged" and (rows > 0) == paired, (kernel, rows)
    y_gen, kernel_gen, rows_gen = run(LS_AMD_ROW_KERNEL="generic")
    assert kernel_gen == "direct-pull" and rows_gen == 0
    y_rec, kernel_rec, rows_rec = run(LS_AMD_CHAIN_RECORDS="1")
    assert kernel_rec == kernel and rows_rec == rows
    y_un, kernel_un, rows_un = run(LS_AMD_CHAIN_PAIRED="0")
    assert kernel_un == kernel and rows_un == 0

    scale = np.abs(y_gen).max()
    tol = 1e-12 * scale
    for name, other in (("generic", y_gen), ("unpaired", y_un)):
        err = np.abs(y - other).max()
        print(f"{shape}: default ({rows} rows on paired tiles) against {name}: max|dy| = {err:.3e}, max|y| = {scale:.3e}")
        assert err <= tol, (shape, name, err, int(np.abs(y - other).argmax()))
    assert y.tobytes() == y_rec.tobytes(), (shape, np.abs(y - y_rec).max())


@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("P", [2, 3])
def test_rows_of_a_partition_in_the_whole_x(torch, monkeypatch, P, cplx):
    """ring16-w8, the rows [n p / P, n (p + 1) / P) of each partition against the whole x (the staged kernel with a first row != 0
    and an x longer than its rows: the first and the last tiles of a partition are interior now, the ends of x are not)"""
    import distributed_matvec_amd as D

    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(16, 8)
    n = comb(16, 8)
    x = _vector(n, 77, cplx)
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, kernel_gen, _ = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_ROW_KERNEL")
    assert kernel_gen == "direct-pull"
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    reps_global = D.arrFromHashedToBlock(reps, masks)
    xg = torch.from_numpy(x).cuda()
    dtype = torch.complex128 if cplx else torch.float64
    parts = []
    for p in range(P):
        n0, n1 = n * p // P, n * (p + 1) // P
        pl = D.ReplicatedPlan(h, reps_global[n0:n1], reps_global, dtype, P, p)
        assert pl.kernel == "replicated-direct-pull+staged", pl.kernel
        y = torch.full((n1 - n0,), 3.0, dtype=dtype, device="cuda")
        pl.matvec(xg, y)
        parts.append(y.cpu().numpy())
        pl.destroy()
    y = np.concatenate(parts)
    err = np.abs(y - y_gen).max()
    print(f"ring16-w8 over {P} partitions ({'c128' if cplx else 'f64'}): max|dy| = {err:.3e}, max|y| = {np.abs(y_gen).max():.3e}")
    assert err <= 1e-12 * np.abs(y_gen).max(), (P, err, int(np.abs(y - y_gen).argmax()))


@pytest.mark.gpu
def test_x_off_the_16_byte_grid_takes_the_checked_loads(torch, monkeypatch):
    """ring16-w8 with x a view one element into a larger tensor (8-byte aligned): no tile is interior; the same y to the bit as from
    the aligned x, where most are"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(16, 8)
    x = _vector(comb(16, 8), 78, False)
    y, kernel, rows = _matvec(torch, cfg, x)
    y_off, kernel_off, rows_off = _matvec(torch, cfg, x, offset=1)
    assert kernel == kernel_off == "direct-pull+staged" and rows == rows_off > 0
    assert y.tobytes() == y_off.tobytes(), np.abs(y - y_off).max()
