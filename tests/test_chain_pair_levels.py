"""Pairing levels of the staged chain kernel (k_chain_pair_t).  The top site bits read as disjoint pairs (L-1, L-2), (L-3, L-4), ... are
levels 1, 2, ...; a row is paired across bond b = L - 2 level of the first level, from the top, whose two bits differ, and reads that
bond's term from the LDS window of its tile's other segment.  Host only: the range table against its closed form, the two tile maps
(every row exactly once), the involution on enumerated states.  GPU: the default plan against LS_AMD_CHAIN_PAIR_LEVELS=1 and 6,
LS_AMD_CHAIN_PAIRED=0 and the generic row kernel (k_direct, which shares no tile code)."""
import ctypes as C
from math import comb

import numpy as np
import pytest

ENV = ("LS_AMD_CHAIN_PAIRED", "LS_AMD_CHAIN_RECORDS", "LS_AMD_ROW_KERNEL", "LS_AMD_TILE_CHUNK", "LS_AMD_PAIR_TILE_CHUNK",
       "LS_AMD_CHAIN_PAIR_LEVELS")
MAX_LEVELS = 6


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
    lib.ls_amd_plan_chain_paired_rows.restype = C.c_int64
    lib.ls_amd_plan_chain_paired_rows.argtypes = [C.c_void_p]
    lib.ls_amd_plan_chain_paired_rows_at.restype = C.c_int64
    lib.ls_amd_plan_chain_paired_rows_at.argtypes = [C.c_void_p, C.c_int]
    lib.ls_amd_plan_chain_pair_levels.restype = C.c_int
    lib.ls_amd_plan_chain_pair_levels.argtypes = [C.c_void_p]
    lib.ls_amd_test_tilemap_paired.restype = C.c_int
    lib.ls_amd_test_tilemap_paired.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, u64pp, u64pp, C.POINTER(C.c_int64)]
    lib.ls_amd_test_tilemap_pair_levels.restype = C.c_int
    lib.ls_amd_test_tilemap_pair_levels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, u64pp, u64pp,
                                                    C.POINTER(C.POINTER(C.c_int64)), C.POINTER(C.c_int64)]
    return lib


def closed_form(L, k, levels, bonds=None):
    """The ranges of whole 512-row segments, written from the combinadic rank alone: rank(word) = sum over its set bits, the j-th from
    below at site p, of C(p, j).  Rows [a0, a1) have the level's pair at 01, rows + d have it at 10.  (level, bond, a0, a1, d, hdr0)
    in (level, ascending rows) order; hdr0 counts the 64-row headers of the second segments of the ranges before.  bonds: the set of
    bonds inside an exchange run (None: all); the levels stop at the first bond outside it and below bond 12."""
    out, hdr = [], 0
    if L < 14:
        return out
    for level in range(1, levels + 1):
        b = L - 2 * level
        if b < 12 or (bonds is not None and b not in bonds):
            break
        for top in range(1 << (2 * (level - 1))):  # the bits above the pair, sites b + 2 ..., ascending = ascending rows
            if any(((top >> (2 * t)) & 1) != ((top >> (2 * t + 1)) & 1) for t in range(level - 1)):
                continue  # a higher pair differs: that row belongs to a level above
            m = k - bin(top).count("1") - 1  # set bits below site b
            if m < 0 or m > b:
                continue
            base, j = 0, m + 1
            for i in range(2 * (level - 1)):
                if (top >> i) & 1:
                    j += 1
                    base += comb(b + 2 + i, j)
            r01, r10 = base + comb(b, m + 1), base + comb(b + 1, m + 1)
            a0, a1 = -(-r01 // 512) * 512, r10 // 512 * 512
            if a1 > a0:
                out.append((level, b, a0, a1, r10 - r01, hdr))
                hdr += (a1 - a0) // 64
    return out


def _maps(lib, L, k, chunk, pair_chunk, levels):
    rest, pairs, ranges = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_int64)()
    out = (C.c_int64 * 4)()
    nr = lib.ls_amd_test_tilemap_pair_levels(L, k, 1024, chunk, pair_chunk, levels, C.byref(rest), C.byref(pairs), C.byref(ranges), out)
    assert nr >= 0
    if nr == 0:
        return None
    n, rest_slots, pair_slots, depth = (int(v) for v in out)
    r = np.ctypeslib.as_array(rest, shape=(8 * max(rest_slots, 1),)).copy()
    p = np.ctypeslib.as_array(pairs, shape=(8 * max(pair_slots, 1),)).copy()
    t = np.ctypeslib.as_array(ranges, shape=(nr, 6)).copy()
    for q in (rest, pairs, ranges):
        lib.ls_amd_test_free(q)
    return n, depth, [tuple(int(v) for v in row) for row in t], r.reshape(8, -1), p.reshape(8, -1)


def _old_maps(lib, L, k, chunk):
    rest, pairs = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
    out = (C.c_int64 * 6)()
    rc = lib.ls_amd_test_tilemap_paired(L, k, 1024, chunk, C.byref(rest), C.byref(pairs), out)
    assert rc >= 0
    if rc == 0:
        return None
    r = np.ctypeslib.as_array(rest, shape=(8 * max(int(out[4]), 1),)).copy()
    p = np.ctypeslib.as_array(pairs, shape=(8 * max(int(out[5]), 1),)).copy()
    lib.ls_amd_test_free(rest)
    lib.ls_amd_test_free(pairs)
    return tuple(int(v) for v in out[:4]), r.reshape(8, -1), p.reshape(8, -1)


@pytest.mark.parametrize("chunk", [256, 3, 0])
def test_tile_maps_and_range_table(chunk):
    """L = 14..24, every weight, levels 1..6: the range table is the closed form; every row lies in exactly one tile of the two maps;
    paired tiles are whole, name their range and start on the 512 grid inside it; a tile of the other map is flagged exactly when it
    starts or ends off the 64-row grid, and one that starts off it ends on it; levels = 1 gives the maps of the one-level hook byte for
    byte"""
    lib = _lib()
    M32, M11 = np.uint64(0xFFFFFFFF), np.uint64(0x7FF)
    per_level_seen, mixed_level = {}, False
    for L in range(14, 25):
        for k in range(1, L):
            for levels in range(1, MAX_LEVELS + 1):
                want = closed_form(L, k, levels)
                got = _maps(lib, L, k, chunk, chunk, levels)
                if got is None:
                    assert not want, (L, k, levels)
                    continue
                n, depth, table, rest, pairs = got
                assert n == comb(L, k) and table == want and depth == want[-1][0], (L, k, levels, table, want)
                if levels == 1:
                    old = _old_maps(lib, L, k, chunk)
                    assert old is not None and old[0] == (n, want[0][2], want[0][3], want[0][4])
                    assert old[1].tobytes() == rest.tobytes() and old[2].tobytes() == pairs.tobytes(), (L, k)
                if levels == MAX_LEVELS:
                    count = [sum(1 for r in want if r[0] == lv) for lv in range(1, MAX_LEVELS + 1)]
                    per_level_seen[(L, k)] = count
                    # an empty range beside a non-empty one: fewer ranges at a level than patterns of the higher pairs that have rows
                    for lv in range(2, MAX_LEVELS + 1):
                        b = L - 2 * lv
                        with_rows = sum(comb(lv - 1, ones) for ones in range(lv) if 0 <= k - 2 * ones - 1 <= b) if b >= 12 else 0
                        mixed_level |= 0 < count[lv - 1] < with_rows
                r = rest.ravel()
                r = r[(r >> np.uint64(48)) != 0]
                start = (r & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64)
                cnt = ((r >> np.uint64(48)) & M11).astype(np.int64)
                plain = (r >> np.uint64(63)).astype(bool)
                end = start + cnt
                if len(r):
                    assert ((r >> np.uint64(59)) & np.uint64(0xF)).max() == 0 and cnt.min() >= 1 and cnt.max() <= 1024
                    assert np.array_equal(plain, (start % 64 != 0) | ((end % 64 != 0) & (end != n))), (L, k, levels)
                    off = start % 64 != 0
                    assert np.all((end[off] % 64 == 0) | (end[off] == n)), (L, k, levels)
                    assert np.all(start // 1024 == (end - 1) // 1024)
                p = pairs.ravel()
                p = p[(p >> np.uint64(48)) != 0]
                assert np.all((p >> np.uint64(48)) == 1024)
                i0 = (p & M32).astype(np.int64)
                rid = ((p >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
                assert rid.max() < len(want) and np.all(i0 % 512 == 0)
                a0 = np.array([w[2] for w in want])[rid]
                a1 = np.array([w[3] for w in want])[rid]
                d = np.array([w[4] for w in want])[rid]
                assert np.all((a0 <= i0) & (i0 + 512 <= a1))
                assert len(i0) == sum((w[3] - w[2]) // 512 for w in want)
                # every row exactly once: the segments of all tiles, sorted, follow each other from 0 to n
                s = np.concatenate([start, i0, i0 + d])
                e = np.concatenate([end, i0 + 512, i0 + d + 512])
                order = np.argsort(s, kind="stable")
                s, e = s[order], e[order]
                assert s[0] == 0 and e[-1] == n and np.array_equal(s[1:], e[:-1]), (L, k, levels)
                if chunk > 0 and levels == MAX_LEVELS:  # ascending rows, chunks of consecutive tiles go round the XCD lists
                    flat = pairs.ravel() & M32
                    live = (pairs.ravel() >> np.uint64(48)) != 0
                    for q, row in enumerate(np.sort(i0)[:40]):
                        xcd = int(np.flatnonzero(live & (flat == np.uint64(row)))[0]) // pairs.shape[1]
                        assert xcd == (q // chunk) % 8
    assert [1, 2, 4, 2] == per_level_seen[(20, 10)][:4], per_level_seen[(20, 10)]
    assert all(c > 0 for c in per_level_seen[(24, 12)]), per_level_seen[(24, 12)]
    assert per_level_seen[(16, 8)][:2] == [1, 1] and mixed_level


def test_paired_map_has_a_chunk_of_its_own():
    """pair_chunk deals the paired map, chunk the other one"""
    lib = _lib()
    a = _maps(lib, 20, 10, 256, 3, 4)
    b = _maps(lib, 20, 10, 256, 256, 4)
    c = _maps(lib, 20, 10, 3, 3, 4)
    assert a[3].tobytes() == b[3].tobytes() and a[4].tobytes() != b[4].tobytes()
    assert a[4].tobytes() == c[4].tobytes() and a[3].tobytes() != c[3].tobytes()


@pytest.mark.parametrize("L,k", [(16, 8), (17, 8), (19, 9), (20, 10)])
def test_ranges_pair_rows_across_their_bond(L, k):
    """on the enumerated states: row a0 + j and row a0 + d + j differ in the two bits of the range's bond and in nothing else, for
    every range of the table, and no row lies in two ranges"""
    lib = _lib()
    words = np.arange(1 << L, dtype=np.uint32)
    ones = np.zeros(1 << L, dtype=np.uint8)
    for b in range(L):
        ones += ((words >> np.uint32(b)) & np.uint32(1)).astype(np.uint8)
    states = words[ones == k].astype(np.int64)  # ascending = the combinadic order
    got = _maps(lib, L, k, 256, 256, MAX_LEVELS)
    assert got is not None and len(states) == got[0]
    claimed = np.zeros(len(states), dtype=np.int32)
    assert len(got[2]) >= 2
    for level, bond, a0, a1, d, _ in got[2]:
        assert bond == L - 2 * level and bond >= 12
        assert np.all(states[a0:a1] ^ states[a0 + d:a1 + d] == 3 << bond), (L, k, level, a0)
        assert np.all((states[a0:a1] >> bond) & 3 == 1)
        claimed[a0:a1] += 1
        claimed[a0 + d:a1 + d] += 1
    assert claimed.max() == 1


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


def _matvec(torch, cfg, x):
    import distributed_matvec_amd as D

    lib = _lib()
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    xs = D.arrFromBlockToHashed(torch.from_numpy(np.ascontiguousarray(x)).cuda(), masks, 1)
    ys = [torch.zeros_like(v) for v in xs]
    pl = D.matrixVectorProduct(h, xs, ys, reps, mode="pull")
    y = D.arrFromHashedToBlock(ys, masks).cpu().numpy()
    rows = [int(lib.ls_amd_plan_chain_paired_rows_at(pl.h, lv)) for lv in range(1, MAX_LEVELS + 1)]
    assert rows[0] == int(lib.ls_amd_plan_chain_paired_rows(pl.h))
    return y, pl.kernel, rows, int(lib.ls_amd_plan_chain_pair_levels(pl.h))


def _rows_per_level(table, depth):
    return [sum(2 * (r[3] - r[2]) for r in table if r[0] == lv and lv <= depth) for lv in range(1, MAX_LEVELS + 1)]


# name: (sites, weight, ring / open, Jz, deepest level with a range, ranges at that level)
SHAPES = {
    "ring16-w8": (16, 8, "ring", 1.0, 2, 1),    # 12 870 rows: level 2 on bond 12, the lowest far pair; one of its two ranges is empty
    "ring17-w8": (17, 8, "ring", 1.0, 2, 2),    # 24 310 rows: odd L, bonds 15 / 13; a second window that starts at an odd row
    "ring19-w9": (19, 9, "ring", 1.0, 3, 3),    # 92 378 rows: three levels, 3 of 4 ranges at level 3
    "ring20-w10": (20, 10, "ring", 1.0, 4, 2),  # 184 756 rows: four levels
    "ring20-w7": (20, 7, "ring", 1.0, 4, 1),    # 77 520 rows: off half filling, level 4 with 1 of 8 ranges
    "open20-w10": (20, 10, "open", 1.0, 4, 2),  # no cached pair
    "xxz20-w10": (20, 10, "ring", 0.35, 4, 2),  # Jz = 0.35: another diagonal
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_levels_match_one_level_unpaired_and_generic_kernel(torch, monkeypatch, shape):
    L, weight, kind, jz, deepest, at_deepest = SHAPES[shape]
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(L, weight, kind, jz)
    n = comb(L, weight)
    x = np.random.RandomState(1000 * L + weight).rand(n) - 0.5
    table = closed_form(L, weight, MAX_LEVELS)
    assert table[-1][0] == deepest and sum(1 for r in table if r[0] == deepest) == at_deepest, table
    if shape == "ring17-w8":
        assert any((r[2] + r[4] - 256) % 2 for r in table)

    def run(**env):
        for key, value in env.items():
            monkeypatch.setenv(key, value)
        out = _matvec(torch, cfg, x)
        for key in env:
            monkeypatch.delenv(key)
        return out

    y, kernel, rows, depth = run()
    assert kernel == "direct-pull+staged" and 1 <= depth <= deepest, (kernel, depth)
    assert rows == _rows_per_level(table, depth), (rows, depth)
    y6, kernel6, rows6, depth6 = run(LS_AMD_CHAIN_PAIR_LEVELS=str(MAX_LEVELS))
    assert kernel6 == kernel and depth6 == deepest and rows6 == _rows_per_level(table, MAX_LEVELS), (rows6, depth6)
    y1, kernel1, rows1, depth1 = run(LS_AMD_CHAIN_PAIR_LEVELS="1")
    assert kernel1 == kernel and depth1 == 1 and rows1 == _rows_per_level(table, 1), (rows1, depth1)
    y_un, kernel_un, rows_un, depth_un = run(LS_AMD_CHAIN_PAIRED="0")
    assert kernel_un == kernel and depth_un == 0 and not any(rows_un)
    y_gen, kernel_gen, rows_gen, depth_gen = run(LS_AMD_ROW_KERNEL="generic")
    assert kernel_gen == "direct-pull" and depth_gen == 0 and not any(rows_gen)

    scale = np.abs(y_gen).max()
    tol = 1e-12 * scale  # the tolerance of the chain kernel's parity tests (test_chain_paired.py), element by element
    for name, other in (("levels=1", y1), ("unpaired", y_un), ("generic", y_gen)):
        for tag, mine in (("default", y), ("levels=6", y6)):
            err = np.abs(mine - other).max()
            print(f"{shape}: {tag} (rows per level {rows if tag == 'default' else rows6}) against {name}: max|dy| = {err:.3e}, max|y| = {scale:.3e}")
            assert err <= tol, (shape, tag, name, err, int(np.abs(mine - other).argmax()))
    # the records switch leaves the pairing alone (the second segments' headers then say "records" too): the same y to the bit
    y_rec, kernel_rec, rows_rec, depth_rec = run(LS_AMD_CHAIN_RECORDS="1")
    assert kernel_rec == kernel and rows_rec == rows and depth_rec == depth
    assert y.tobytes() == y_rec.tobytes(), (shape, np.abs(y - y_rec).max())
    y6_rec, _, rows6_rec, _ = run(LS_AMD_CHAIN_RECORDS="1", LS_AMD_CHAIN_PAIR_LEVELS=str(MAX_LEVELS))
    assert rows6_rec == rows6 and y6.tobytes() == y6_rec.tobytes(), (shape, np.abs(y6 - y6_rec).max())


@pytest.mark.gpu
def test_levels_stop_at_a_bond_outside_the_runs(torch, monkeypatch):
    """an open 20-site chain without bond (16, 17): level 2 would pair across it, so the plan keeps level 1 alone and y is what
    LS_AMD_CHAIN_PAIR_LEVELS=1 gives, to the bit"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(20, 10, "open", drop=(16,))
    n = comb(20, 10)
    x = np.random.RandomState(7).rand(n) - 0.5
    assert len(closed_form(20, 10, MAX_LEVELS, bonds=set(range(19)) - {16})) == 1
    monkeypatch.setenv("LS_AMD_CHAIN_PAIR_LEVELS", str(MAX_LEVELS))
    y, kernel, rows, depth = _matvec(torch, cfg, x)
    assert kernel == "direct-pull+staged" and depth == 1 and rows == _rows_per_level(closed_form(20, 10, 1), 1), (kernel, rows, depth)
    monkeypatch.setenv("LS_AMD_CHAIN_PAIR_LEVELS", "1")
    y1, kernel1, rows1, depth1 = _matvec(torch, cfg, x)
    assert (kernel1, rows1, depth1) == (kernel, rows, depth)
    assert y.tobytes() == y1.tobytes()
    monkeypatch.delenv("LS_AMD_CHAIN_PAIR_LEVELS")
    y_def, _, rows_def, depth_def = _matvec(torch, cfg, x)
    assert depth_def == 1 and rows_def == rows and y_def.tobytes() == y1.tobytes()
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, kernel_gen, _, _ = _matvec(torch, cfg, x)
    assert kernel_gen == "direct-pull"
    assert np.abs(y - y_gen).max() <= 1e-12 * np.abs(y_gen).max()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", ["0", "3"])
@pytest.mark.parametrize("knob", ["LS_AMD_TILE_CHUNK", "LS_AMD_PAIR_TILE_CHUNK"])
def test_levels_under_other_tile_orders(torch, monkeypatch, knob, chunk):
    """both chunk knobs at contiguous eighths and at chunks of three tiles, ring18-w9 at full depth (two levels, three ranges)"""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    cfg = _config(18, 9)
    n = comb(18, 9)
    x = np.random.RandomState(5).rand(n) - 0.5
    monkeypatch.setenv("LS_AMD_ROW_KERNEL", "generic")
    y_gen, _, _, _ = _matvec(torch, cfg, x)
    monkeypatch.delenv("LS_AMD_ROW_KERNEL")
    monkeypatch.setenv(knob, chunk)
    monkeypatch.setenv("LS_AMD_CHAIN_PAIR_LEVELS", str(MAX_LEVELS))
    y, kernel, rows, depth = _matvec(torch, cfg, x)
    table = closed_form(18, 9, MAX_LEVELS)
    assert kernel == "direct-pull+staged" and depth == table[-1][0] == 2 and rows == _rows_per_level(table, MAX_LEVELS), (kernel, rows)
    assert np.abs(y - y_gen).max() <= 1e-12 * np.abs(y_gen).max()
