"""Sector-state expansion without a device: the reference formula <s|psi> = conj(character(s)) norm(rep) psi[index(rep)] of
tests/entanglement_reference.py equals the explicit projector columns P|r> / |P|r>| of oracle.model.dense_sector_matrix's
convention; the block table of a bipartition (ls_amd_test_expand_layout) is the binomials with cumulative offsets; the refusals
that need no device fire; and the C ABI and the Python names are declared and exported."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import entanglement_reference as E
from distributed_matvec_amd import SectorExpansion  # noqa: F401  (the feature under test: without it nothing here can run)
from distributed_matvec_amd import config
from helpers import model_config
from oracle import model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_expand_create", "ls_amd_expand_num_blocks", "ls_amd_expand_block", "ls_amd_expand_total", "ls_amd_expand_apply",
         "ls_amd_expand_check", "ls_amd_expand_kernel_name", "ls_amd_expand_destroy", "ls_amd_test_expand_layout")

CASES = {
    "ring8_k0": lambda: E.ring(8, 4, 0),
    "ring8_k1": lambda: E.ring(8, 4, 1),
    "ring8_k3": lambda: E.ring(8, 4, 3),
    "ring8_reflection_odd": lambda: E.ring(8, 4, None, reflect=1),
    "ring8_k0_reflection_inversion_minus": lambda: E.ring(8, 4, 0, inv=-1, reflect=0),
    "ring10_inversion_minus_only": lambda: E.ring(10, 5, None, inv=-1),
    "square_4x4_lattice_group": lambda: {"basis": model_config("heisenberg_square_4x4")["basis"]},
}


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_expansion_equals_the_projector_columns(name):
    cfg = CASES[name]()
    model, full, reps, idx, coef, live = E.tables(cfg)
    assert np.array_equal(reps, M.enumerate_representatives(model)) if len(full) <= 256 else len(reps) > 0
    preps, B = E.projector_columns(cfg)
    assert np.array_equal(preps, reps)
    got = np.zeros_like(B)
    got[np.nonzero(live)[0], idx[live]] = coef[live]
    err = np.abs(got - B).max()
    print(f"{name}: {len(full)} states, {len(reps)} representatives, {int((~live).sum())} states of zero norm, max deviation {err:.2e}")
    assert err <= 1e-13
    # expand_full is that matrix applied to psi
    psi = np.random.RandomState(3).randn(len(reps)) + 1j * np.random.RandomState(4).randn(len(reps))
    assert np.abs(E.expand_full(cfg, psi) - B @ psi).max() <= 1e-13 * np.abs(psi).max() * 4
    if name == "ring8_k1":
        assert (~live).any()  # a sector where some orbits have zero norm


@pytest.mark.parametrize("name", ["ring8_k3", "ring8_k0_reflection_inversion_minus", "square_4x4_lattice_group"])
def test_vectorised_state_info_is_the_oracles(name):
    cfg = CASES[name]()
    model, full = E.tables(cfg)[0], E.tables(cfg)[1]
    sample = full if len(full) <= 256 else full[:: len(full) // 40]
    rep, ch, nrm = E.state_info_all(model, sample)
    for s, r, c, n in zip(sample, rep, ch, nrm):
        r0, c0, n0 = M.state_info(model, int(s))
        assert int(r) == r0 and abs(n - n0) <= 1e-15
        if n0 > 0:  # (the character of a zero-norm orbit depends on which minimising element is met first)
            assert abs(c - c0) <= 1e-15


def _layout(basis, mask, cap=65):
    na, rows, cols, offs, total = (C.c_int * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64()
    nb = _lib().ls_amd_test_expand_layout(basis.payload, C.c_uint64(mask), cap, na, rows, cols, offs, C.byref(total))
    assert nb >= 0, _lib().ls_amd_last_error().decode()
    return [(na[i], rows[i], cols[i], offs[i]) for i in range(nb)], total.value


LAYOUTS = [
    ("contiguous_low", E.ring(12, 6, 0), [0, 1, 2, 3, 4, 5]),
    ("contiguous_high", E.ring(12, 6, 0), [6, 7, 8, 9, 10, 11]),
    ("scattered", E.ring(12, 6, 0), [0, 2, 5, 7]),
    ("one_site", E.ring(12, 6, 0), [3]),
    ("all_sites", E.ring(12, 6, 0), list(range(12))),
    ("weight_4_of_12_A_of_7", E.ring(12, 4, None), [0, 1, 2, 3, 4, 5, 6]),
    ("weight_9_of_12_A_of_5", E.ring(12, 9, None), [1, 3, 5, 7, 9]),
    ("L34_weight_2", E.ring(34, 2, 0), list(range(17))),
    ("L34_weight_17_scattered", E.ring(34, 17, 0), list(range(0, 34, 2))),
    ("L34_all_sites", E.ring(34, 2, 0), list(range(34))),
]


@pytest.mark.parametrize("name,cfg,sites", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_layout_matches_the_binomials(name, cfg, sites):
    basis = D.loadConfigFromDict(cfg)
    L, w = cfg["basis"]["number_spins"], cfg["basis"]["hamming_weight"]
    blocks, total = _layout(basis, sum(1 << s for s in sites))
    want, off = [], 0
    for na in range(len(sites) + 1):
        r, c = math.comb(len(sites), na), (math.comb(L - len(sites), w - na) if 0 <= w - na else 0)
        if r * c == 0:
            continue  # empty blocks are dropped
        want.append((na, r, c, off))
        off += r * c
    assert blocks == want and total == off == math.comb(L, w)
    ex = D.SectorExpansion(basis, _no_reps(), sites)
    assert ex.blocks == [b[:3] for b in want] and ex.offsets == [b[3] for b in want] and ex.total == off
    if name == "all_sites":
        assert blocks == [(6, 924, 1, 0)]
    if name == "weight_9_of_12_A_of_5":
        assert [b[0] for b in blocks] == [2, 3, 4, 5]  # n_A < 2 would need more than 7 particles on the 7 sites of B


def _no_reps():
    import torch

    return torch.zeros(0, dtype=torch.int64)


def test_layout_without_a_fixed_weight_is_one_block():
    basis = D.loadConfigFromDict({"basis": {"number_spins": 10, "symmetries": []}})
    assert _layout(basis, 0b0000011111) == ([(-1, 32, 32, 0)], 1024)
    assert _layout(basis, 0b1010010001) == ([(-1, 16, 64, 0)], 1024)
    assert _layout(basis, (1 << 10) - 1) == ([(-1, 1024, 1, 0)], 1024)
    assert D.SectorExpansion(basis, _no_reps(), None).blocks == [(-1, 1024, 1)]


def test_refusals_that_need_no_device():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    spin = D.loadConfigFromDict(E.ring(8, 4, 0))
    # a mask with bits outside the sites
    assert L.ls_amd_test_expand_layout(spin.payload, C.c_uint64(1 << 8), 0, None, None, None, None, None) == -1
    assert "outside the 8 sites" in err()
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    assert L.ls_amd_expand_create(C.byref(h), spin.payload, reps, 4, C.c_uint64(1 << 9), None) == -1 and "outside the 8 sites" in err()
    assert L.ls_amd_expand_create(None, spin.payload, reps, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert L.ls_amd_expand_create(C.byref(h), None, reps, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert L.ls_amd_expand_create(C.byref(h), spin.payload, None, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert h.value is None
    assert L.ls_amd_expand_apply(None, 0, reps, reps, 0, 1, None) == -1 and "NULL" in err()
    assert L.ls_amd_expand_check(None, None) == -1 and L.ls_amd_expand_total(None) == -1 and L.ls_amd_expand_num_blocks(None) == -1
    assert L.ls_amd_expand_kernel_name(None) is None
    L.ls_amd_expand_destroy(None)
    # fermionic bases of every kind: refused by name, in C and in Python
    fermions = [
        {"basis": {"particle": "spinless-fermion", "number_sites": 6, "number_particles": 3}},
        {"basis": {"particle": "spinful-fermion", "number_sites": 4, "number_particles": 4, "number_up": 2}},
        {"basis": {"particle": "spinless-fermion", "number_sites": 6, "number_particles": 3,
                   "symmetries": [{"permutation": [1, 2, 3, 4, 5, 0], "sector": 0}]}},
    ]
    for cfg in fermions:
        fb = D.loadConfigFromDict(cfg)
        assert L.ls_amd_test_expand_layout(fb.payload, C.c_uint64(3), 0, None, None, None, None, None) == -1
        assert "fermionic" in err() and "mode-ordering signs" in err()
        assert L.ls_amd_expand_create(C.byref(h), fb.payload, reps, 4, C.c_uint64(3), None) == -1 and "mode-ordering signs" in err()
        with pytest.raises(D.LsAmdError, match="mode-ordering signs"):
            D.SectorExpansion(fb, _no_reps(), [0, 1])
        with pytest.raises(D.LsAmdError, match="mode-ordering signs"):
            D.unproject(fb, _no_reps(), _no_reps().double())
    # sites: out of range, duplicates, not integers -- before any device is asked for
    for sites, what in (([0, 8], "outside the 8 sites"), ([-1], "outside the 8 sites"), ([1, 3, 1], "listed twice"), ([0.5], "integers")):
        with pytest.raises(D.LsAmdError, match=what):
            D.SectorExpansion(spin, _no_reps(), sites)
        with pytest.raises(D.LsAmdError, match=what):
            D.reduced_density_matrix(spin, _no_reps(), _no_reps().double(), sites)
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.SectorExpansion(spin, [_no_reps(), _no_reps()], [0])
    # psi: shape, length, dtype, device -- before any device is asked for
    import torch

    ex = D.SectorExpansion(spin, torch.zeros(10, dtype=torch.int64), [0, 1, 2, 3])
    with pytest.raises(D.LsAmdError, match="ONE vector"):
        ex.expand(torch.zeros(10, 2, dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match="9 elements"):
        ex.expand(torch.zeros(9, dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match="neither float64 nor complex128"):
        ex.expand(torch.zeros(10, dtype=torch.float32))
    with pytest.raises(D.LsAmdError, match="device tensor"):
        ex.expand(torch.zeros(10, dtype=torch.float64))
    with pytest.raises(D.LsAmdError, match="consecutive"):
        ex.expand(torch.zeros(10, dtype=torch.float64), blocks=[0, 2])


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_expand_create\s*\(\s*ls_amd_expand\s*\*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*\s*\w+\s*,\s*uint64_t\s+const\s*\*"
                     r"\s*d_reps\s*,\s*int64_t\s+n\s*,\s*uint64_t\s+subsystem_mask\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"int\s+ls_amd_expand_apply\s*\(\s*ls_amd_expand\s*\*\s*\w+\s*,\s*ls_amd_dtype\s+\w+\s*,\s*void\s+const\s*\*\s*d_psi\s*,\s*void\s*\*"
                     r"\s*d_out\s*,\s*int\s+first_block\s*,\s*int\s+num_blocks\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
    from distributed_matvec_amd import entanglement

    for name in ("SectorExpansion", "unproject", "reduced_density_matrix", "entanglement_spectrum", "entanglement_entropy"):
        assert callable(getattr(D, name)) and getattr(D, name) is getattr(entanglement, name) and name in D.__all__
    for name in ("expand", "check", "destroy", "kernel", "blocks"):
        assert hasattr(D.SectorExpansion, name) or name == "blocks"
    assert "max_bytes" in D.SectorExpansion.expand.__code__.co_varnames
    assert "k_expand.hip" in open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile")).read()
    assert config.PARTICLES["spin-1/2"] == 0
