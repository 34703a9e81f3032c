"""Fermionic sector-state expansion without a device: the bipartition sign of the device code's host run
(ls_amd_test_fermi_split_parity) equals the brute-force pair count; the block tables of spinless and spinful bases
(ls_amd_test_fermi_expand_layout) equal shapes and offsets computed in numpy; the refusals that need no device fire; the reference's
vectorised projector columns equal those of fermion_symm / fermion_spinful_symm; and the C ABI and the Python names are declared and
exported."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import distributed_matvec_amd as D
import fermion_entanglement_reference as R
import fermion_spinful_symm as FS
import fermion_symm as F
from distributed_matvec_amd import FermionSectorExpansion  # noqa: F401  (the feature under test: without it nothing here can run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_fermi_expand_create", "ls_amd_fermi_expand_block", "ls_amd_test_fermi_expand_layout", "ls_amd_test_fermi_split_parity")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def _no_reps():
    import torch

    return torch.zeros(0, dtype=torch.int64)


def _brute(mask, modes, state):
    """(-1)^#{(i, j): i in A, j in B, both occupied, j < i}, one pair at a time"""
    count = 0
    for i in range(modes):
        if (mask >> i) & 1 and (state >> i) & 1:
            for j in range(i):
                if not (mask >> j) & 1 and (state >> j) & 1:
                    count += 1
    return -1 if count & 1 else 1


@pytest.mark.parametrize("modes", [1, 31, 32, 33, 63, 64])
def test_split_parity_is_the_pair_count(modes):
    L = _lib()
    rs = np.random.RandomState(modes)
    full = (1 << modes) - 1
    top = 1 << (modes - 1)

    def word():
        return int(rs.randint(0, 1 << 32)) << 32 | int(rs.randint(0, 1 << 32))

    pairs = [(0, full), (full, full), (0, 0), (full, 0), (top, full), (full & ~top, full), (top, top), (full & ~top, top | 1)]
    for _ in range(600):
        m, s = word() & full, word() & full
        pairs += [(m, s), (m | top, s | top), (m & ~top, s | top)]
    worst = 0
    for m, s in pairs:
        got = L.ls_amd_test_fermi_split_parity(C.c_uint64(m), modes, C.c_uint64(s))
        worst += got != _brute(m, modes, s)
    assert worst == 0 and len(pairs) > 1800
    assert any(m >> (modes - 1) & 1 and s >> (modes - 1) & 1 for m, s in pairs)
    # the empty and the full mask: nothing to carry past
    assert all(L.ls_amd_test_fermi_split_parity(C.c_uint64(mm), modes, C.c_uint64(s)) == 1 for mm in (0, full) for _, s in pairs[:50])
    # bad arguments
    if modes < 64:
        assert L.ls_amd_test_fermi_split_parity(C.c_uint64(1 << modes), modes, C.c_uint64(0)) == 0
        assert L.ls_amd_test_fermi_split_parity(C.c_uint64(0), modes, C.c_uint64(1 << modes)) == 0
    assert L.ls_amd_test_fermi_split_parity(C.c_uint64(0), 0, C.c_uint64(0)) == 0 and L.ls_amd_test_fermi_split_parity(C.c_uint64(0), 65, C.c_uint64(0)) == 0


def test_split_parity_is_the_references_sigma():
    L = _lib()
    states = np.arange(1 << 10, dtype=np.uint64)
    for a_modes in ([0, 2, 5, 7], [1, 4, 6], [0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [9], []):
        want = R.sigma(states, a_modes, 10)
        mask = sum(1 << m for m in a_modes)
        got = np.array([L.ls_amd_test_fermi_split_parity(C.c_uint64(mask), 10, C.c_uint64(int(s))) for s in states])
        assert np.array_equal(got, want)
        if a_modes in ([0, 1, 2, 3, 4], []):
            assert (want == 1).all()  # the modes of A already stand in front
    assert (R.sigma(states, [0, 2, 5, 7], 10) == -1).any()


def _layout(basis, mask, cap=33 * 33):
    nu, nd = (C.c_int * cap)(), (C.c_int * cap)()
    rows, cols, offs, total = (C.c_int64 * cap)(), (C.c_int64 * cap)(), (C.c_int64 * cap)(), C.c_int64()
    nb = _lib().ls_amd_test_fermi_expand_layout(basis.payload, C.c_uint64(mask), cap, nu, nd, rows, cols, offs, C.byref(total))
    assert nb >= 0, _lib().ls_amd_last_error().decode()
    return [(nu[i], nd[i], rows[i], cols[i], offs[i]) for i in range(nb)], total.value


def _spinless(L, N, gens=(), secs=()):
    return D.loadConfigFromDict({"basis": R.Case(L, N, gens=gens, secs=secs).basis_config()})


def _spinful(L, nu, nd, gens=(), secs=(), flip=0):
    return D.loadConfigFromDict({"basis": R.Case(L, up=(nu, nd), gens=gens, secs=secs, flip=flip).basis_config()})


SPINLESS_LAYOUTS = [
    ("scattered", 12, 6, [0, 2, 5, 7]), ("low", 12, 6, list(range(6))), ("high", 12, 6, list(range(6, 12))), ("one", 12, 5, [3]),
    ("empty", 12, 6, []), ("all", 12, 6, list(range(12))), ("few_particles", 12, 2, [1, 3, 5, 7, 9]), ("many_particles", 12, 9, [1, 3, 5, 7, 9]),
    ("34_modes", 34, 2, list(range(0, 34, 2))), ("64_modes", 64, 3, [0, 31, 32, 63]),
]


@pytest.mark.parametrize("name,L,N,modes", SPINLESS_LAYOUTS, ids=[c[0] for c in SPINLESS_LAYOUTS])
def test_spinless_layout_with_fixed_number(name, L, N, modes):
    basis = _spinless(L, N, F.translations(L), [1]) if name != "64_modes" else _spinless(L, N)
    blocks, total = _layout(basis, sum(1 << m for m in modes))
    want, off = [], 0
    for na in range(len(modes) + 1):
        r, c = math.comb(len(modes), na), (math.comb(L - len(modes), N - na) if N - na >= 0 else 0)
        if r * c == 0:
            continue
        want.append((na, -1, r, c, off))
        off += r * c
    assert blocks == want and total == off == math.comb(L, N)
    ex = D.FermionSectorExpansion(basis, _no_reps(), sites=modes)  # (spinless: sites are modes)
    assert ex.blocks == [(b[0], b[2], b[3]) for b in want] and ex.offsets == [b[4] for b in want] and ex.total == off
    assert D.FermionSectorExpansion(basis, _no_reps(), modes=modes).blocks == ex.blocks
    if name == "all":
        assert blocks == [(6, -1, 924, 1, 0)]
    if name == "empty":
        assert blocks == [(0, -1, 1, 924, 0)]


def test_spinless_layout_with_every_number_is_one_block():
    basis = _spinless(10, None, F.translations(10), [1])
    assert _layout(basis, 0b0000011111) == ([(-1, -1, 32, 32, 0)], 1024)
    assert _layout(basis, 0b1010010001) == ([(-1, -1, 16, 64, 0)], 1024)
    assert _layout(basis, (1 << 10) - 1) == ([(-1, -1, 1024, 1, 0)], 1024)
    assert _layout(basis, 0) == ([(-1, -1, 1, 1024, 0)], 1024)
    assert D.FermionSectorExpansion(basis, _no_reps()).blocks == [(-1, 1024, 1)]
    # a spinful basis with number_up unset is a spinless one on its 2 L modes; a site brings both of its modes
    for npart in (4, None):
        b = {"particle": "spinful-fermion", "number_sites": 5}
        if npart is not None:
            b["number_particles"] = npart
        basis = D.loadConfigFromDict({"basis": b})
        ex = D.FermionSectorExpansion(basis, _no_reps(), sites=[0, 3])
        assert ex.mask == 0b0100101001 and not ex.spinful_layout
        if npart is None:
            assert ex.blocks == [(-1, 16, 64)]
        else:
            assert ex.blocks == [(n, math.comb(4, n), math.comb(6, 4 - n)) for n in range(5)] and ex.total == math.comb(10, 4)


def _product_layout(L, nu, nd, a_modes):
    au, ad = sum(1 for m in a_modes if m < L), sum(1 for m in a_modes if m >= L)
    want, off = [], 0
    for n_up in range(au + 1):
        for n_dn in range(ad + 1):
            if nu - n_up < 0 or nd - n_dn < 0:
                continue
            r = math.comb(au, n_up) * math.comb(ad, n_dn)
            c = math.comb(L - au, nu - n_up) * math.comb(L - ad, nd - n_dn)
            if r * c == 0:
                continue
            want.append((n_up, n_dn, r, c, off))
            off += r * c
    return want, off


SPINFUL_LAYOUTS = [
    ("sites_scattered", 6, 3, 3, dict(sites=[0, 2, 3])), ("sites_low", 6, 3, 3, dict(sites=[0, 1, 2])), ("sites_one", 6, 3, 2, dict(sites=[4])),
    ("up_modes_only", 6, 3, 3, dict(modes=[0, 2, 3])), ("down_modes_only", 6, 2, 4, dict(modes=[7, 8, 11])),
    ("mixed_modes", 7, 3, 2, dict(modes=[0, 5, 8, 9, 13])), ("empty", 6, 3, 3, dict(sites=[])), ("all", 6, 3, 3, dict()),
    ("34_modes", 17, 1, 1, dict(sites=[0, 2, 5, 7])), ("64_modes", 32, 2, 1, dict(sites=[0, 31])),
]


@pytest.mark.parametrize("name,L,nu,nd,sub", SPINFUL_LAYOUTS, ids=[c[0] for c in SPINFUL_LAYOUTS])
def test_spinful_product_layout(name, L, nu, nd, sub):
    basis = _spinful(L, nu, nd, F.translations(L), [1]) if L < 32 else _spinful(L, nu, nd)
    case = R.Case(L, up=(nu, nd))
    a_modes = case.modes_of(**sub)
    want, off = _product_layout(L, nu, nd, a_modes)
    blocks, total = _layout(basis, sum(1 << m for m in a_modes))
    assert blocks == want and total == off == math.comb(L, nu) * math.comb(L, nd)
    assert [b[:2] for b in blocks] == sorted(b[:2] for b in blocks)  # lexicographic in (n_up, n_dn)
    ex = D.FermionSectorExpansion(basis, _no_reps(), **sub)
    assert ex.spinful_layout and ex.mask == sum(1 << m for m in a_modes)
    assert ex.blocks == [((b[0], b[1]), b[2], b[3]) for b in want] and ex.offsets == [b[4] for b in want] and ex.total == off
    if name == "all":
        assert blocks == [(3, 3, 400, 1, 0)]
    if name == "empty":
        assert blocks == [(0, 0, 1, 400, 0)]
    if name == "up_modes_only":
        assert [b[:2] for b in blocks] == [(0, 0), (1, 0), (2, 0), (3, 0)]
    if name == "sites_scattered":
        assert len(blocks) == 16
    if L <= 7:  # the reference's bipartition has the same shapes
        ref = R.bipartition(case, np.ones(len(case.states)), a_modes)
        assert [(lab, m.shape[0], m.shape[1]) for lab, m in ref] == ex.blocks


def test_refusals_that_need_no_device():
    L = _lib()
    err = lambda: L.ls_amd_last_error().decode()  # noqa: E731
    h = C.c_void_p()
    reps = (C.c_uint64 * 4)()
    # spin bases, by name
    spin = D.loadConfigFromDict({"basis": {"number_spins": 8, "hamming_weight": 4}})
    assert L.ls_amd_test_fermi_expand_layout(spin.payload, C.c_uint64(3), 0, None, None, None, None, None, None) == -1 and "spin-1/2" in err()
    assert L.ls_amd_fermi_expand_create(C.byref(h), spin.payload, reps, 4, C.c_uint64(3), None) == -1 and "spin-1/2" in err()
    assert h.value is None
    with pytest.raises(D.LsAmdError, match="spin-1/2"):
        D.FermionSectorExpansion(spin, _no_reps(), [0, 1])
    with pytest.raises(D.LsAmdError, match="spin-1/2"):
        D.fermion_unproject(spin, _no_reps(), _no_reps().double())
    with pytest.raises(D.LsAmdError, match="modes="):
        D.reduced_density_matrix(spin, _no_reps(), _no_reps().double(), None, modes=[0])
    # NULL arguments
    fb = _spinless(8, 4)
    assert L.ls_amd_fermi_expand_create(None, fb.payload, reps, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert L.ls_amd_fermi_expand_create(C.byref(h), None, reps, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert L.ls_amd_fermi_expand_create(C.byref(h), fb.payload, None, 4, C.c_uint64(1), None) == -1 and "NULL" in err()
    assert L.ls_amd_fermi_expand_block(None, 0, None, None, None, None, None) == -1
    # masks outside the modes
    assert L.ls_amd_test_fermi_expand_layout(fb.payload, C.c_uint64(1 << 8), 0, None, None, None, None, None, None) == -1
    assert "outside the 8 modes" in err()
    assert L.ls_amd_fermi_expand_create(C.byref(h), fb.payload, reps, 4, C.c_uint64(1 << 9), None) == -1 and "outside the 8 modes" in err()
    sf = _spinful(4, 2, 2)
    assert L.ls_amd_test_fermi_expand_layout(sf.payload, C.c_uint64(1 << 8), 0, None, None, None, None, None, None) == -1
    assert "outside the 8 modes" in err()
    assert L.ls_amd_test_fermi_expand_layout(sf.payload, C.c_uint64(1 << 7), 0, None, None, None, None, None, None) == 2
    # a particle number beyond the binomial table (C(n, k), k < 34): such a basis is refused where it is created, so the layout's own
    # check of the weight is never the first to speak; the largest admissible number has its table
    with pytest.raises(D.LsAmdError, match="binomial table"):
        _spinless(40, 34)
    with pytest.raises(D.LsAmdError, match="binomial table"):
        D.loadConfigFromDict({"basis": {"particle": "spinful-fermion", "number_sites": 20, "number_particles": 34}})
    assert L.ls_amd_test_fermi_expand_layout(_spinless(40, 33).payload, C.c_uint64(3), 0, None, None, None, None, None, None) == 3
    # more than 40 modes without a fixed number
    assert L.ls_amd_test_fermi_expand_layout(_spinless(41, None).payload, C.c_uint64(3), 0, None, None, None, None, None, None) == -1
    assert "41 modes without a fixed" in err()
    wide = D.loadConfigFromDict({"basis": {"particle": "spinful-fermion", "number_sites": 21}})
    with pytest.raises(D.LsAmdError, match="42 modes without a fixed"):
        D.FermionSectorExpansion(wide, _no_reps(), sites=[0])
    assert L.ls_amd_test_fermi_expand_layout(_spinless(40, None).payload, C.c_uint64(3), 0, None, None, None, None, None, None) == 1
    # sites and modes: both, out of range, duplicates, not integers -- before any device is asked for
    with pytest.raises(D.LsAmdError, match="not both"):
        D.FermionSectorExpansion(sf, _no_reps(), sites=[0], modes=[0])
    with pytest.raises(D.LsAmdError, match="not both"):
        D.entanglement_entropy(sf, _no_reps(), _no_reps().double(), [0], modes=[0])
    for kw, what in ((dict(sites=[0, 4]), "site 4 is outside the 4 sites"), (dict(modes=[8]), "mode 8 is outside the 8 modes"),
                     (dict(modes=[-1]), "outside the 8 modes"), (dict(sites=[1, 3, 1]), "listed twice"), (dict(modes=[0.5]), "integers")):
        with pytest.raises(D.LsAmdError, match=what):
            D.FermionSectorExpansion(sf, _no_reps(), **kw)
        with pytest.raises(D.LsAmdError, match=what):
            D.reduced_density_matrix(sf, _no_reps(), _no_reps().double(), kw.get("sites"), modes=kw.get("modes"))
    with pytest.raises(D.LsAmdError, match="one partition"):
        D.FermionSectorExpansion(sf, [_no_reps(), _no_reps()], [0])
    # the spin entry points still refuse fermions, and say where to go
    assert L.ls_amd_expand_create(C.byref(h), fb.payload, reps, 4, C.c_uint64(3), None) == -1
    assert "fermionic" in err() and "mode-ordering signs" in err() and "ls_amd_fermi_expand_create" in err()
    # psi: shape, length, dtype, device -- before any device is asked for
    import torch

    ex = D.FermionSectorExpansion(sf, torch.zeros(10, dtype=torch.int64), [0, 1])
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


def test_vectorised_projector_columns_are_the_references():
    """the columns the GPU tests expand with, against the scalar spinless and the spinful reference of the sector tests"""
    case = R.Case(8, 4, gens=F.translations(8), secs=[1])
    reps, _ = F.representatives(8, 4, case.group)
    assert np.array_equal(reps, case.reps)
    states, B = F.projector_columns(8, 4, case.group, reps)
    assert np.array_equal(states, case.states) and np.abs(case.columns.toarray() - B).max() <= 1e-14
    case = R.Case(8, None, gens=F.dihedral(8), secs=[0, 1])
    reps, _ = F.representatives(8, -1, case.group)
    states, B = F.projector_columns(8, -1, case.group, reps)
    assert np.array_equal(reps, case.reps) and np.abs(case.columns.toarray() - B).max() <= 1e-14
    case = R.Case(6, up=(3, 3), gens=F.translations(6), secs=[2], flip=-1)
    reps, _ = FS.representatives(6, 3, 3, case.group)
    states, B = FS.projector_columns(6, 3, 3, case.group, reps)
    assert np.array_equal(reps, case.reps) and np.array_equal(states, case.states)
    assert abs(case.columns - B).max() <= 1e-14
    assert (~case.live).any() or len(case.reps) * len(case.group) >= len(case.states)
    # an isometry, and the unprojected basis is the identity
    G = (case.columns.conj().T @ case.columns).toarray()
    assert np.abs(G - np.eye(len(case.reps))).max() <= 1e-13
    assert abs(case.plain().columns - np.eye(400)).max() == 0.0


def test_reference_entropy_of_free_fermions_needs_sigma():
    """the numpy reference alone: with sigma the entropy of M is Peschel's, without it a scattered subsystem is off"""
    case = R.Case(10, 5)
    model = F.tv_model(R.JW.ring(10))
    _, psi = case.ground_state(model)
    for a, off in (([0, 2, 5, 7], True), ([1, 4, 6], True), ([0, 1, 2, 3], False)):
        want = R.peschel_entropy(R.ring_hopping(10), 5, a)
        got = R.entropy(R.spectrum(R.bipartition(case, psi, a))[0])
        bare = R.entropy(R.spectrum(R.bipartition(case, psi, a, signed=False))[0])
        assert abs(got - want) <= 1e-12, (a, got, want)
        assert (abs(bare - want) > 0.1) == off, (a, bare, want)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_fermi_expand_create\s*\(\s*ls_amd_expand\s*\*\*\s*\w+\s*,\s*ls_hs_basis\s+const\s*\*\s*\w+\s*,\s*uint64_t\s+const"
                     r"\s*\*\s*d_reps\s*,\s*int64_t\s+n\s*,\s*uint64_t\s+mode_mask\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"int\s+ls_amd_test_fermi_split_parity\s*\(\s*uint64_t\s+mode_mask_a\s*,\s*int\s+modes\s*,\s*uint64_t\s+state\s*\)\s*;", header)
    L = _lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert hasattr(L, name), name
    from distributed_matvec_amd import entanglement

    for name in ("FermionSectorExpansion", "fermion_unproject"):
        assert callable(getattr(D, name)) and getattr(D, name) is getattr(entanglement, name) and name in D.__all__ and name in entanglement.__all__
    for name in ("expand", "check", "destroy", "kernel"):
        assert hasattr(D.FermionSectorExpansion, name)
    assert "max_bytes" in D.FermionSectorExpansion.expand.__code__.co_varnames
    for fn in (D.reduced_density_matrix, D.entanglement_spectrum):
        assert "modes" in fn.__code__.co_varnames
    mk = open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile")).read()
    assert "k_expand_fermi.hip" in mk and "k_expand.hip" in mk
