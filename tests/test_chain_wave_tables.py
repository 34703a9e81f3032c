"""Word tables behind the wave headers of the staged row kernel (host.c: chain_wave_tables), through the host-only hook
ls_amd_test_chain_wave_tables.  No device needed."""
import ctypes as C
from math import comb

import numpy as np
import pytest

from distributed_matvec_amd import _lib


def _tables(low_site):
    L = _lib.load()
    U = np.zeros(4096, dtype=np.uint16)
    Rg = np.zeros(4096, dtype=np.uint16)
    off = np.zeros(14, dtype=np.int32)
    rc = L.ls_amd_test_chain_wave_tables(low_site, U.ctypes.data_as(C.POINTER(C.c_uint16)), Rg.ctypes.data_as(C.POINTER(C.c_uint16)),
                                         off.ctypes.data_as(C.POINTER(C.c_int)))
    assert rc == 0
    return U, Rg, off


def _weight(w):
    return bin(int(w)).count("1")


def test_words_grouped_by_weight_ascending():
    """U lists, for every weight k, exactly the C(12, k) words of that weight in ascending order"""
    U, _, off = _tables(0)
    assert off[0] == 0 and off[13] == 4096
    for k in range(13):
        assert off[k + 1] - off[k] == comb(12, k), k
        want = np.array([w for w in range(4096) if _weight(w) == k], dtype=np.uint16)
        assert np.array_equal(U[off[k]:off[k + 1]], want), k


@pytest.mark.parametrize("low_site", [0, 5])
def test_partner_rank_inside_its_class(low_site):
    """Rg[low] = rank of low ^ bit inside its own weight class, for all 4096 words"""
    U, Rg, off = _tables(low_site)
    rank = {}
    for k in range(13):
        for r, w in enumerate(w for w in range(4096) if _weight(w) == k):
            rank[w] = r
    want = np.array([rank[w ^ (1 << low_site)] for w in range(4096)], dtype=np.uint16)
    assert np.array_equal(Rg, want)
    # and the table agrees with itself: the partner word sits at its class start + Rg
    for w in range(4096):
        p = w ^ (1 << low_site)
        assert U[off[_weight(p)] + Rg[w]] == p


def test_low_site_out_of_range_is_refused():
    L = _lib.load()
    buf = np.zeros(4096, dtype=np.uint16)
    off = np.zeros(14, dtype=np.int32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint16))
    assert L.ls_amd_test_chain_wave_tables(12, p, p, off.ctypes.data_as(C.POINTER(C.c_int))) != 0
