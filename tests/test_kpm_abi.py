"""Chebyshev step (ls_amd_matvec_block_axpby, ls_amd_plan_axpby_kernel_name, ls_amd_block_axpby_dots) without a device: the C ABI is
declared and exported, argument errors come back as -1 with a message, and the kernels of csrc/k_cheb.hip are in the compiler's
resource report within the budget of the block kernels they mirror."""
import ctypes as C
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_matvec_block_axpby", "ls_amd_plan_axpby_kernel_name", "ls_amd_block_axpby_dots")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_matvec_block_axpby\s*\(\s*ls_amd_plan\s*\*\s*\w+\s*,\s*int\s+K\s*,[^;]*double\s+alpha\s*,\s*double\s+beta\s*,"
                     r"\s*double\s+gamma\s*,\s*double\s*\*\s*d_dots\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"char\s+const\s*\*\s*ls_amd_plan_axpby_kernel_name\s*\(\s*ls_amd_plan\s+const\s*\*\s*\w+\s*,\s*int\s+K\s*\)", header)
    assert re.search(r"int\s+ls_amd_block_axpby_dots\s*\(\s*int\s+cplx\s*,\s*int64_t\s+n\s*,\s*int\s+K\s*,", header)
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    import distributed_matvec_amd as D
    from distributed_matvec_amd import kpm

    assert callable(D.block_axpby_dots) and callable(D.MatvecPlan.matvec_block_axpby) and callable(D.MatvecPlan.axpby_kernel)
    for name in ("chebyshev_moments", "spectral_bounds", "reconstruct", "density_of_states", "spectral_function", "KpmResult"):
        assert hasattr(kpm, name), name


def _vp(a):
    return C.cast(a, C.c_void_p)


def test_null_plan_and_bad_k_are_refused_without_a_device():
    L = _lib()
    x = (C.c_double * 8)()
    y = (C.c_double * 8)()
    assert L.ls_amd_matvec_block_axpby(None, 2, _vp(x), 2, 1, _vp(y), 2, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "NULL" in L.ls_amd_last_error().decode()
    assert L.ls_amd_plan_axpby_kernel_name(None, 4) is None
    assert "NULL" in L.ls_amd_last_error().decode()
    fake = C.c_void_p(8)  # a non-NULL handle with K out of range: refused before the plan is dereferenced
    for K in (0, 65, -3):
        assert L.ls_amd_matvec_block_axpby(fake, K, _vp(x), 1, 1, _vp(y), 1, 1, 1.0, 0.0, 0.0, None, None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_plan_axpby_kernel_name(fake, K) is None
        assert "[1, 64]" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_axpby_dots(0, 4, K, _vp(x), 1, 4, _vp(x), 1, 4, _vp(y), 1, 4, 1.0, 0.0, 0.0, None, None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode()


def test_epilogue_refuses_bad_strides_and_overlap_without_a_device():
    L = _lib()
    w = (C.c_double * 16)()
    x = (C.c_double * 16)()
    y = (C.c_double * 16)()
    ok = (2, 1)  # 4 rows x 2 columns, interleaved
    call = lambda W, ws, X, xs, Y, ys: L.ls_amd_block_axpby_dots(0, 4, 2, _vp(W), ws[0], ws[1], _vp(X), xs[0], xs[1], _vp(Y), ys[0], ys[1],  # noqa: E731
                                                                  1.0, 0.0, 0.0, None, None)
    for bad in ((1, 1), (2, 3), (-2, 1), (1, 2)):  # two elements on one word, or not nested
        for which in range(3):
            strides = [ok, ok, ok]
            strides[which] = bad
            assert call(w, strides[0], x, strides[1], y, strides[2]) == -1, (bad, which)
            msg = L.ls_amd_last_error().decode()
            assert "share" in msg and "WXY"[which] in msg, msg
    assert call(w, ok, x, ok, x, ok) == -1 and "X and Y overlap" in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, w, ok) == -1 and "W and Y overlap" in L.ls_amd_last_error().decode()
    # interleaved halves of one buffer: the address ranges overlap
    big = (C.c_double * 32)()
    second = C.c_void_p(C.addressof(big) + 16)
    assert L.ls_amd_block_axpby_dots(0, 4, 2, _vp(w), 2, 1, _vp(big), 4, 1, second, 4, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "overlap" in L.ls_amd_last_error().decode()
    assert L.ls_amd_block_axpby_dots(0, 4, 2, None, 2, 1, _vp(x), 2, 1, _vp(y), 2, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "NULL" in L.ls_amd_last_error().decode()


def test_the_two_layouts_every_block_entry_refuses_without_a_device():
    """row stride 1, column stride 1 at K = 4, and the interleaved halves of one buffer: the stride rule and the overlap rule are one
    pair of helpers behind every block entry point, and these are the two cases their GPU tests ask of the entries that need a live
    plan (ls_amd_matvec_block in test_gpu_block_matvec.py, ls_amd_matvec_block_axpby in test_gpu_kpm.py, ls_amd_cross_apply_block in
    test_gpu_cross_block.py); here through the entry that needs none"""
    L = _lib()
    w = (C.c_double * 16)()
    x = (C.c_double * 16)()
    y = (C.c_double * 16)()
    for which in range(3):
        strides = [(4, 1), (4, 1), (4, 1)]
        strides[which] = (1, 1)
        (wr, wc), (xr, xc), (yr, yc) = strides
        assert L.ls_amd_block_axpby_dots(0, 4, 4, _vp(w), wr, wc, _vp(x), xr, xc, _vp(y), yr, yc, 1.0, 0.0, 0.0, None, None) == -1
        msg = L.ls_amd_last_error().decode()
        assert "share storage" in msg and "(row 1, column 1)" in msg and f"of {'WXY'[which]} " in msg and "4 x 4 block" in msg, msg
    big = (C.c_double * 32)()
    second = C.c_void_p(C.addressof(big) + 4 * 8)  # X = big[:, :4], Y = big[:, 4:] of a 4 x 8 interleaved buffer
    assert L.ls_amd_block_axpby_dots(0, 4, 4, _vp(w), 4, 1, _vp(big), 8, 1, second, 8, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "X and Y overlap" in L.ls_amd_last_error().decode()
    assert L.ls_amd_block_axpby_dots(0, 4, 4, _vp(big), 8, 1, _vp(x), 4, 1, second, 8, 1, 1.0, 0.0, 0.0, None, None) == -1
    assert "W and Y overlap" in L.ls_amd_last_error().decode()


def _stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    return kernel_resources.resources(source="k_cheb.hip")


def test_cheb_kernels_in_the_resource_report():
    stats = _stats()
    direct = {k: v for k, v in stats.items() if k.startswith("_Z13k_direct_chebI")}
    gather = {k: v for k, v in stats.items() if k.startswith("_Z18k_pull_gather_chebI")}
    epilogue = {k: v for k, v in stats.items() if k.startswith("_Z12k_axpby_dotsI")}
    assert len(direct) == 8, sorted(direct)  # {f64, c128} x {identity, combinadic, search, product}: those of k_direct_blk
    assert len(gather) == 2, sorted(gather)  # {f64, c128}
    assert len(epilogue) == 6, sorted(epilogue)  # c128 x {rows, columns}; f64 x {scalar, 16-byte} x {rows, columns}
    assert len(stats) == 16, sorted(stats)  # nothing else in the unit
    for name, v in stats.items():
        assert v["scratch"] == 0, (name, v)
        # the admitted-blocks rule of test_hot_kernel_register_budget: the SGPR file must not admit fewer blocks than LDS and VGPRs
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (name, v)
    for name, v in direct.items():  # persistent grid sized by the occupancy API: keep it where the API is right
        assert v["sgpr"] <= 80 and v["occ"] == 8, (name, v)

