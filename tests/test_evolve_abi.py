"""Accumulate step of Chebyshev time evolution (ls_amd_matvec_block_axpby_acc, ls_amd_plan_acc_kernel_name, ls_amd_block_axpby_acc)
without a device: the C ABI is declared and exported, argument errors come back as -1 with a message that names the argument, and
the kernels of csrc/k_evolve.hip are in the compiler's resource report within the budget of the kernels they mirror."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ls_amd_matvec_block_axpby_acc", "ls_amd_plan_acc_kernel_name", "ls_amd_block_axpby_acc")


def _lib():
    from distributed_matvec_amd import _lib as L

    return L.load()


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_matvec_block_axpby_acc\s*\(\s*ls_amd_plan\s*\*\s*\w+\s*,\s*int\s+K\s*,[^;]*double\s+alpha\s*,\s*double\s+beta\s*,"
                     r"\s*double\s+gamma\s*,\s*void\s*\*\s*d_z\s*,\s*int64_t\s+z_row\s*,\s*int64_t\s+z_col\s*,\s*int\s+z_cplx\s*,\s*double\s+c_re\s*,"
                     r"\s*double\s+c_im\s*,\s*double\s*\*\s*d_dots\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert re.search(r"char\s+const\s*\*\s*ls_amd_plan_acc_kernel_name\s*\(\s*ls_amd_plan\s+const\s*\*\s*\w+\s*,\s*int\s+K\s*\)", header)
    assert re.search(r"int\s+ls_amd_block_axpby_acc\s*\(\s*int\s+cplx\s*,\s*int\s+z_cplx\s*,\s*int64_t\s+n\s*,\s*int\s+K\s*,", header)
    L = _lib()
    for name in NAMES:
        assert hasattr(L, name), name
    import distributed_matvec_amd as D

    assert callable(D.block_axpby_acc) and callable(D.MatvecPlan.matvec_block_axpby_acc) and callable(D.MatvecPlan.acc_kernel)
    for name in ("bessel_series", "propagator_coefficients", "propagate", "autocorrelation", "EvolveResult"):
        assert hasattr(D, name), name
    assert callable(D.evolve.evolve)
    assert "k_evolve.hip" in open(os.path.join(ROOT, "distributed-matvec_amd", "csrc", "Makefile")).read()


def _vp(a):
    return C.cast(a, C.c_void_p)


def test_null_plan_and_bad_k_are_refused_without_a_device():
    L = _lib()
    x, y, z = ((C.c_double * 8)() for _ in range(3))
    assert L.ls_amd_matvec_block_axpby_acc(None, 2, _vp(x), 2, 1, _vp(y), 2, 1, 1.0, 0.0, 0.0, _vp(z), 2, 1, 0, 1.0, 0.0, None, None) == -1
    assert "NULL" in L.ls_amd_last_error().decode()
    assert L.ls_amd_plan_acc_kernel_name(None, 4) is None
    assert "NULL" in L.ls_amd_last_error().decode()
    fake = C.c_void_p(8)  # a non-NULL handle with K out of range: refused before the plan is dereferenced
    for K in (0, 65, -3):
        assert L.ls_amd_matvec_block_axpby_acc(fake, K, _vp(x), 1, 1, _vp(y), 1, 1, 1.0, 0.0, 0.0, _vp(z), 1, 1, 0, 1.0, 0.0, None, None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_plan_acc_kernel_name(fake, K) is None
        assert "[1, 64]" in L.ls_amd_last_error().decode()
        assert L.ls_amd_block_axpby_acc(0, 0, 4, K, _vp(x), 1, 4, _vp(x), 1, 4, _vp(y), 1, 4, _vp(z), 1, 4, 1.0, 0.0, 0.0, 1.0, 0.0, None,
                                        None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode()
    assert L.ls_amd_block_axpby_acc(0, 0, -1, 2, _vp(x), 2, 1, _vp(x), 2, 1, _vp(y), 2, 1, _vp(z), 2, 1, 1.0, 0.0, 0.0, 1.0, 0.0, None, None) == -1
    assert "negative" in L.ls_amd_last_error().decode()


def test_epilogue_refuses_bad_z_strides_overlap_and_types_without_a_device():
    L = _lib()
    w, x, y = ((C.c_double * 16)() for _ in range(3))
    z = (C.c_double * 32)()  # room for 4 x 2 c128 elements
    ok = (2, 1)  # 4 rows x 2 columns, interleaved

    def call(W, ws, X, xs, Y, ys, Z, zs, cplx=0, z_cplx=0, c_im=0.0):
        return L.ls_amd_block_axpby_acc(cplx, z_cplx, 4, 2, _vp(W) if W is not None else None, ws[0], ws[1], _vp(X), xs[0], xs[1], _vp(Y), ys[0],
                                        ys[1], _vp(Z) if Z is not None else None, zs[0], zs[1], 1.0, 0.0, 0.0, 0.7, c_im, None, None)

    for bad in ((1, 1), (2, 3), (-2, 1), (1, 2)):  # two elements on one word, or not nested
        for which in range(4):
            strides = [ok, ok, ok, ok]
            strides[which] = bad
            assert call(w, strides[0], x, strides[1], y, strides[2], z, strides[3]) == -1, (bad, which)
            msg = L.ls_amd_last_error().decode()
            assert "share" in msg and f"of {'WXYZ'[which]} " in msg, msg
        assert call(w, ok, x, ok, y, ok, z, bad, z_cplx=1, c_im=0.2) == -1 and "of Z " in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, y, ok, None, ok) == -1 and "Z is NULL" in L.ls_amd_last_error().decode()
    assert call(None, ok, x, ok, y, ok, z, ok) == -1 and "NULL" in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, y, ok, y, ok) == -1 and "Z and Y overlap" in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, y, ok, x, ok) == -1 and "Z and X overlap" in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, y, ok, w, ok) == -1 and "Z and W overlap" in L.ls_amd_last_error().decode()
    assert call(w, ok, x, ok, x, ok, z, ok) == -1 and "X and Y overlap" in L.ls_amd_last_error().decode()
    # a c128 Z is twice as long as the f64 blocks: its second half alone reaches into Y
    big = (C.c_double * 32)()
    y_in_z = C.c_void_p(C.addressof(big) + 8 * 10)
    assert L.ls_amd_block_axpby_acc(0, 1, 4, 2, _vp(w), 2, 1, _vp(x), 2, 1, y_in_z, 2, 1, _vp(big), 2, 1, 1.0, 0.0, 0.0, 0.7, 0.2, None, None) == -1
    assert "Z and Y overlap" in L.ls_amd_last_error().decode()
    # the types: an f64 Z takes a real c only, and c128 vectors a c128 Z only
    assert call(w, ok, x, ok, y, ok, z, ok, z_cplx=0, c_im=0.2) == -1
    msg = L.ls_amd_last_error().decode()
    assert "z_cplx" in msg and "c_im" in msg, msg
    assert call(w, ok, x, ok, y, ok, z, ok, cplx=1, z_cplx=0) == -1
    msg = L.ls_amd_last_error().decode()
    assert "z_cplx" in msg and "c128" in msg, msg


def _stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    return kernel_resources.resources(source="k_evolve.hip")


def test_evolve_kernels_in_the_resource_report():
    stats = _stats()
    direct = {k: v for k, v in stats.items() if k.startswith("_Z15k_direct_evolveI")}
    gather = {k: v for k, v in stats.items() if k.startswith("_Z20k_pull_gather_evolveI")}
    epilogue = {k: v for k, v in stats.items() if k.startswith("_Z11k_axpby_accI")}
    # (X / Y, Z) in {(f64, f64), (f64, c128), (c128, c128)} x {identity, combinadic, search, product}
    assert len(direct) == 12, sorted(direct)
    assert len(gather) == 3, sorted(gather)
    # c128 x {rows, columns}; f64 x Z in {f64, c128} x {scalar, 16-byte} x {rows, columns}
    assert len(epilogue) == 10, sorted(epilogue)
    assert len(stats) == 25, sorted(stats)  # nothing else in the unit
    for name, v in stats.items():
        assert v["scratch"] == 0, (name, v)
        # the admitted-blocks rule of test_hot_kernel_register_budget: the SGPR file must not admit fewer blocks than LDS and VGPRs
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (name, v)
    for name, v in direct.items():  # persistent grid sized by the occupancy API: keep it where the API is right
        assert v["sgpr"] <= 80, (name, v)


def test_design_lists_exactly_the_kernels_of_the_unit():
    """the table of DESIGN.md section 6b names every instantiation (demangled template arguments) with its reported resources"""
    stats = _stats()
    names = subprocess.run(["c++filt"], input="\n".join(stats), capture_output=True, text=True).stdout.split("\n")
    have = {}
    for (_, v), dn in zip(stats.items(), names):
        short = re.sub(r"^void ", "", dn.split("(")[0]).replace("(lsk_index_kind)", "")
        have[short] = v
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    rows = re.findall(r"^\| `(k_(?:direct_evolve|pull_gather_evolve|axpby_acc)<[^`]*>)` \| (\d+) \| (\d+) \| (\d+) \| (\d+) \| (\d+) \|$", design, re.M)
    listed = {r[0]: tuple(int(q) for q in r[1:]) for r in rows}
    assert sorted(listed) == sorted(have), (sorted(set(have) ^ set(listed)))
    for name, v in have.items():
        assert listed[name] == (v["sgpr"], v["vgpr"], v["occ"], v["scratch"], v["lds"]), (name, listed[name], v)
