"""Block matvec (ls_amd_matvec_block) without a device: the C ABI is declared and exported, argument errors come back as -1 with a
message, and the two block kernels are in the compiler's resource report within the register budget of the row kernels."""
import ctypes as C
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_block_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_matvec_block\s*\(\s*ls_amd_plan\s*\*\s*\w+\s*,\s*int\s+K\s*,", header)
    assert re.search(r"char\s+const\s*\*\s*ls_amd_plan_block_kernel_name\s*\(\s*ls_amd_plan\s+const\s*\*\s*\w+\s*,\s*int\s+K\s*\)", header)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    for name in ("ls_amd_matvec_block", "ls_amd_plan_block_kernel_name"):
        assert hasattr(L, name), name


def test_null_plan_and_bad_k_are_refused_without_a_device():
    from distributed_matvec_amd import _lib

    L = _lib.load()
    x = (C.c_double * 4)()
    y = (C.c_double * 4)()
    rc = L.ls_amd_matvec_block(None, 2, C.cast(x, C.c_void_p), 2, 1, C.cast(y, C.c_void_p), 2, 1, None)
    assert rc == -1
    assert "NULL" in L.ls_amd_last_error().decode()
    assert L.ls_amd_plan_block_kernel_name(None, 4) is None
    assert "NULL" in L.ls_amd_last_error().decode()
    # a non-NULL handle with K = 0 / 65: refused before the plan is dereferenced
    fake = C.c_void_p(8)
    for K in (0, 65, -3):
        assert L.ls_amd_matvec_block(fake, K, C.cast(x, C.c_void_p), 1, 1, C.cast(y, C.c_void_p), 1, 1, None) == -1
        assert f"K = {K}" in L.ls_amd_last_error().decode()
        assert L.ls_amd_plan_block_kernel_name(fake, K) is None
        assert "[1, 64]" in L.ls_amd_last_error().decode()


def _stats():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    return kernel_resources.resources()


def test_block_kernels_in_the_resource_report():
    stats = _stats()
    direct = {k: v for k, v in stats.items() if k.startswith("_Z12k_direct_blkI")}
    gather = {k: v for k, v in stats.items() if k.startswith("_Z17k_pull_gather_blkI")}
    assert len(direct) == 8, sorted(direct)  # {f64, c128} x {identity, combinadic, search, product}
    assert len(gather) == 2, sorted(gather)  # {f64, c128}
    assert len(stats) <= 300
    for name, v in {**direct, **gather}.items():
        assert v["scratch"] == 0, (name, v)
        # the admitted-blocks rule of test_hot_kernel_register_budget: the SGPR file must not admit fewer blocks than LDS and VGPRs
        by_sgpr = 800 // (-(-v["sgpr"] // 16) * 16 + 16)
        by_lds = (160 * 1024) // v["lds"] if v["lds"] else 8
        assert by_sgpr >= min(by_lds, v["occ"], 8), (name, v)
    for name, v in direct.items():  # persistent grid sized by the occupancy API: keep it where the API is right
        assert v["sgpr"] <= 80 and v["occ"] == 8, (name, v)
