"""The block Gram-Schmidt entry points (csrc/orth_block.hip) without a device: declared and exported, bad sizes and strides refused
with -1 and a message before anything launches, and the compiler's resource report: the expected kernels, no scratch, and the
occupancy the grid is sized for."""
import ctypes as C
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "ls_amd.h")).read()
    assert re.search(r"int\s+ls_amd_orth_block_pass\s*\(\s*int\s+m\s*,\s*int\s+K\s*,\s*int64_t\s+n\s*,\s*double\s+const\s*\*\s*\w+\s*,"
                     r"\s*int64_t\s+ldv\s*,\s*double\s*\*\s*\w+\s*,\s*int64_t\s+ldw\s*,\s*double\s+const\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*stream\s*\)", header)
    assert re.search(r"int\s+ls_amd_block_rotate\s*\(\s*int\s+m_in\s*,\s*int\s+m_out\s*,\s*int64_t\s+n\s*,", header)
    assert re.search(r"int\s+ls_amd_orth_block_max_rows\s*\(\s*void\s*\)", header)
    from distributed_matvec_amd import _lib

    L = _lib.load()
    for name in ("ls_amd_orth_block_pass", "ls_amd_block_rotate", "ls_amd_orth_block_max_rows"):
        assert hasattr(L, name), name
    assert L.ls_amd_orth_block_max_rows() == 128


def test_bad_arguments_are_refused_without_a_device():
    from distributed_matvec_amd import _lib

    L = _lib.load()
    fake = C.c_void_p(64)  # never dereferenced: the checks come first
    n = 100
    for m, K, nn, ldv, ldw in ((-1, 4, n, n, n), (129, 4, n, n, n), (4, 0, n, n, n), (4, 17, n, n, n), (4, 4, -5, n, n),
                               (4, 4, n, n - 1, n), (4, 4, n, n, n - 1), (0, 4, n, 0, n - 1)):
        rc = L.ls_amd_orth_block_pass(m, K, nn, fake, ldv, fake, ldw, None, fake, None)
        assert rc == -1, (m, K, nn, ldv, ldw)
        msg = L.ls_amd_last_error().decode()
        assert "ls_amd_orth_block_pass: bad arguments" in msg and f"m = {m}" in msg and f"K = {K}" in msg, msg
    for m_in, m_out, nn, ldv in ((0, 1, n, n), (129, 4, n, n), (4, 5, n, n), (4, 0, n, n), (4, 4, n, n - 1), (4, 4, -1, n)):
        assert L.ls_amd_block_rotate(m_in, m_out, nn, fake, ldv, fake, None) == -1, (m_in, m_out, nn, ldv)
        assert "ls_amd_block_rotate: bad arguments" in L.ls_amd_last_error().decode()


def test_kernels_in_the_resource_report():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    import sys

    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources

    st = kernel_resources.resources(source="orth_block.hip")
    passes = {k: v for k, v in st.items() if k.startswith("_Z17k_orth_block_passI")}
    rotates = {k: v for k, v in st.items() if k.startswith("_Z14k_block_rotateI")}
    assert len(passes) == 4 and len(rotates) == 2 and len(st) == 6, sorted(st)  # {update, none} x {aligned, not} + rotate x 2
    for name, v in st.items():
        assert v["scratch"] == 0 and v["occ"] >= 4, (name, v)
        assert v["lds"] * 4 <= 160 * 1024, (name, v)  # four workgroups per CU: the grid the host launches
