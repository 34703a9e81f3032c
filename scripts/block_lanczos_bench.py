#!/usr/bin/env python3
"""Block Lanczos against lanczos_smallest on the measured models, and the HBM rate of the block Gram-Schmidt sweep.
Appends one JSON line per case to profiles/block_lanczos_bench.jsonl (or --out).

usage: block_lanczos_bench.py sweep [--n N] [--m M] [--K K]
       block_lanczos_bench.py solve --model chain_<L>_symm|hubbard_chain_16 --num-evals E --K K [--cache on|off] [--max-basis B]
K = 1 runs lanczos_smallest (diagonalize's default path); K >= 2 lanczos_block_smallest.  Per case: wall seconds, matvec columns,
seconds in the matvec (timed around every call, synchronised), in orth and in restart (LS_AMD_LANCZOS_PROFILE), restarts,
block_kernel(K), eigenvalues and the largest residual."""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sweep(args, out):
    import ctypes as C

    import torch

    from distributed_matvec_amd import _lib

    lib = _lib.load()
    n, m, K = args.n, args.m, args.K
    V = torch.randn((m, n), dtype=torch.float64, device="cuda")
    W = torch.randn((K, n), dtype=torch.float64, device="cuda")
    H = torch.randn((m, K), dtype=torch.float64, device="cuda") * 1e-3
    o = torch.zeros(m * K + K * K, dtype=torch.float64, device="cuda")
    rec = {"case": "orth_block_pass", "n": n, "m": m, "K": K}
    for name, h, nbytes in (("sweep", None, (m + K) * n * 8), ("sweep_update", H, (m + 2 * K) * n * 8)):
        def run():
            _lib.check(lib.ls_amd_orth_block_pass(m, K, n, C.c_void_p(V.data_ptr()), n, C.c_void_p(W.data_ptr()), n,
                                                  C.c_void_p(h.data_ptr()) if h is not None else None, C.c_void_p(o.data_ptr()), None))
        run()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 10
        a.record()
        for _ in range(reps):
            run()
        b.record()
        torch.cuda.synchronize()
        s = a.elapsed_time(b) / 1e3 / reps
        rec[name + "_ms"] = round(s * 1e3, 3)
        rec[name + "_TBps"] = round(nbytes / s / 1e12, 3)
    # the rotation of a thick restart (m_in -> m_out = m / 2) and of the normalisation (K -> K)
    S = torch.randn((m, m // 2), dtype=torch.float64, device="cuda")
    for name, mi, mo, nbytes in (("rotate", m, m // 2, (m + m // 2) * n * 8), ("rotate_KxK", K, K, 2 * K * n * 8)):
        def run():
            _lib.check(lib.ls_amd_block_rotate(mi, mo, n, C.c_void_p(V.data_ptr()), n, C.c_void_p(S.data_ptr()), None))
        run()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(5):
            run()
        b.record()
        torch.cuda.synchronize()
        s = a.elapsed_time(b) / 1e3 / 5
        rec[name + "_ms"] = round(s * 1e3, 3)
        rec[name + "_TBps"] = round(nbytes / s / 1e12, 3)
    out(rec)


def solve(args, out):
    import numpy as np
    import torch

    import distributed_matvec_amd as D
    from distributed_matvec_amd import config
    from distributed_matvec_amd.diagonalize import LocalOperator, lanczos_block_smallest, lanczos_smallest

    if re.fullmatch(r"chain_\d+_symm", args.model):
        cfg = config.heisenberg_chain_config(int(args.model.split("_")[1]), symm=True)
    elif args.model == "hubbard_chain_16":  # product basis, half filling, N_up = N_down = 8 (k_hubbard / k_direct_blk)
        cfg = config.hubbard_config(16, [(i, (i + 1) % 16) for i in range(16)], t=1.0, U=4.0)
    else:
        raise SystemExit(f"unknown model {args.model}")
    basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    cache = 0
    if args.cache == "on":
        free, _ = torch.cuda.mem_get_info()
        mb = max(args.max_basis, 2 * args.num_evals + 3 * args.K)
        cache = max(0, int(free) - (mb + 2 * args.K + 6) * n * 8 - (5 << 30))
    op = LocalOperator(h, reps, torch.float64, slot_cache_bytes=cache)
    t_mv = [0.0]
    for name in ("matvec", "matvec_block"):
        f = getattr(op, name)

        def timed(*a, _f=f):
            torch.cuda.synchronize()
            t = time.perf_counter()
            _f(*a)
            torch.cuda.synchronize()
            t_mv[0] += time.perf_counter() - t
        setattr(op, name, timed)
    os.environ["LS_AMD_LANCZOS_PROFILE"] = "1"
    buf = io.StringIO()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        if args.K == 1:
            r = lanczos_smallest(op, num_evals=args.num_evals, eps=args.eps, max_basis=args.max_basis)
        else:
            r = lanczos_block_smallest(op, num_evals=args.num_evals, block_size=args.K, eps=args.eps, max_basis=args.max_basis)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    prof = {}
    for line in buf.getvalue().splitlines()[::-1]:
        if "profile" in line:
            prof = {k: float(v) for k, v in re.findall(r"(\w+) ([0-9.]+) s", line)}
            break
    out({"case": "solve", "model": args.model, "n": n, "num_evals": args.num_evals, "K": args.K, "solver": "lanczos_smallest" if args.K == 1 else
         "lanczos_block_smallest", "slot_cache": args.cache, "cached_rows": op.cached_rows, "max_basis": args.max_basis, "eps": args.eps,
         "block_kernel": op.block_kernel(max(args.K, 1)), "wall_s": round(wall, 3), "matvec_columns": r.matvecs,
         "matvec_s": round(t_mv[0], 3), "orth_s": round(prof.get("orth", 0.0) + prof.get("normalise", 0.0), 3),
         "restart_s": round(prof.get("restart", 0.0), 3), "restarts": r.restarts, "converged": r.converged,
         "eigenvalues": [round(e, 10) for e in r.eigenvalues], "max_residual": max(r.residual_norms)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sweep", "solve"])
    ap.add_argument("--n", type=int, default=63068876)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--model", default="chain_36_symm")
    ap.add_argument("--num-evals", type=int, default=8)
    ap.add_argument("--cache", choices=["on", "off"], default="off")
    ap.add_argument("--max-basis", type=int, default=48)
    ap.add_argument("--eps", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_lanczos_bench.jsonl"))
    args = ap.parse_args()

    def out(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    (sweep if args.what == "sweep" else solve)(args, out)


if __name__ == "__main__":
    main()
