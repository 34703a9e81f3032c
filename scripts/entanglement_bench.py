#!/usr/bin/env python3
"""What one sector-state expansion costs: the Heisenberg ring of --sites sites at half filling with translation symmetry (k = 0),
a vector on its representatives expanded by SectorExpansion (k_expand_push) for A = half chain and for A = every site (unproject),
in f64 and c128 -- 18.8 M representatives to 601 M elements at 32 sites.  Next to each expansion: a hipMemsetAsync over the same
buffer (the write floor; the expansion clears its blocks with one, so its own time contains it) and one matrix-free matvec of H
in the same sector.  Everything alternates inside one process after a warm-up and is timed by device events; medians over --steps.
One JSON line per (dtype, A), appended to --out.
usage: entanglement_bench.py [--sites 32] [--steps 5] [--warmup 1] [--dtypes f64,c128] [--out profiles/entanglement_bench.jsonl]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import _lib, config  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--dtypes", default="f64,c128")
ap.add_argument("--out", default=None)
args = ap.parse_args()
L = args.sites
torch.cuda.set_device(0)
lib = _lib.load()

t0 = time.perf_counter()
cfg = config.heisenberg_chain_config(L)
cfg["basis"]["symmetries"] = [{"permutation": [(i + 1) % L for i in range(L)], "sector": 0}]
basis, h = D.loadConfigFromDict(cfg, hamiltonian=True)
reps, _ = D.enumerateStates(basis, 1)
n = int(reps[0].numel())
torch.cuda.synchronize()
setup_s = time.perf_counter() - t0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731

for dt in args.dtypes.split(","):
    dtype = torch.complex128 if dt == "c128" else torch.float64
    elt = 16 if dt == "c128" else 8
    psi = D.fillRandom(reps[0], 1, dtype)
    plan = D.MatvecPlan(h, reps, dtype)
    y = torch.zeros_like(psi)
    for name, sites in (("half", list(range(L // 2))), ("all", None)):
        ex = D.SectorExpansion(basis, reps[0], sites)
        out = torch.empty(ex.total, dtype=dtype, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def do_expand():
            ex.expand(psi, out=out, max_bytes=None, check=False)

        def do_memset():
            _lib.check(lib.ls_amd_memset(C.c_void_p(out.data_ptr()), 0, ex.total * elt, stream))

        def do_matvec():
            plan.matvec([psi], [y], check=False)

        for _ in range(args.warmup):
            do_expand()
            do_memset()
            do_matvec()
        ex.check()
        plan.check()
        te, tz, tm = [], [], []
        for _ in range(args.steps):  # alternating
            te.append(timed(do_expand))
            tz.append(timed(do_memset))
            tm.append(timed(do_matvec))
        ex.check()
        plan.check()
        do_expand()
        norm_out, norm_psi = float(torch.linalg.vector_norm(out)), float(torch.linalg.vector_norm(psi))
        ms = med(te)
        rec = {"model": f"heisenberg_chain_{L}", "symmetries": "translation", "sector": 0, "dtype": dt, "subsystem": name,
               "n_representatives": n, "elements": ex.total, "blocks": len(ex.blocks), "group_order": basis.groupOrder(),
               "kernel": ex.kernel, "steps": args.steps, "warmup": args.warmup,
               "expand_ms_median": round(ms, 4), "expand_ms_min": round(min(te), 4), "expand_ms_max": round(max(te), 4),
               "elements_per_s": round(ex.total / (ms * 1e-3), 1), "bytes_written_per_s": round(ex.total * elt / (ms * 1e-3), 1),
               "memset_ms_median": round(med(tz), 4), "scatter_ms_median_minus_memset": round(ms - med(tz), 4),
               "matvec_kernel": plan.kernel, "matvec_ms_median": round(med(tm), 4), "expand_over_matvec": round(ms / med(tm), 4),
               "norm_defect": abs(norm_out - norm_psi) / norm_psi, "setup_seconds": round(setup_s, 2)}
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")
        ex.destroy()
        del out
    plan.destroy()
    del psi, y
    torch.cuda.empty_cache()
