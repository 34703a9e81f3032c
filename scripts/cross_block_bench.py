#!/usr/bin/env python3
"""What the block form of the cross-sector product buys: CrossSectorPlan.apply_block on an interleaved (n, K) block (k_cross_pull_blk,
k_cross_pull_blk_fermi) against K calls of CrossSectorPlan.apply on contiguous columns of the same plan (k_cross_pull,
k_cross_pull_fermi: the single-vector kernel, which repeats stages A, B1 and the look-up for every column), on the two plans that
scripts/cross_sector_bench.py and scripts/fermion_cross_bench.py time:
  spin      S^z_q on heisenberg_chain_32 with translations, k = 0 -> q (default 5)
  fermion   c+_q on the 28-mode t-V ring (V = 1) with translations, N = 14, k = 0 -> N = 15, k = q (default 5)
c128, device events, 1 warm-up and 3 timed runs of each, alternating in one process; min-max.  --thermal adds one
evolve.thermal_correlation run on the spin pair (K random vectors, a few output times, bounds [-3 L, L] by the norm of the bonds,
so that no Lanczos run is timed) with the share of the time spent in apply_block.  One JSON line per record, appended to --out.
usage: cross_block_bench.py [--which spin|fermion|both] [--sites 32] [--modes 28] [--q 5] [--K 8] [--steps 3] [--warmup 1] [--thermal]
                            [--out profiles/cross_block_bench.jsonl]"""
import argparse
import cmath
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config, evolve  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--which", default="both", choices=["spin", "fermion", "both"])
ap.add_argument("--sites", type=int, default=32)
ap.add_argument("--modes", type=int, default=28)
ap.add_argument("--q", type=int, default=5)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--thermal", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
K = args.K
dtype = torch.complex128
torch.cuda.set_device(0)


def phase(L, q, j):
    z = cmath.exp(-2j * math.pi * q * j / L)
    return "(" + repr(z.real) + ("+" if z.imag >= 0 else "-") + repr(abs(z.imag)) + "j)"


def translation(L, k):
    return [{"permutation": [(i + 1) % L for i in range(L)], "sector": k}]


def spin_ring(L, k):
    cfg = config.heisenberg_chain_config(L)
    cfg["basis"]["symmetries"] = translation(L, k)
    return cfg


def sz_q(L, q):
    return {"terms": [{"expression": phase(L, q, j) + " σᶻ₀", "sites": [[j]]} for j in range(L)]}


def fermi_ring(L, n, k):
    return {"basis": {"particle": "spinless-fermion", "number_sites": L, "number_particles": n, "symmetries": translation(L, k)}}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


def block_against_columns(head, src_cfg, dst_cfg, op_cfg):
    t0 = time.perf_counter()
    sbasis = D.loadConfigFromDict(src_cfg)
    tbasis = D.loadConfigFromDict(dst_cfg)
    A = D.Operator.fromSpec(sbasis, config.parse_operator(op_cfg, sbasis.spec))
    sreps, _ = D.enumerateStates(sbasis, 1)
    treps, _ = D.enumerateStates(tbasis, 1)
    cross = D.CrossSectorPlan(A, sreps[0], tbasis, treps[0], dtype)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    n1, n2 = int(sreps[0].numel()), int(treps[0].numel())
    cols = [D.fillRandom(sreps[0], 1 + k, dtype) for k in range(K)]           # K contiguous columns ...
    x = torch.stack(cols, dim=1).contiguous()                                  # ... and the same numbers interleaved
    y = torch.zeros((n2, K), dtype=dtype, device="cuda")
    outs = [torch.zeros(n2, dtype=dtype, device="cuda") for _ in range(K)]

    def do_block():
        cross.apply_block(x, y, check=False)

    def do_columns():
        for k in range(K):
            cross.apply(cols[k], outs[k], check=False)

    for _ in range(args.warmup):
        do_block()
        do_columns()
    cross.check()
    diff = max(float((y[:, k] - outs[k]).abs().max()) for k in range(K))
    size = max(float(o.abs().max()) for o in outs)
    tb, tc = [], []
    for _ in range(args.steps):  # alternating
        tb.append(timed(do_block))
        tc.append(timed(do_columns))
    cross.check()
    tb.sort()
    tc.sort()
    slower = tb[0] > tc[-1]  # beyond the min-max spread of the timed runs
    emit({**head, "dtype": "c128", "K": K, "layout": "interleaved", "n_source": n1, "n_target": n2, "cross_nnz": cross.nnz,
          "block_kernel": cross.block_kernel(K), "column_kernel": cross.kernel, "steps": args.steps, "warmup": args.warmup,
          "block_ms_min": round(tb[0], 4), "block_ms_max": round(tb[-1], 4), "columns_ms_min": round(tc[0], 4), "columns_ms_max": round(tc[-1], 4),
          "block_over_columns_min": round(tb[0] / tc[-1], 4), "block_over_columns_max": round(tb[-1] / tc[0], 4),
          "block_is_slower": bool(slower), "max_abs_difference": diff, "max_abs_y": size, "setup_seconds": round(setup_s, 2)})
    cross.destroy()


def thermal(L, q):
    """one thermal_correlation on the spin pair with every apply_block bracketed by device events"""
    events = []
    inner = D.CrossSectorPlan.apply_block

    def bracketed(self, x, y, check=True, method=None):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(self, x, y, check=check, method=method)
        e1.record()
        events.append((e0, e1))

    cfg = spin_ring(L, 0)
    cfg["observables"] = [sz_q(L, q)]
    times = [0.0, 0.05, 0.1, 0.15]
    D.CrossSectorPlan.apply_block = bracketed
    try:
        torch.cuda.synchronize()
        res = evolve.thermal_correlation(cfg, 0, 0.1, times, num_vectors=K, seed=1, target=spin_ring(L, q)["basis"],
                                         bounds=(-3.0 * L - 0.5, L + 0.5))
        torch.cuda.synchronize()
    finally:
        D.CrossSectorPlan.apply_block = inner
    apply_ms = sum(e0.elapsed_time(e1) for e0, e1 in events)
    emit({"record": "thermal_correlation", "model": f"heisenberg_chain_{L}", "symmetries": "translation", "operator": "S^z_q", "source_sector": 0,
          "target_sector": q, "K": K, "beta": 0.1, "times": times, "dimension": res.dimension, "bounds": list(res.bounds),
          "orders": [int(n) for n in res.orders], "matvec_columns": res.matvec_columns, "kernel": res.kernel,
          "apply_block_calls": len(events), "apply_block_ms": round(apply_ms, 3), "seconds": round(res.seconds, 3),
          "apply_block_share": round(apply_ms / (1e3 * res.seconds), 5),
          "correlation_real": [float(c.real) for c in res.correlation], "correlation_imag": [float(c.imag) for c in res.correlation]})


if args.which in ("spin", "both"):
    L, q = args.sites, args.q % args.sites
    block_against_columns({"record": "block_against_columns", "model": f"heisenberg_chain_{L}", "symmetries": "translation", "operator": "S^z_q",
                           "source_sector": 0, "target_sector": q}, {"basis": spin_ring(L, 0)["basis"]}, {"basis": spin_ring(L, q)["basis"]}, sz_q(L, q))
if args.which in ("fermion", "both"):
    L, q = args.modes, args.q % args.modes
    N = L // 2
    op = {"terms": [{"expression": phase(L, q, j) + " × c†₀", "sites": [[j]]} for j in range(L)]}
    block_against_columns({"record": "block_against_columns", "model": f"tV_ring_{L}", "symmetries": "translation", "operator": "c+_q",
                           "source_particles": N, "target_particles": N + 1, "source_sector": 0, "target_sector": q},
                          fermi_ring(L, N, 0), fermi_ring(L, N + 1, q), op)
if args.thermal:
    thermal(args.sites, args.q % args.sites)
