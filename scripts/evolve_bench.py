#!/usr/bin/env python3
"""One order of the Chebyshev propagator, Y <- alpha H X + beta X + gamma Y ; Z += c Y with the two dots, in three forms on the same
plan and blocks:
  a  MatvecPlan.matvec_block_axpby_acc under LS_AMD_BLOCK=auto, LS_AMD_ACC=fused (k_direct_evolve / k_pull_gather_evolve / epilogue
     with k_axpby_acc)
  s  the same under LS_AMD_ACC=split: the Chebyshev kernel of the path, then one accumulate pass of k_axpby_acc (the epilogue path
     has one form: s repeats a there)
  b  MatvecPlan.matvec_block_axpby, then the cheapest torch accumulate that is correct for the type pair:
       f64 -> c128   view_as_real(z)[..., 0].add_(y, alpha=c_re); view_as_real(z)[..., 1].add_(y, alpha=c_im)   (no complex copy of y)
       c128 -> c128  z.add_(y, alpha=c)
       f64 -> f64    z.add_(y, alpha=c_re)
Form b is what a caller composes without the fused step and is the baseline.  The forms alternate inside one process; every shape
is warmed up; each step is timed by device events; before anything is timed the two forms must agree on Y, Z and the dots.  One JSON
line per case and form: median, min, max ms over --steps (min..max is the run-to-run spread the comparison is read against).
Cases (model:dtype:K): chain_32:f64:1 (epilogue path), chain_36_symm:f64:8 (gather path), hubbard_chain_16_pairhop:f64:8 (direct
path).  --propagate adds, per case, one evolve.propagate of the block at a t = 100: order N, wall seconds.
usage: evolve_bench.py [--cases model:dtype:K,...] [--steps 10] [--warmup 2] [--propagate] [--out profiles/evolve_bench.jsonl]"""
import argparse
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config, evolve, kpm  # noqa: E402
from distributed_matvec_amd.diagonalize import LocalOperator  # noqa: E402


def model(name):
    m = re.fullmatch(r"chain_(\d+)(_symm)?", name)
    if m:
        return config.heisenberg_chain_config(int(m.group(1)), symm=bool(m.group(2)))
    m = re.fullmatch(r"hubbard_chain_(\d+)_pairhop", name)
    if m:
        L = int(m.group(1))
        cfg = config.hubbard_config(L, [(i, (i + 1) % L) for i in range(L)], t=1.0, U=4.0)
        cfg["hamiltonian"]["terms"] += [{"expression": "0.5 × c†₀↑ c†₀↓ c₁↓ c₁↑", "sites": [[0, L // 2]]},
                                        {"expression": "0.5 × c†₁↑ c†₁↓ c₀↓ c₀↑", "sites": [[0, L // 2]]}]
        return cfg
    raise SystemExit(f"unknown model {name}")


ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="chain_32:f64:1,chain_36_symm:f64:8,hubbard_chain_16_pairhop:f64:8")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--ztype", default="c128", help="accumulator of the f64 cases: c128 (real time) or f64 (imaginary time)")
ap.add_argument("--propagate", action="store_true")
ap.add_argument("--out", default=None, help="append the JSON lines here as well")
args = ap.parse_args()
torch.cuda.set_device(0)
os.environ.pop("LS_AMD_BLOCK", None)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
out = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


for case in [c for c in args.cases.split(",") if c]:
    name, dt, K = case.split(":")
    K = int(K)
    dtype = torch.complex128 if dt == "c128" else torch.float64
    zdtype = torch.float64 if (dt == "f64" and args.ztype == "f64") else torch.complex128
    t0 = time.perf_counter()
    basis, h = D.loadConfigFromDict(model(name), hamiltonian=True)
    reps, _ = D.enumerateStates(basis, 1)
    op = LocalOperator(h, reps, dtype)
    pl = op.plan
    n = reps[0].numel()
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    x = (torch.rand((n, K), dtype=torch.float64, device="cuda") - 0.5).to(dtype)
    y0 = (torch.rand((n, K), dtype=torch.float64, device="cuda") - 0.5).to(dtype)
    z0 = (torch.rand((n, K), dtype=torch.float64, device="cuda") - 0.5).to(zdtype)
    y, z = y0.clone(), z0.clone()
    dots = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
    al, be, ga = 0.25, -0.1, -1.0
    c = 0.7 if zdtype == torch.float64 else -0.3 + 1.1j

    def form_a():
        pl.matvec_block_axpby_acc(x, y, al, be, ga, z, c, dots=dots, check=False)

    def form_b():
        pl.matvec_block_axpby(x, y, al, be, ga, dots=dots, check=False)
        if zdtype == dtype:
            z.add_(y, alpha=c)
        else:
            zr = torch.view_as_real(z)
            zr[..., 0].add_(y, alpha=c.real)
            zr[..., 1].add_(y, alpha=c.imag)

    def form_s():
        os.environ["LS_AMD_ACC"] = "split"
        form_a()

    def form_f():
        os.environ["LS_AMD_ACC"] = "fused"
        form_a()

    forms = {"a": form_f, "s": form_s, "b": form_b}
    form_b()  # the two forms agree before anything is timed
    ref_y, ref_z, ref_dots = y.clone(), z.clone(), dots.clone()
    sy, sz = float(ref_y.abs().max()), float(ref_z.abs().max())
    for f in "as":
        y.copy_(y0)
        z.copy_(z0)
        forms[f]()
        assert float((ref_y - y).abs().max()) <= 1e-12 * max(1.0, sy), f"Y of form {f} differs"
        assert float((ref_z - z).abs().max()) <= 1e-12 * max(1.0, sz), f"Z of form {f} differs"
        assert torch.allclose(dots, ref_dots, rtol=1e-10, atol=0), f"dots of form {f} differ"
    pl.check()
    del ref_y, ref_z, ref_dots
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    ts = {f: [] for f in forms}
    for _ in range(args.steps):  # alternating: a b a b ...
        for f, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[f].append(e0.elapsed_time(e1))
    pl.check()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(torch.view_as_real(z) if z.is_complex() else z).all())
    paths = {"b": pl.axpby_kernel(K) + " + torch"}
    for f in "as":
        os.environ["LS_AMD_ACC"] = "fused" if f == "a" else "split"
        paths[f] = pl.acc_kernel(K)
    os.environ.pop("LS_AMD_ACC", None)
    for f in forms:
        t = sorted(ts[f])
        emit({"model": name, "N": n, "dtype": dt, "z_dtype": "c128" if zdtype == torch.complex128 else "f64", "K": K, "kernel": pl.kernel,
              "form": f, "path": paths[f], "steps": len(t),
              "ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3), "setup_seconds": round(setup_s, 2)})
    del y, z, y0, z0
    if args.propagate:
        t1 = time.perf_counter()
        bounds = kpm.spectral_bounds(op)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        a = 0.5 * (bounds[1] - bounds[0])
        info = {}
        psi = evolve.propagate(op, x, 100.0 / a, bounds=bounds, _info=info)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        n0, n1 = torch.linalg.vector_norm(x, dim=0), torch.linalg.vector_norm(psi, dim=0)
        emit({"model": name, "N": n, "dtype": dt, "K": K, "driver": "propagate", "path": pl.acc_kernel(K), "a_t": 100.0, "bounds": list(bounds),
              "order": info["order"], "seconds_bounds": round(t2 - t1, 3), "seconds_propagate": round(t3 - t2, 3),
              "norm_defect": float(((n1 - n0).abs() / n0).max())})
        del psi
    del x, op, pl, reps, basis, h
    torch.cuda.empty_cache()
