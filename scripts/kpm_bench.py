#!/usr/bin/env python3
"""One Chebyshev step Y <- alpha H X + beta X + gamma Y with <X|X> and <X|Y> per column, in three forms on the same plan and blocks:
  a  MatvecPlan.matvec_block_axpby under LS_AMD_BLOCK=auto (k_direct_cheb / k_pull_gather_cheb / epilogue)        3 or 6 words
  b  matvec_block into a scratch block, then block_axpby_dots (one hand-written epilogue pass)                   6 words
  c  matvec_block, then torch in-place ops (y *= gamma; y += alpha w; y += beta x) and torch.linalg.vecdot twice   13 words
(streamed 8- or 16-byte words per row and column next to the partner gathers, which all three pay alike).  Form c is what a caller
composes without this entry point and is the baseline of every time quoted.  The forms alternate inside one process; every shape
is warmed up; each step is timed by device events.  One JSON line per case and form: median, min, max ms over --steps.
Cases: chain_36_symm f64 K = 8 and c128 K = 4, hubbard_chain_16_pairhop f64 K = 8, chain_32 f64 K = 1 and K = 4.
--dos adds the end-to-end figure: density_of_states of chain_36_symm, M = 512, K = 8.
usage: kpm_bench.py [--cases name:dtype:K,...] [--steps 10] [--warmup 2] [--dos] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config, kpm  # noqa: E402

WORDS = {"k_direct_cheb": 3, "k_pull_gather_cheb": 3, "epilogue": 6}


def model(name):
    if name == "chain_36_symm":
        return config.heisenberg_chain_config(36, symm=True)
    if name == "hubbard_chain_16_pairhop":
        cfg = config.hubbard_config(16, [(i, (i + 1) % 16) for i in range(16)], t=1.0, U=4.0)
        cfg["hamiltonian"]["terms"] += [{"expression": "0.5 × c†₀↑ c†₀↓ c₁↓ c₁↑", "sites": [[0, 8]]},
                                        {"expression": "0.5 × c†₁↑ c†₁↓ c₀↓ c₀↑", "sites": [[0, 8]]}]
        return cfg
    if name == "chain_32":
        return config.heisenberg_chain_config(32)
    raise SystemExit(f"unknown model {name}")


ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="chain_36_symm:f64:8,chain_36_symm:c128:4,hubbard_chain_16_pairhop:f64:8,chain_32:f64:1,chain_32:f64:4")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dos", action="store_true")
ap.add_argument("--out", default=None, help="append the JSON lines here as well")
args = ap.parse_args()
torch.cuda.set_device(0)
os.environ.pop("LS_AMD_BLOCK", None)
out = open(args.out, "a") if args.out else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


plans = {}
for case in [c for c in args.cases.split(",") if c]:
    name, dt, K = case.split(":")
    K = int(K)
    dtype = torch.complex128 if dt == "c128" else torch.float64
    if (name, dt) not in plans:
        plans.clear()
        torch.cuda.empty_cache()
        basis, h = D.loadConfigFromDict(model(name), hamiltonian=True)
        reps, _ = D.enumerateStates(basis, 1)
        plans[(name, dt)] = (D.MatvecPlan(h, reps, dtype), reps, h)
    pl, reps, _ = plans[(name, dt)]
    n = reps[0].numel()
    x = (torch.rand((n, K), dtype=torch.float64, device="cuda") - 0.5).to(dtype)
    y0 = (torch.rand((n, K), dtype=torch.float64, device="cuda") - 0.5).to(dtype)
    y, w = y0.clone(), torch.empty_like(x)
    dots = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
    al, be, ga = 0.25, -0.1, -1.0

    def form_a():
        pl.matvec_block_axpby(x, y, al, be, ga, dots=dots, check=False)

    def form_b():
        pl.matvec_block(x, w, check=False)
        D.block_axpby_dots(w, x, y, al, be, ga, dots=dots)

    def form_c():
        pl.matvec_block(x, w, check=False)
        y.mul_(ga)
        y.add_(w, alpha=al)
        y.add_(x, alpha=be)
        dots[:K] = torch.linalg.vecdot(x, x, dim=0).real
        dots[K:] = torch.linalg.vecdot(x, y, dim=0).real

    forms = {"a": form_a, "b": form_b, "c": form_c}
    y.copy_(y0)  # the three forms agree before anything is timed
    form_c()
    ref_y, ref_dots = y.clone(), dots.clone()
    scale = float(ref_y.abs().max())
    for f in "ab":
        y.copy_(y0)
        forms[f]()
        y.sub_(ref_y)
        assert float(y.abs().max()) <= 1e-12 * max(1.0, scale), f
        assert torch.allclose(dots, ref_dots, rtol=1e-10, atol=0), f
    pl.check()
    del ref_y, ref_dots
    for _ in range(args.warmup):
        for fn in forms.values():
            fn()
    ts = {f: [] for f in forms}
    for _ in range(args.steps):  # alternating: a b c a b c ...
        for f, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[f].append(e0.elapsed_time(e1))
    pl.check()
    path = pl.axpby_kernel(K)
    for f in forms:
        t = sorted(ts[f])
        emit({"model": name, "N": n, "dtype": dt, "K": K, "kernel": pl.kernel, "form": f, "path": path if f == "a" else pl.block_kernel(K),
              "words_per_row_and_column": {"a": WORDS[path], "b": 6, "c": 13}[f], "steps": len(t), "ms_median": round(t[len(t) // 2], 3),
              "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3)})
    del x, y, y0, w
plans.clear()
torch.cuda.empty_cache()

if args.dos:
    t0 = time.perf_counter()
    E, rho, res = kpm.density_of_states(model("chain_36_symm"), num_moments=512, num_vectors=8, seed=0)
    emit({"model": "chain_36_symm", "driver": "density_of_states", "M": 512, "K": 8, "path": res.kernel, "bounds": list(res.bounds),
          "matvec_columns": res.matvec_columns, "seconds_wall": round(time.perf_counter() - t0, 3),
          "seconds_in_steps": round(res.step_seconds, 3)})
