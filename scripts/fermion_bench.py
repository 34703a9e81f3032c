#!/usr/bin/env python3
"""Spinful Hubbard models on the species-split row kernel (k_hubbard) against the generic row kernel (LS_AMD_ROW_KERNEL=generic,
k_direct with a searched index):
  hubbard_chain_16     ring, t = 1, U = 4, 8 up 8 down (N = 12870^2 = 165 636 900)
  hubbard_square_4x4   periodic 4 x 4 square lattice at half filling, t = 1, U = 4
Prints one JSON line per (model, dtype, kernel): ms per matvec (HIP events inside the library), off-diagonal non-zeros (counted by
the species plan), and the fraction of the HBM line at compulsory bytes N (2 w + row_bytes) -- x read once, y written once."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import distributed_matvec_amd as D  # noqa: E402
from distributed_matvec_amd import config  # noqa: E402

HBM_TBPS = 8.0  # MI355X HBM3E line


def model(name):
    if name == "hubbard_chain_16":
        return config.hubbard_config(16, [(i, (i + 1) % 16) for i in range(16)], t=1.0, U=4.0)
    if name == "hubbard_square_4x4":
        bonds = []
        for y in range(4):
            for x in range(4):
                bonds += [(4 * y + x, 4 * y + (x + 1) % 4), (4 * y + x, 4 * ((y + 1) % 4) + x)]
        return config.hubbard_config(16, bonds, t=1.0, U=4.0)
    raise SystemExit(f"unknown model {name}")


ap = argparse.ArgumentParser()
ap.add_argument("--models", default="hubbard_chain_16,hubbard_square_4x4")
ap.add_argument("--dtypes", default="f64,c128")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--kernels", default="auto,generic", help="LS_AMD_ROW_KERNEL values, comma-separated")
args = ap.parse_args()
for name in args.models.split(","):
    basis, h = D.loadConfigFromDict(model(name), hamiltonian=True)
    reps, masks = D.enumerateStates(basis, 1)
    n = int(reps[0].numel())
    for dt in args.dtypes.split(","):
        dtype = torch.float64 if dt == "f64" else torch.complex128
        w = 8 if dt == "f64" else 16
        x = [D.fillRandom(reps[0], 42, dtype)]
        y = [torch.zeros_like(x[0])]
        y_ref, nnz, ms_first = None, None, None
        for rk in args.kernels.split(","):
            os.environ["LS_AMD_ROW_KERNEL"] = rk
            pl = D.MatvecPlan(h, reps, dtype, mode="pull")
            if pl.nnz:
                nnz = pl.nnz
            pl.enable_timing(256)
            pl.matvec(x, y)
            pl.matvec(x, y)
            pl.kernel_times_ms()
            for _ in range(args.steps):
                pl.matvec(x, y, check=False)
            pl.check()
            ks = pl.kernel_times_ms()
            ms = sum(ks) / len(ks)
            if y_ref is None:
                y_ref, ms_first = y[0].clone(), ms
            err = float((y[0] - y_ref).abs().max() / y_ref.abs().max())
            compulsory = n * (2 * w + pl.row_bytes)
            print(json.dumps({"model": name, "dtype": dt, "states": n, "nnz_offdiag": nnz, "row_kernel": rk, "kernel": pl.kernel,
                              "ms": ms, "compulsory_gb": compulsory / 1e9, "hbm_fraction": compulsory / (ms * 1e-3) / (HBM_TBPS * 1e12),
                              "speedup_of_first": ms / ms_first, "max_rel_diff_vs_first": err}), flush=True)
            pl.destroy()
        del x, y
        torch.cuda.empty_cache()
    del reps, masks
    torch.cuda.empty_cache()
os.environ.pop("LS_AMD_ROW_KERNEL", None)
