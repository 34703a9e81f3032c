// k_fermi.hip -- projected fermionic bases (spinless; spinful with fixed (N_up, N_down) over their 2 L modes): the K4 of every group
// element carries the permutation sign of the Fock state (lsk_fermi.hpp).  Enumeration flags (the spinful product candidates are in
// k_fermi_product.hip), norms, state_info, and the fermionic instantiations of the indexed pull kernel k_pull_t (k_pull_t.hpp) for
// one-partition plans: fused f64 / c128 and the resolve half of the split matvec, 32- and 64-bit words.  The gather kernels
// (k_pull_gather, k_pull_gather_blk) need nothing new: the sign is folded into each packet's coefficient.
// A translation unit of its own so that the hot units (scripts/kernel_resources.py) keep their device-function budget.
#include "k_pull_t.hpp"

extern "C" int lsk_test_fermi_parity(lsk_group_elem e, uint64_t const *tab, uint64_t a, int L, int table) {
    return fermi_parity<uint64_t>(e, tab, a, L, table != 0);
}
// host mirror of fermi_apply_elem_w for the LIFT kinds (host_apply_elem, host.c, has the others)
extern "C" uint64_t lsk_test_fermi_apply_lift(lsk_group_elem e, uint64_t x, int L) {
    return fermi_apply_lift<uint64_t>(e, x, L, L >= 64 ? ~0ULL : ((1ULL << L) - 1));
}

// k_enum_flags (k_plan.hip) with the signed test: a candidate is kept when it is its orbit minimum AND its norm does not vanish
__global__ __launch_bounds__(kBlock) void k_fermi_enum_flags(lsk_basis bs, lsk_group_elem const *__restrict__ elems,
                                                             uint64_t const *__restrict__ g_binom, int64_t n_cand, int64_t n_threads,
                                                             int chunk, uint64_t *__restrict__ flags, int64_t *__restrict__ counts) {
    __shared__ uint64_t s_binom[64 * LSK_BINOM_K];
    load_binom(s_binom, g_binom);
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n_threads; t += (int64_t)gridDim.x * kBlock) {
        const int64_t c0 = t * chunk;
        const int64_t c1 = c0 + chunk < n_cand ? c0 + chunk : n_cand;
        uint64_t s = bs.hamming_weight >= 0 ? unrank_combinadic(c0, bs.hamming_weight, s_binom) : (uint64_t)c0;
        uint64_t m = 0;
        for (int64_t c = c0; c < c1; ++c) {
            if (fermi_is_representative(bs, elems, s)) m |= 1ULL << (c - c0);
            if (c + 1 < c1) s = (bs.hamming_weight > 0) ? next_fixed_hamming(s) : s + 1;
        }
        flags[t] = m;
        counts[t] = __popcll(m);
    }
}
extern "C" int lsk_fermi_enum_flags(lsk_basis bs, uint64_t const *d_binom, int64_t n_cand, int64_t n_threads, int chunk, uint64_t *flags,
                                    int64_t *counts, void *stream) {
    if (!bs.fermi || !bs.fsign || bs.spin_inversion != 0 || chunk < 1 || chunk > 64) {
        snprintf(g_err, sizeof(g_err), "lsk_fermi_enum_flags: not a projected fermionic basis");
        return -1;
    }
    if (n_threads <= 0) return 0;
    hipLaunchKernelGGL(k_fermi_enum_flags, dim3(grid_for(n_threads)), dim3(kBlock), 0, (hipStream_t)stream, bs, bs.elems, d_binom, n_cand,
                       n_threads, chunk, flags, counts);
    LSK_LAUNCH_CHECK();
    return 0;
}

__global__ __launch_bounds__(kBlock) void k_fermi_state_info(lsk_basis bs, lsk_group_elem const *__restrict__ elems, int64_t n,
                                                             uint64_t const *__restrict__ alphas, uint64_t *__restrict__ betas,
                                                             double *__restrict__ chars, double *__restrict__ norms) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        uint64_t rep;
        double chr, chi, stab;
        if (bs.chars_pm1) fermi_state_info_w<uint64_t, true>(bs, elems, alphas[i], rep, chr, chi, stab);
        else fermi_state_info_w<uint64_t, false>(bs, elems, alphas[i], rep, chr, chi, stab);
        const double n2 = stab * bs.inv_order;
        if (betas) {
            betas[i] = rep;
            chars[2 * i] = chr;
            chars[2 * i + 1] = chi;
        }
        norms[i] = n2 > 1e-12 ? sqrt(n2) : 0.0;
    }
}
static int fermi_args_ok(lsk_basis const &bs, char const *who) {
    if (bs.fermi && bs.fsign && bs.spin_inversion == 0 && bs.k4_mode == 0 && bs.proj == LSK_PROJ_FULL) return 0;
    snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", who);
    return -1;
}
extern "C" int lsk_fermi_state_info(lsk_basis bs, int64_t n, uint64_t const *alphas, uint64_t *betas, double *characters, double *norms,
                                    void *stream) {
    if (fermi_args_ok(bs, "lsk_fermi_state_info") != 0) return -1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_fermi_state_info, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, bs, bs.elems, n, alphas, betas,
                       characters, norms);
    LSK_LAUNCH_CHECK();
    return 0;
}
// the plan's per-row norms: state_info without the representative and character outputs
extern "C" int lsk_fermi_norms(lsk_basis bs, int64_t n, uint64_t const *reps, double *norms, void *stream) {
    if (fermi_args_ok(bs, "lsk_fermi_norms") != 0) return -1;
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_fermi_state_info, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, bs, bs.elems, n, reps, nullptr,
                       nullptr, norms);
    LSK_LAUNCH_CHECK();
    return 0;
}

// the (K4, coefficient) kinds pull_kinds gives a fermionic basis: FERMI_PM1 with real or complex coefficients, FERMI (complex
// characters) with complex ones; fused over f64 (real coefficients only) or c128, or the resolve half (x-free)
template <typename W, bool CPLX, int SINK>
static int fermi_dispatch(lsk_operator const &op, lsk_basis const &bs, int64_t row0, int64_t row1, uint64_t const *reps, double const *norms_local,
                          lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global, void const *xsrc, int halo, void *y, lsk_pullbuf buf,
                          int *d_err, hipStream_t s) {
    int k4m, coef;
    pull_kinds(op, bs, k4m, coef);
#define LSK_FP(K4M, COEF) launch_pull_t<W, K4M, COEF, CPLX, SINK>(op, bs, row0, row1, reps, norms_local, ix, reps_global, n_global, xsrc, halo, y, buf, d_err, s)
    if (coef == COEF_CPLX) {
        if constexpr (!CPLX && SINK == SINK_FUSED) { snprintf(g_err, sizeof(g_err), "lsk_tile_pull: complex coefficients need c128 vectors"); return -1; }
        else { if (k4m == K4_FERMI_PM1) LSK_FP(K4_FERMI_PM1, COEF_CPLX); else LSK_FP(K4_FERMI, COEF_CPLX); }
    } else if (coef == COEF_REAL && k4m == K4_FERMI_PM1) LSK_FP(K4_FERMI_PM1, COEF_REAL);
    else { snprintf(g_err, sizeof(g_err), "lsk_fermi_pull: no kernel for K4 kind %d with coefficient kind %d", k4m, coef); return -1; }
#undef LSK_FP
    return 0;
}
extern "C" int lsk_fermi_pull(lsk_operator op, lsk_basis bs, int wide, int cplx, int sink, int64_t row0, int64_t row1, uint64_t const *reps,
                              double const *norms_local, lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global, void const *xsrc, int halo,
                              void *y, lsk_pullbuf buf, int *d_err, void *stream) {
    if (fermi_args_ok(bs, "lsk_fermi_pull") != 0) return -1;
    if (ix.vtab || ix.perm || (sink != SINK_FUSED && sink != SINK_RESOLVE) || (sink == SINK_RESOLVE && cplx)) {
        snprintf(g_err, sizeof(g_err), "lsk_fermi_pull: fermionic bases run the fused and the resolve kernel of one partition only");
        return -1;
    }
    if (wide != (bs.number_sites > 32)) { snprintf(g_err, sizeof(g_err), "lsk_fermi_pull: word width does not match the basis"); return -1; }
    hipStream_t s = (hipStream_t)stream;
    int rc;
#define LSK_FA op, bs, row0, row1, reps, norms_local, ix, reps_global, n_global, xsrc, halo, y, buf, d_err, s
    if (sink == SINK_RESOLVE) rc = wide ? fermi_dispatch<uint64_t, false, SINK_RESOLVE>(LSK_FA) : fermi_dispatch<uint32_t, false, SINK_RESOLVE>(LSK_FA);
    else if (wide) rc = cplx ? fermi_dispatch<uint64_t, true, SINK_FUSED>(LSK_FA) : fermi_dispatch<uint64_t, false, SINK_FUSED>(LSK_FA);
    else rc = cplx ? fermi_dispatch<uint32_t, true, SINK_FUSED>(LSK_FA) : fermi_dispatch<uint32_t, false, SINK_FUSED>(LSK_FA);
#undef LSK_FA
    if (rc != 0) return -1;
    LSK_LAUNCH_CHECK();
    return 0;
}
