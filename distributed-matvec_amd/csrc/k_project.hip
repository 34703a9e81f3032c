// k_project.hip -- projection of full-basis vectors into a sector of a spin-1/2 basis (ls_amd_project, host.c):
// k_project_pull, the pull counterpart of k_expand_push.  psi[r] = (|G| n(r))^-1 sum_g chi(g) Phi[index(g r)], the flipped image of
// every permutation element with chi(g) inv when the basis has the global inversion.  The body, the lane mapping and the bounds are
// in k_project_t.hpp; the fermionic entry point (orbit signs, product-basis ranking) is k_project_pull_fermi (k_project_fermi.hip).
#include "k_project_t.hpp"

extern "C" char const *lsk_project_kernel_name(void) { return "k_project_pull"; }

template <typename W, bool PM1, bool CPLX, int KIND, int KT>
__global__ __launch_bounds__(kBlock) void k_project_pull(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_project pj,
                                                         uint64_t const *__restrict__ g_binom, int64_t n,
                                                         uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                         double const *__restrict__ phi, double *__restrict__ out, int *err) {
    __shared__ uint64_t s_binom[KIND != PJ_ALL ? 64 * LSK_BINOM_K : 1];
    if (KIND != PJ_ALL) load_binom(s_binom, g_binom); // (synchronises the block)
    pj_block<W, PM1, CPLX, KIND, false, KT>(bs, elems, pj, s_binom, n, reps, norms, phi, out, err);
}

extern "C" int lsk_project_pull(lsk_basis bs, lsk_project pj, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                                double const *norms, void const *phi, void *out, int *d_err, void *stream) {
    if (n <= 0) return 0;
    if (bs.fermi) { snprintf(g_err, sizeof(g_err), "%s: fermionic bases are not projected here (orbit signs: lsk_project_pull_fermi)", __func__); return -1; }
    if (!pj_args_ok(__func__, bs, pj, cplx)) return -1;
    const bool fixed = bs.hamming_weight >= 0;
    if ((fixed && (pj.kind != PJ_FIXED || bs.hamming_weight >= LSK_BINOM_K)) || (!fixed && (pj.kind != PJ_ALL || bs.number_sites > 40))) {
        snprintf(g_err, sizeof(g_err), "%s: the layout does not belong to the basis (a weight beyond the binomial table, or more than 40 sites without one)", __func__);
        return -1;
    }
    const int KT = pj.K == 1 ? 1 : kProjectCols;
    const dim3 g = pj_grid(n, pj.K, KT), b(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSK_PJ_ARGS bs, bs.elems, pj, d_binom, n, reps, norms, (double const *)phi, (double *)out, d_err
#define LSK_PJ_KIND(W, PM1, CPLX, KIND)                                                                                                   \
    do {                                                                                                                                  \
        if (KT == 1) hipLaunchKernelGGL((k_project_pull<W, PM1, CPLX, KIND, 1>), g, b, 0, s, LSK_PJ_ARGS);                                \
        else hipLaunchKernelGGL((k_project_pull<W, PM1, CPLX, KIND, kProjectCols>), g, b, 0, s, LSK_PJ_ARGS);                             \
    } while (0)
#define LSK_PJ_ONE(W, PM1, CPLX)                                                                                                          \
    do {                                                                                                                                  \
        if (fixed) LSK_PJ_KIND(W, PM1, CPLX, PJ_FIXED);                                                                                   \
        else LSK_PJ_KIND(W, PM1, CPLX, PJ_ALL);                                                                                           \
    } while (0)
    // {32, 64-bit words} x {f64 (+-1 characters) | c128 x {+-1, complex characters}} x {fixed weight, all states} x {1, 8 columns}: 24 kernels
#define LSK_PJ_LAUNCH(W)                                                                                                                  \
    do {                                                                                                                                  \
        if (!cplx) LSK_PJ_ONE(W, true, false);                                                                                            \
        else if (bs.chars_pm1) LSK_PJ_ONE(W, true, true);                                                                                 \
        else LSK_PJ_ONE(W, false, true);                                                                                                  \
    } while (0)
    if (bs.number_sites <= 32) LSK_PJ_LAUNCH(uint32_t); else LSK_PJ_LAUNCH(uint64_t);
#undef LSK_PJ_LAUNCH
#undef LSK_PJ_ONE
#undef LSK_PJ_KIND
#undef LSK_PJ_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
