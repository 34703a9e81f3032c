// k_project_fermi.hip -- projection of full-basis vectors into a sector of a fermionic basis (ls_amd_project, host.c; DESIGN.md section
// 6g): k_project_pull_fermi, the pull counterpart of k_expand_push_fermi.
//     psi[r] = (|G| n(r))^-1 sum_g chi(g) sign(g, r) Phi[index(g r)],     U_g |r> = sign(g, r) |g r>  (fermi_parity, lsk_fermi.hpp)
// A basis without a group has the identity alone and no sign table.  No spin inversion: fermionic bases have none (the up <-> down
// flip of a spinful basis is a group element, LSK_ELEM_LIFT_SWAP).  Layouts: ALL (no fixed number), FIXED, and PRODUCT -- the spinful
// (N_up, N_down) basis, index = rank(down half) C(L, N_up) + rank(up half), the order of lsk_enumerate_product.  The body, the lane
// mapping and the bounds are in k_project_t.hpp.
#include "k_project_t.hpp"

extern "C" char const *lsk_project_fermi_kernel_name(void) { return "k_project_pull_fermi"; }

template <typename W, bool PM1, bool CPLX, int KIND, int KT>
__global__ __launch_bounds__(kBlock) void k_project_pull_fermi(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_project pj,
                                                               uint64_t const *__restrict__ g_binom, int64_t n,
                                                               uint64_t const *__restrict__ reps, double const *__restrict__ norms,
                                                               double const *__restrict__ phi, double *__restrict__ out, int *err) {
    __shared__ uint64_t s_binom[KIND != PJ_ALL ? 64 * LSK_BINOM_K : 1];
    if (KIND != PJ_ALL) load_binom(s_binom, g_binom); // (synchronises the block)
    pj_block<W, PM1, CPLX, KIND, true, KT>(bs, elems, pj, s_binom, n, reps, norms, phi, out, err);
}

extern "C" int lsk_project_pull_fermi(lsk_basis bs, lsk_project pj, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                                      double const *norms, void const *phi, void *out, int *d_err, void *stream) {
    if (n <= 0) return 0;
    if (bs.spin_inversion != 0 || (bs.fermi && !bs.fsign) || (!bs.fermi && bs.n_elems != 1)) {
        snprintf(g_err, sizeof(g_err), "%s: not a fermionic basis (a group without its sign table, or a spin inversion)", __func__);
        return -1;
    }
    if (!pj_args_ok(__func__, bs, pj, cplx)) return -1;
    const int M = bs.number_sites;
    bool ok;
    if (pj.kind == PJ_FIXED) ok = bs.hamming_weight >= 0 && bs.hamming_weight < LSK_BINOM_K;
    else if (pj.kind == PJ_PRODUCT)
        ok = bs.hamming_weight < 0 && M == 2 * pj.half && pj.half >= 1 && pj.half <= 32 && pj.n_up >= 0 && pj.n_up <= pj.half && pj.n_dn >= 0 &&
             pj.n_dn <= pj.half && pj.n_low >= 1;
    else ok = pj.kind == PJ_ALL && bs.hamming_weight < 0 && M <= 40 && pj.full == ((int64_t)1 << M);
    if (!ok) { snprintf(g_err, sizeof(g_err), "%s: the layout does not belong to the basis", __func__); return -1; }
    const int KT = pj.K == 1 ? 1 : kProjectCols;
    const dim3 g = pj_grid(n, pj.K, KT), b(kBlock);
    hipStream_t s = (hipStream_t)stream;
#define LSK_PJF_ARGS bs, bs.elems, pj, d_binom, n, reps, norms, (double const *)phi, (double *)out, d_err
#define LSK_PJF_KIND(W, PM1, CPLX, KIND)                                                                                                  \
    do {                                                                                                                                  \
        if (KT == 1) hipLaunchKernelGGL((k_project_pull_fermi<W, PM1, CPLX, KIND, 1>), g, b, 0, s, LSK_PJF_ARGS);                         \
        else hipLaunchKernelGGL((k_project_pull_fermi<W, PM1, CPLX, KIND, kProjectCols>), g, b, 0, s, LSK_PJF_ARGS);                      \
    } while (0)
#define LSK_PJF_ONE(W, PM1, CPLX)                                                                                                         \
    do {                                                                                                                                  \
        if (pj.kind == PJ_FIXED) LSK_PJF_KIND(W, PM1, CPLX, PJ_FIXED);                                                                    \
        else if (pj.kind == PJ_PRODUCT) LSK_PJF_KIND(W, PM1, CPLX, PJ_PRODUCT);                                                           \
        else LSK_PJF_KIND(W, PM1, CPLX, PJ_ALL);                                                                                          \
    } while (0)
    // {32, 64-bit words} x {f64 | c128 x {+-1, complex characters}} x {all states, fixed number, product} x {1, 8 columns}: 36 kernels
#define LSK_PJF_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                  \
        if (!cplx) LSK_PJF_ONE(W, true, false);                                                                                           \
        else if (bs.chars_pm1) LSK_PJF_ONE(W, true, true);                                                                                \
        else LSK_PJF_ONE(W, false, true);                                                                                                 \
    } while (0)
    if (M <= 32) LSK_PJF_LAUNCH(uint32_t); else LSK_PJF_LAUNCH(uint64_t);
#undef LSK_PJF_LAUNCH
#undef LSK_PJF_ONE
#undef LSK_PJF_KIND
#undef LSK_PJF_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
