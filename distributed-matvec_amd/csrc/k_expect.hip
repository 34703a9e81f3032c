// k_expect.hip -- expectation values of arbitrary operators on a sector state (ls_amd_expect, host.c): the raw
// sums R[u] over the representatives alone for every unique device term of a batch, which the host combines into the group averages.
//   k_expect  the row kernel (k_expect_t.hpp); this unit holds the 6 instantiations without permutation signs, and lsk_expect hands a
//             projected fermionic basis to the signed ones of k_expect_fermi.hip.
// The partial sums of the blocks are added by k_corr_sum (k_corr.hip), in ascending block order.
#include "k_expect_t.hpp"

extern "C" char const *lsk_expect_kernel_name(void) { return "k_expect"; }

extern "C" int lsk_expect(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                          lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                          double const *norms, void const *psi, double *partial, double *out, int *d_err, void *stream) {
    if (bs.fermi)
        return lsk_expect_fermi(bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, psi, partial, out, d_err, stream);
    return expect_launch<false>(bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, psi, partial, out, d_err, stream);
}
