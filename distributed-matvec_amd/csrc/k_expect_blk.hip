// k_expect_blk.hip -- expectation values of arbitrary operators on the K columns of a block of sector states,
// ls_amd_expect_values_block (host.c): the raw sums R[u][c] over the representatives alone for every unique
// device term u of a batch and every column c, which the host combines into the group averages column by column.  The kernel is the
// template of k_expect_blk_t.hpp -- the stages of k_expect once per chunk of 8 columns; this unit holds its 6 instantiations without
// permutation signs (FERMI = false), and lsk_expect_blk hands a projected fermionic basis to the signed ones of
// k_expect_blk_fermi.hip.  The partial sums of the blocks are added by k_corr_sum (k_corr.hip), in ascending block order.
#include "k_expect_blk_t.hpp" // the k_expect_blk template, shared with k_expect_blk_fermi.hip

extern "C" char const *lsk_expect_blk_kernel_name(void) { return "k_expect_blk"; }

extern "C" int lsk_expect_blk(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                              lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                              double const *norms, int K, void const *psi, int64_t p_row, int64_t p_col, double *partial, double *out,
                              int *d_err, void *stream) {
    if (bs.fermi)
        return lsk_expect_blk_fermi(bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, K, psi, p_row, p_col,
                                    partial, out, d_err, stream);
    return expect_blk_launch<false>(__func__, bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, K, psi, p_row,
                                    p_col, partial, out, d_err, stream);
}
