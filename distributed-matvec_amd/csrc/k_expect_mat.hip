// k_expect_mat.hip -- matrix elements of arbitrary operators between the columns of two blocks of sector states,
// ls_amd_expect_matrix_elements (host.c): the raw sums R[u][a][b] over the representatives alone for every
// unique device term u of a batch, every bra column a and every ket column b, which the host combines into the group averages pair
// by pair.  The kernel is the template of k_expect_mat_t.hpp -- the stages of k_expect once per chunk of 8 bra x 8 ket columns; this
// unit holds its 6 instantiations without permutation signs (FERMI = false), and lsk_expect_mat hands a projected fermionic basis to
// the signed ones of k_expect_mat_fermi.hip.  The partial sums of the blocks are added by k_corr_sum (k_corr.hip), in ascending
// block order.
#include "k_expect_mat_t.hpp" // the k_expect_mat template, shared with k_expect_mat_fermi.hip

extern "C" char const *lsk_expect_mat_kernel_name(void) { return "k_expect_mat"; }

extern "C" int lsk_expect_mat(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                              lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                              double const *norms, int Ka, void const *phi, int64_t a_row, int64_t a_col, int Kb, void const *psi,
                              int64_t k_row, int64_t k_col, double *partial, double *out, int *d_err, void *stream) {
    if (bs.fermi)
        return lsk_expect_mat_fermi(bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, Ka, phi, a_row, a_col, Kb,
                                    psi, k_row, k_col, partial, out, d_err, stream);
    return expect_mat_launch<false>(__func__, bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, Ka, phi, a_row,
                                    a_col, Kb, psi, k_row, k_col, partial, out, d_err, stream);
}
