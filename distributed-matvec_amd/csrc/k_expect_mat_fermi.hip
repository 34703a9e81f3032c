// k_expect_mat_fermi.hip -- the matrix-element kernel on projected FERMIONIC bases (spinless; spinful over their 2 L modes): the
// k_expect_mat template of k_expect_mat_t.hpp with its FERMI switch on, so that stage B1 projects every image with the signed
// characters chi(g) sign(g, a) of lsk_fermi.hpp, as k_expect_blk_fermi does for one block.  The same 6 kinds as k_expect_mat.hip.
// DESIGN.md section 6j.
#include "k_expect_mat_t.hpp"

// the name of the family in plans and reports: k_expect_mat<W, PM1, CPLX, FERMI = true>
extern "C" char const *lsk_expect_mat_fermi_kernel_name(void) { return "k_expect_mat_fermi"; }

// lsk_expect_mat for bs.fermi (same arguments; reached through it).  The basis is always projected, so always looked up in its static
// index table: the sign table and the table's key width bound every shift and load of the kernel.
extern "C" int lsk_expect_mat_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups,
                                    lsk_expect_group const *groups, lsk_expect_term const *terms, int term0, int n_terms, int cplx,
                                    int64_t n, uint64_t const *reps, double const *norms, int Ka, void const *phi, int64_t a_row,
                                    int64_t a_col, int Kb, void const *psi, int64_t k_row, int64_t k_col, double *partial, double *out,
                                    int *d_err, void *stream) {
    if (!bs.fermi || !bs.fsign || bs.spin_inversion != 0 || bs.k4_mode != 0 || bs.proj != LSK_PROJ_FULL) {
        snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (n > 0 && n_groups > 0 && n_terms > 0 && (!gt.entries || gt.L != bs.number_sites)) {
        snprintf(g_err, sizeof(g_err), "%s: a projected fermionic basis is looked up in its static index table", __func__);
        return -1;
    }
    return expect_mat_launch<true>(__func__, bs, six, gt, cons, n_groups, groups, terms, term0, n_terms, cplx, n, reps, norms, Ka, phi, a_row,
                                   a_col, Kb, psi, k_row, k_col, partial, out, d_err, stream);
}
