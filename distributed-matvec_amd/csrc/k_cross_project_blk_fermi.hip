// k_cross_project_blk_fermi.hip -- the block form of the projecting cross-sector kernel with a projected FERMIONIC basis on either side
// (spinless; spinful over their 2 L modes): the k_cross_project_blk template of k_cross_project_blk_t.hpp with its FERMI switch on, as
// k_cross_project_fermi.hip is to k_cross_project.  The same 8 kinds as k_cross_project_blk.hip, in a translation unit of their own.
// DESIGN.md sections 6b, 6h.
#include "k_cross_project_blk_t.hpp"

// the name of the family in plans and reports: k_cross_project_blk<W, PM1, CPLX, REAL, TPM1, FERMI = true>
extern "C" char const *lsk_cross_project_blk_fermi_kernel_name(void) { return "k_cross_project_blk_fermi"; }

// lsk_cross_project_blk for src.fermi || dst.fermi (same arguments; reached through it).  The refusals are those of
// lsk_cross_project_fermi: the sign table and the table's key width bound every shift and load of stage B1.
extern "C" int lsk_cross_project_blk_fermi(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src,
                                           lsk_index six, lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps,
                                           double const *dst_norms, int K, void const *x, int64_t x_row, int64_t x_col, void *y,
                                           int64_t y_row, int64_t y_col, double tiny, int *d_err, void *stream) {
    if (!src.fermi && !dst.fermi) { snprintf(g_err, sizeof(g_err), "%s: neither basis is a projected fermionic one", __func__); return -1; }
    if (src.fermi && (!src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL)) {
        snprintf(g_err, sizeof(g_err), "%s: the source is not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (dst.fermi && (!dst.fsign || dst.spin_inversion != 0)) {
        snprintf(g_err, sizeof(g_err), "%s: the target is not a projected fermionic basis with a sign table", __func__);
        return -1;
    }
    if (K < 1 || K > 64) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, 64]", __func__, K); return -1; }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (src.fermi && (!gt.entries || gt.L != src.number_sites)) {
        snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__);
        return -1;
    }
    return cross_project_blk_launch<true>(__func__, n_groups, groups, terms, is_real, src, six, gt, dst, cplx, n_dst, dst_reps, dst_norms, K,
                                          x, x_row, x_col, y, y_row, y_col, tiny, d_err, stream);
}
