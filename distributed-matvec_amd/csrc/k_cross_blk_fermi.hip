// k_cross_blk_fermi.hip -- the block form of the cross-sector kernel between projected FERMIONIC bases: the k_cross_pull_blk template
// of k_cross_blk_t.hpp with its FERMI switch on, so that stage B1 projects every packet into the source basis with the signed
// characters chi(g) sign(g, a) of lsk_fermi.hpp, as k_cross_pull_fermi does for one vector.  The same 10 kinds as k_cross_blk.hip.
// DESIGN.md section 6h.
#include "k_cross_blk_t.hpp"

// the name of the family in plans and reports: k_cross_pull_blk<W, PM1, CPLX, REAL, FERMI = true>
extern "C" char const *lsk_cross_blk_fermi_kernel_name(void) { return "k_cross_pull_blk_fermi"; }

// lsk_cross_pull_blk for src.fermi (same arguments; reached through it).  The source is always projected, so always looked up in its
// static index table: the sign table and the table's key width bound every shift and load of the kernel.
extern "C" int lsk_cross_fermi_pull_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src,
                                        lsk_index six, lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps,
                                        double const *dst_norms, int K, void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row,
                                        int64_t y_col, double tiny, int *d_err, void *stream) {
    if (!src.fermi || !src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL) {
        snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (n_dst > 0 && n_groups > 0 && (!gt.entries || gt.L != src.number_sites)) {
        snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__);
        return -1;
    }
    return cross_blk_launch<true>(__func__, n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, K, x, x_row,
                                  x_col, y, y_row, y_col, tiny, d_err, stream);
}
