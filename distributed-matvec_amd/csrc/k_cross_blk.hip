// k_cross_blk.hip -- cross-sector operators on blocks of vectors: Y[:, k] = A X[:, k] for the K columns of an (n_src, K) block with
// element strides (row, column), ls_amd_cross_apply_block (host.c).  The kernel is the template of k_cross_blk_t.hpp -- the stages of
// k_cross_pull with a tail that gathers a chunk of 8 columns per resolved packet; this unit holds its 10
// instantiations without permutation signs (FERMI = false), and lsk_cross_pull_blk hands a projected fermionic source to the signed
// ones of k_cross_blk_fermi.hip.
#include "k_cross_blk_t.hpp" // the k_cross_pull_blk template, shared with k_cross_blk_fermi.hip

extern "C" char const *lsk_cross_blk_kernel_name(void) { return "k_cross_pull_blk"; }

extern "C" int lsk_cross_pull_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                  lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, int K,
                                  void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny,
                                  int *d_err, void *stream) {
    if (src.fermi)
        return lsk_cross_fermi_pull_blk(n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, K, x, x_row, x_col,
                                        y, y_row, y_col, tiny, d_err, stream);
    if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", __func__); return -1; }
    return cross_blk_launch<false>(__func__, n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, K, x, x_row,
                                   x_col, y, y_row, y_col, tiny, d_err, stream);
}
