// k_cross_project_blk.hip -- the projecting cross-sector operator on blocks of vectors: Y[:, k] = B2+ A B1 X[:, k] for the K columns of an
// (n_src, K) block with element strides (row, column), ls_amd_cross_apply_block on a LS_AMD_CROSS_PROJECT plan with the kernel path
// (host.c).  The kernel is the template of k_cross_project_blk_t.hpp -- the stages of k_cross_project once per chunk of 8 columns, the
// row's sums in registers (DESIGN.md sections 6b, 6h); this unit holds its 8 instantiations without permutation signs (spin bases,
// unprojected fermionic bases), and lsk_cross_project_blk hands a pair with a projected fermionic basis on either side to the signed
// ones of k_cross_project_blk_fermi.hip.
#include "k_cross_project_blk_t.hpp"

extern "C" char const *lsk_cross_project_blk_kernel_name(void) { return "k_cross_project_blk"; }

extern "C" int lsk_cross_project_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                     lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                                     int K, void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny,
                                     int *d_err, void *stream) {
    if (src.fermi || dst.fermi)
        return lsk_cross_project_blk_fermi(n_groups, groups, terms, is_real, src, six, gt, dst, cplx, n_dst, dst_reps, dst_norms, K, x, x_row,
                                           x_col, y, y_row, y_col, tiny, d_err, stream);
    return cross_project_blk_launch<false>(__func__, n_groups, groups, terms, is_real, src, six, gt, dst, cplx, n_dst, dst_reps, dst_norms, K,
                                           x, x_row, x_col, y, y_row, y_col, tiny, d_err, stream);
}
