// k_cross_project.hip -- cross-sector operators between bases with DIFFERENT symmetry groups, any operator (ls_amd_cross_create_groups
// with LS_AMD_CROSS_PROJECT, host.c): y = B2+ A B1 x, the sum over the target group's elements outside the
// stages of k_cross_pull.  The kernel is the template of k_cross_project_t.hpp; this unit holds its 8 instantiations without
// permutation signs (spin bases, unprojected fermionic bases), and lsk_cross_project hands a pair with a projected fermionic basis
// on either side to the signed ones of k_cross_project_fermi.hip.
#include "k_cross_project_t.hpp"

extern "C" char const *lsk_cross_project_kernel_name(void) { return "k_cross_project"; }

// d_count != NULL: nothing is read from x or written to y; the packets that reach a source row are added to *d_count
extern "C" int lsk_cross_project(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                 lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                                 void const *x, void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (src.fermi || dst.fermi)
        return lsk_cross_project_fermi(n_groups, groups, terms, is_real, src, six, gt, dst, cplx, n_dst, dst_reps, dst_norms, x, y, tiny, d_count, d_err, stream);
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cxp_args_ok(__func__, is_real, src, gt, dst, cplx)) return -1;
    const bool real_coef = is_real && src.chars_pm1 && dst.chars_pm1;
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
    if (src.number_sites <= 32) LSK_CXP_LAUNCH(uint32_t, false); else LSK_CXP_LAUNCH(uint64_t, false);
    LSK_LAUNCH_CHECK();
    return 0;
}
