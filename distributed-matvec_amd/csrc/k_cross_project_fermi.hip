// k_cross_project_fermi.hip -- the projecting cross-sector kernel with a projected FERMIONIC basis on either side (spinless; spinful
// over their 2 L modes): the k_cross_project template of k_cross_project_t.hpp with its FERMI switch on.  The target's elements carry
// sign(g, r') of lsk_fermi.hpp where the target has a sign table, and stage B1 projects every packet into the source basis with the
// signed characters where the source is projected.  The same 8 kinds as k_cross_project.hip, in a translation unit of their own as
// k_cross_fermi.hip is.  DESIGN.md section 6b.
#include "k_cross_project_t.hpp"

// the name of the family in plans and reports: k_cross_project<W, PM1, CPLX, REAL, TPM1, FERMI = true>
extern "C" char const *lsk_cross_project_fermi_kernel_name(void) { return "k_cross_project_fermi"; }

// lsk_cross_project for src.fermi || dst.fermi (same arguments; reached through it).  A projected fermionic source is looked up in
// its static index table: the sign table and the table's key width bound every shift and load of stage B1.
extern "C" int lsk_cross_project_fermi(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src,
                                       lsk_index six, lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps,
                                       double const *dst_norms, void const *x, void *y, double tiny, unsigned long long *d_count,
                                       int *d_err, void *stream) {
    if (!src.fermi && !dst.fermi) { snprintf(g_err, sizeof(g_err), "%s: neither basis is a projected fermionic one", __func__); return -1; }
    if (src.fermi && (!src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL)) {
        snprintf(g_err, sizeof(g_err), "%s: the source is not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (dst.fermi && (!dst.fsign || dst.spin_inversion != 0)) {
        snprintf(g_err, sizeof(g_err), "%s: the target is not a projected fermionic basis with a sign table", __func__);
        return -1;
    }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (src.fermi && (!gt.entries || gt.L != src.number_sites)) {
        snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__);
        return -1;
    }
    if (!cxp_args_ok(__func__, is_real, src, gt, dst, cplx)) return -1;
    const bool real_coef = is_real && src.chars_pm1 && dst.chars_pm1;
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
    if (src.number_sites <= 32) LSK_CXP_LAUNCH(uint32_t, true); else LSK_CXP_LAUNCH(uint64_t, true);
    LSK_LAUNCH_CHECK();
    return 0;
}
