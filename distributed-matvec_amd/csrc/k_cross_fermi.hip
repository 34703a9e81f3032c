// k_cross_fermi.hip -- cross-sector operators between projected FERMIONIC bases (spinless; spinful over their 2 L modes): the
// k_cross_pull template of k_cross_t.hpp with its FERMI switch on, so that stage B1 projects every packet into the source basis with the
// signed characters chi(g) sign(g, a) of lsk_fermi.hpp.  c+_k, c_k, n_q, S^z_q between the (momentum, point-group, flip) sectors of
// a t-V or Hubbard model: the Jordan-Wigner signs of the operator are in the terms' sign masks, the permutation signs of the
// projection are here.  The same 10 kinds as k_cross.hip; a translation unit of its own so that k_cross.hip and k_fermi.hip keep
// their kernel counts (tests pin both).  DESIGN.md section 6b.
#include "k_cross_t.hpp"

// the name of the family in plans and reports: k_cross_pull<W, PM1, CPLX, REAL, FERMI = true>
extern "C" char const *lsk_cross_fermi_kernel_name(void) { return "k_cross_pull_fermi"; }

// lsk_cross_pull for src.fermi (same arguments; reached through it).  The source is always projected, so always looked up in its
// static index table: the sign table and the table's key width bound every shift and load of the kernel.
extern "C" int lsk_cross_fermi_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                    lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x,
                                    void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (!src.fermi || !src.fsign || src.spin_inversion != 0 || src.k4_mode != 0 || src.proj != LSK_PROJ_FULL) {
        snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!gt.entries || gt.L != src.number_sites) { snprintf(g_err, sizeof(g_err), "%s: a projected fermionic source is looked up in its static index table", __func__); return -1; }
    return cross_pull_launch<true>(__func__, n_groups, groups, terms, is_real, src, six, gt, cplx, n_dst, dst_reps, dst_norms, x, y, tiny, d_count, d_err, stream);
}
