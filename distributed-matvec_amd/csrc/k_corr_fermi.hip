// k_corr_fermi.hip -- the hopping kernel of the correlation matrices on projected FERMIONIC bases (spinless; spinful over their 2 L
// modes): the k_corr_hop template of k_corr_t.hpp with its FERMI switch on, so that stage B1 projects every image with the signed
// characters chi(g) sign(g, a) of lsk_fermi.hpp.  The Jordan-Wigner sign of c+_i c_j is the kernel's `jw` argument, which an
// unprojected fermionic basis sets as well (k_corr.hip).  The same 6 kinds as k_corr.hip; a translation unit of its own, as
// k_cross_fermi.hip is.  DESIGN.md section 6e.
#include "k_corr_t.hpp"

// the name of the family in plans and reports: k_corr_hop<W, PM1, CPLX, FERMI = true>
extern "C" char const *lsk_corr_hop_fermi_kernel_name(void) { return "k_corr_hop_fermi"; }

// lsk_corr_hop for bs.fermi (same arguments; reached through it).  The basis is always projected, so always looked up in its static
// index table: the sign table and the table's key width bound every shift and load of the kernel.
extern "C" int lsk_corr_hop_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, int jw, int n_pairs, uint16_t const *pairs, int cplx, int64_t n,
                                  uint64_t const *reps, double const *norms, void const *psi, double *partial, double *out, int *d_err,
                                  void *stream) {
    if (!bs.fermi || !bs.fsign || bs.spin_inversion != 0 || bs.k4_mode != 0 || bs.proj != LSK_PROJ_FULL) {
        snprintf(g_err, sizeof(g_err), "%s: not a projected fermionic basis in K4 mode 0", __func__);
        return -1;
    }
    if (n <= 0 || n_pairs <= 0) return 0;
    if (!gt.entries || gt.L != bs.number_sites) { snprintf(g_err, sizeof(g_err), "%s: a projected fermionic basis is looked up in its static index table", __func__); return -1; }
    return corr_hop_launch<true>(bs, six, gt, jw, n_pairs, pairs, cplx, n, reps, norms, psi, partial, out, d_err, stream);
}
