// k_amplitude_fermi.hip -- amplitudes of sector states on product states and orbit images (ls_amd_amp, host.c)
// for projected fermionic bases: stage B1 with the signed characters chi(g) sign(g, s) of lsk_fermi.hpp, so the character of a state
// carries its orbit sign (include/ls_hs.h), and the lifted ring elements of a spinful basis (fermi_apply_elem_w), the up <-> down
// flip among them.  The body is k_amplitude_t.hpp with FERMI = true.
#include "k_amplitude_t.hpp"

extern "C" char const *lsk_amplitude_fermi_kernel_name(void) { return "k_amplitude_pull_fermi"; }

extern "C" int lsk_amplitude_pull_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int cplx, int64_t B,
                                        uint64_t const *states, void const *psi, void *out, int *d_err, void *stream) {
    return amp_pull_launch<true>(__func__, bs, six, gt, pj, cplx, B, states, psi, out, d_err, stream);
}
extern "C" int lsk_amplitude_info_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int64_t B, uint64_t const *states,
                                        uint64_t *reps_out, int64_t *index, double *characters, double *norms, int *d_err, void *stream) {
    return amp_info_launch<true>(__func__, bs, six, gt, pj, B, states, reps_out, index, characters, norms, d_err, stream);
}
extern "C" int lsk_orbit_image_fermi(lsk_basis bs, int64_t n, uint64_t const *reps, int64_t B, int64_t const *rows, int32_t const *elements,
                                     uint64_t *out, int *d_err, void *stream) {
    return orbit_image_launch<true>(__func__, bs, n, reps, B, rows, elements, out, d_err, stream);
}
