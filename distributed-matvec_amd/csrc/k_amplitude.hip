// k_amplitude.hip -- amplitudes of sector states on product states and orbit images (ls_amd_amp, host.c) for
// the bases without permutation signs: spin-1/2 bases, with the global inversion, and unprojected fermionic bases.  The kernels
// k_amplitude_pull, k_amplitude_info and k_orbit_image, their lane mapping and their bounds are in k_amplitude_t.hpp; the projected
// fermionic bases (signed characters) are k_amplitude_fermi.hip.
#include "k_amplitude_t.hpp"

extern "C" char const *lsk_amplitude_kernel_name(void) { return "k_amplitude_pull"; }

extern "C" int lsk_amplitude_pull(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int cplx, int64_t B, uint64_t const *states,
                                  void const *psi, void *out, int *d_err, void *stream) {
    return amp_pull_launch<false>(__func__, bs, six, gt, pj, cplx, B, states, psi, out, d_err, stream);
}
extern "C" int lsk_amplitude_info(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int64_t B, uint64_t const *states,
                                  uint64_t *reps_out, int64_t *index, double *characters, double *norms, int *d_err, void *stream) {
    return amp_info_launch<false>(__func__, bs, six, gt, pj, B, states, reps_out, index, characters, norms, d_err, stream);
}
extern "C" int lsk_orbit_image(lsk_basis bs, int64_t n, uint64_t const *reps, int64_t B, int64_t const *rows, int32_t const *elements,
                               uint64_t *out, int *d_err, void *stream) {
    return orbit_image_launch<false>(__func__, bs, n, reps, B, rows, elements, out, d_err, stream);
}
