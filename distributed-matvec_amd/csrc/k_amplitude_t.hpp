// k_amplitude_t.hpp -- amplitudes of sector states on a batch of product states, and the orbit images that Born sampling draws
// (ls_amd_amp, host.c).  With state_info(s) = (rep, character, n) of a word s of the basis WITHOUT symmetries,
//     <s|psi> = conj(character(s)) n(rep) psi[index(rep)]                          (the formula of k_expand_push, read the other way)
// on a projected basis -- the character carries the orbit sign sign(g0, s) on a projected fermionic one -- and psi[index(s)] on an
// unprojected one.  k_amplitude_pull: one QUERIED state per lane, in any order, duplicates allowed:
//   1. membership (pj_is_state, k_project_t.hpp): a word with a bit above the sites, another weight / particle number or another
//      (N_up, N_down) split is no state of the basis -- every column reads 0, no error (the rule of ExpectationPlan for images that
//      leave the conserved numbers);
//   2. stage B1 (sector_project, k_cross_t.hpp) on a projected basis: representative, character, n(rep); a zero-norm orbit reads 0;
//   3. the look-up of the seven sector kernels: the static index table of the array (the key-width guard gt.L < 64, the out-of-range
//      rule), or cross_index on an unprojected basis; a representative that is missing from the array raises *err and reads 0;
//   4. the K columns in chunks of 8 INSIDE the kernel: steps 1-3 run once per state whatever K; a chunk's 8 loads are issued before
//      any is used (an interleaved c128 chunk is one 128-byte gather); one plain store per (state, column), no atomics: two calls
//      return the same bytes.
// The info mode is the same body without psi: rep, index (-1 outside the basis or on a zero-norm orbit), character (re, im) and n per
// state -- the device-pointer form of ls_hs_state_info + ls_hs_state_index.
// k_orbit_image: one (row, element) pair per lane, out = g_e reps[row] over the EFFECTIVE group: on a spin basis with the global
// inversion element 2 p is permutation p and 2 p + 1 is permutation p followed by ^ site_mask; every other basis has its element list
// (the up <-> down flip of a spinful basis is a group element).  The descriptor is loaded per lane: elements differ from lane to lane.
// No LDS, no cross-lane traffic.  As k_cross_t.hpp this header holds the kernels and their launchers as templates on FERMI:
// k_amplitude.hip instantiates FERMI = false (spin bases and unprojected fermionic ones), k_amplitude_fermi.hip FERMI = true (projected
// fermionic bases: the signed characters of lsk_fermi.hpp; the plans call that family "k_amplitude_pull_fermi").
#pragma once
#include "k_cross_t.hpp"
#include "k_project_t.hpp"

constexpr int kAmpCols = LSK_AMP_COLS; // columns per chunk

// steps 1-3 for one word: false when the state reads 0 (rep, chr, chi, nb are then what the info mode reports)
template <typename W, bool PM1, int KIND, bool FERMI>
__device__ __forceinline__ bool amp_resolve(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, lsk_index const &six,
                                            lsk_gtab const &gt, lsk_project const &pj, uint64_t s64, uint64_t &rep64, double &chr,
                                            double &chi, double &nb, int64_t &idx, int *err) {
    const W mask = (W)bs.site_mask;
    rep64 = s64; chr = 0.0; chi = 0.0; nb = 0.0; idx = -1;
    if ((s64 & ~bs.site_mask) != 0 || !pj_is_state<W, KIND>((W)s64, mask, bs.hamming_weight, pj)) return false;
    chr = 1.0; nb = 1.0;
    if (bs.proj != LSK_PROJ_NONE) {
        W rep;
        const bool alive = sector_project<W, PM1, FERMI>(bs, elems, (W)s64, rep, chr, chi, nb, FERMI && bs.fermi != 0);
        rep64 = (uint64_t)rep;
        if (!alive) { nb = 0.0; return false; }
    }
    if (gt.entries != nullptr) {
        if (!(gt.L < 64 && (rep64 >> gt.L) != 0)) {
            uint64_t bucket; uint32_t tag;
            gt_split(gt, rep64, bucket, tag);
            const uint32_t pay = gt_resolve(gt, gt.entries, bucket, tag, *(ulonglong2 const *)(gt.entries + 2 * bucket));
            idx = pay == 0xffffffffu ? -1 : (int64_t)pay;
        }
    } else idx = cross_index(six, rep64);
    if (idx < 0 || idx >= six.count) { idx = -1; atomicExch(err, 1); return false; } // inside the conserved numbers, missing from reps
    return true;
}

template <typename W, bool PM1, bool CPLX, int KIND, bool FERMI>
__device__ __forceinline__ void amp_states(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, lsk_index const &six,
                                           lsk_gtab const &gt, lsk_project const &pj, int64_t B, uint64_t const *__restrict__ states,
                                           double const *__restrict__ psi, double *__restrict__ out, int *err) {
    const bool project = bs.proj != LSK_PROJ_NONE;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < B; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + threadIdx.x;
        if (i >= B) continue; // (no barrier below)
        uint64_t rep; double chr, chi, nb; int64_t idx;
        const bool live = amp_resolve<W, PM1, KIND, FERMI>(bs, elems, six, gt, pj, states[i], rep, chr, chi, nb, idx, err);
        const double ar = chr * nb, ai = PM1 ? 0.0 : -chi * nb; // conj(character) n(rep)
        for (int c0 = 0; c0 < pj.K; c0 += kAmpCols) {
            const int kc = pj.K - c0 < kAmpCols ? pj.K - c0 : kAmpCols;
            double vr[kAmpCols], vi[kAmpCols];
#pragma unroll
            for (int c = 0; c < kAmpCols; ++c) {
                vr[c] = 0.0; vi[c] = 0.0;
                if (live && c < kc) {
                    const int64_t at = idx * pj.phi_s0 + (int64_t)(c0 + c) * pj.phi_s1;
                    if (CPLX) { const double2 v = reinterpret_cast<double2 const *>(psi)[at]; vr[c] = v.x; vi[c] = v.y; }
                    else vr[c] = psi[at];
                }
            }
#pragma unroll
            for (int c = 0; c < kAmpCols; ++c) {
                if (c >= kc) break;
                const int64_t at = i * pj.out_s0 + (int64_t)(c0 + c) * pj.out_s1;
                double yr = vr[c], yi = vi[c];
                if (live && project) {
                    if (PM1) { yr = ar * vr[c]; yi = ar * vi[c]; }
                    else { yr = ar * vr[c] - ai * vi[c]; yi = ar * vi[c] + ai * vr[c]; }
                }
                if (CPLX) reinterpret_cast<double2 *>(out)[at] = make_double2(yr, yi);
                else out[at] = yr;
            }
        }
    }
}

// the info mode: any output may be NULL
template <typename W, bool PM1, int KIND, bool FERMI>
__device__ __forceinline__ void amp_info(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, lsk_index const &six,
                                         lsk_gtab const &gt, lsk_project const &pj, int64_t B, uint64_t const *__restrict__ states,
                                         uint64_t *__restrict__ o_rep, int64_t *__restrict__ o_idx, double *__restrict__ o_ch,
                                         double *__restrict__ o_nrm, int *err) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
        uint64_t rep; double chr, chi, nb; int64_t idx;
        amp_resolve<W, PM1, KIND, FERMI>(bs, elems, six, gt, pj, states[i], rep, chr, chi, nb, idx, err);
        if (o_rep) o_rep[i] = rep;
        if (o_idx) o_idx[i] = idx;
        if (o_ch) { o_ch[2 * i] = chr; o_ch[2 * i + 1] = PM1 ? 0.0 : chi; }
        if (o_nrm) o_nrm[i] = nb;
    }
}

template <typename W, bool FERMI>
__device__ __forceinline__ void orbit_images(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, int64_t n,
                                             uint64_t const *__restrict__ reps, int64_t B, int64_t const *__restrict__ rows,
                                             int32_t const *__restrict__ elements, uint64_t *__restrict__ out, int *err) {
    const int L = bs.number_sites, inv = FERMI ? 0 : bs.spin_inversion;
    const int n_eff = inv != 0 ? 2 * bs.n_elems : bs.n_elems;
    const W mask = (W)bs.site_mask;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < B; i += (int64_t)gridDim.x * kBlock) {
        const int64_t row = rows[i];
        const int el = elements[i];
        if (row < 0 || row >= n || el < 0 || el >= n_eff) { atomicExch(err + 1, 1); out[i] = 0; continue; }
        lsk_group_elem const &e = elems[inv != 0 ? el >> 1 : el]; // per lane: the elements differ from lane to lane
        const W r = (W)reps[row];
        W t = FERMI ? fermi_apply_elem_w<W>(e, r, L, mask) : apply_elem_w<W>(e, r, L, mask);
        if (inv != 0 && (el & 1)) t = (W)(t ^ mask);
        out[i] = (uint64_t)t;
    }
}

// the grid of every launch here: what is co-resident; LS_AMD_AMP_BLOCKS=<k>, read at every launch, lowers the ceiling (a test hook:
// several trips of the grid-stride loop at sizes a dense reference reaches)
template <typename Kern>
static int amp_grid(Kern kernel, int64_t B) {
    const int64_t work_blocks = (B + kBlock - 1) / kBlock;
    int64_t g = resident_grid(kernel, work_blocks);
    if (char const *e = getenv("LS_AMD_AMP_BLOCKS")) { const long k = atol(e); if (k >= 1 && k < g) g = k; }
    return (int)(g < 1 ? 1 : g);
}

static inline int amp_args_ok(char const *who, lsk_basis const &bs, lsk_gtab const &gt, lsk_project const &pj, bool fermi_unit) {
    if (bs.number_sites < 1 || bs.number_sites > 64) { snprintf(g_err, sizeof(g_err), "%s: the basis has %d sites", who, bs.number_sites); return 0; }
    if (bs.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected basis is looked up by its index", who); return 0; }
    if (pj.kind != PJ_ALL && pj.kind != PJ_FIXED && pj.kind != PJ_PRODUCT) { snprintf(g_err, sizeof(g_err), "%s: unknown membership kind %d", who, pj.kind); return 0; }
    if (pj.kind == PJ_PRODUCT && (bs.number_sites != 2 * pj.half || pj.half < 1 || pj.half > 32 || bs.spin_inversion != 0)) {
        snprintf(g_err, sizeof(g_err), "%s: the (N_up, N_down) split does not belong to the basis", who);
        return 0;
    }
    if (fermi_unit ? (bs.spin_inversion != 0 || !bs.fermi || !bs.fsign) : bs.fermi != 0) {
        snprintf(g_err, sizeof(g_err), "%s: %s", who, fermi_unit ? "not a projected fermionic basis (no sign table, or a spin inversion)"
                                                                  : "projected fermionic bases carry orbit signs (the _fermi unit)");
        return 0;
    }
    return 1;
}

template <typename W, bool PM1, bool CPLX, int KIND, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_amplitude_pull(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                           lsk_project pj, int64_t B, uint64_t const *__restrict__ states,
                                                           double const *__restrict__ psi, double *__restrict__ out, int *err) {
    amp_states<W, PM1, CPLX, KIND, FERMI>(bs, elems, six, gt, pj, B, states, psi, out, err);
}
template <typename W, bool PM1, int KIND, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_amplitude_info(lsk_basis bs, lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                           lsk_project pj, int64_t B, uint64_t const *__restrict__ states,
                                                           uint64_t *__restrict__ o_rep, int64_t *__restrict__ o_idx,
                                                           double *__restrict__ o_ch, double *__restrict__ o_nrm, int *err) {
    amp_info<W, PM1, KIND, FERMI>(bs, elems, six, gt, pj, B, states, o_rep, o_idx, o_ch, o_nrm, err);
}
template <typename W, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_orbit_image(lsk_basis bs, lsk_group_elem const *__restrict__ elems, int64_t n,
                                                        uint64_t const *__restrict__ reps, int64_t B, int64_t const *__restrict__ rows,
                                                        int32_t const *__restrict__ elements, uint64_t *__restrict__ out, int *err) {
    orbit_images<W, FERMI>(bs, elems, n, reps, B, rows, elements, out, err);
}

// the launches of both units (who: the entry point, for its messages): {32, 64-bit words} x {f64 | c128 x {+-1, complex characters}} x
// {all states, fixed number, product}: 18 amplitude kernels per unit; the info mode has no dtype: 12
#define LSK_AMP_KINDS(ONE, W, ...)                                                                                                       \
    do {                                                                                                                                 \
        if (pj.kind == PJ_FIXED) ONE(W, __VA_ARGS__, PJ_FIXED);                                                                          \
        else if (pj.kind == PJ_PRODUCT) ONE(W, __VA_ARGS__, PJ_PRODUCT);                                                                 \
        else ONE(W, __VA_ARGS__, PJ_ALL);                                                                                                \
    } while (0)
template <bool FERMI>
static int amp_pull_launch(char const *who, lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int cplx, int64_t B,
                           uint64_t const *states, void const *psi, void *out, int *d_err, void *stream) {
    if (pj.K < 1 || pj.K > LSK_PROJECT_MAX_K) { snprintf(g_err, sizeof(g_err), "%s: K = %d columns, outside [1, %d]", who, pj.K, LSK_PROJECT_MAX_K); return -1; }
    if (!cplx && !bs.chars_pm1) { snprintf(g_err, sizeof(g_err), "%s: f64 needs +-1 characters", who); return -1; }
    if (B <= 0) return 0;
    if (!amp_args_ok(who, bs, gt, pj, FERMI)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 b(kBlock);
#define LSK_AMP_ONE(W, PM1, CPLX, KIND)                                                                                                  \
    hipLaunchKernelGGL((k_amplitude_pull<W, PM1, CPLX, KIND, FERMI>), dim3(amp_grid(k_amplitude_pull<W, PM1, CPLX, KIND, FERMI>, B)), b, \
                       0, s, bs, bs.elems, six, gt, pj, B, states, (double const *)psi, (double *)out, d_err)
#define LSK_AMP_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (!cplx) LSK_AMP_KINDS(LSK_AMP_ONE, W, true, false);                                                                           \
        else if (bs.chars_pm1) LSK_AMP_KINDS(LSK_AMP_ONE, W, true, true);                                                                \
        else LSK_AMP_KINDS(LSK_AMP_ONE, W, false, true);                                                                                 \
    } while (0)
    if (bs.number_sites <= 32) LSK_AMP_LAUNCH(uint32_t); else LSK_AMP_LAUNCH(uint64_t);
#undef LSK_AMP_LAUNCH
#undef LSK_AMP_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}
template <bool FERMI>
static int amp_info_launch(char const *who, lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int64_t B, uint64_t const *states,
                           uint64_t *o_rep, int64_t *o_idx, double *o_ch, double *o_nrm, int *d_err, void *stream) {
    if (B <= 0) return 0;
    if (!amp_args_ok(who, bs, gt, pj, FERMI)) return -1;
    hipStream_t s = (hipStream_t)stream;
    const dim3 b(kBlock);
#define LSK_AMP_ONE(W, PM1, KIND)                                                                                                        \
    hipLaunchKernelGGL((k_amplitude_info<W, PM1, KIND, FERMI>), dim3(amp_grid(k_amplitude_info<W, PM1, KIND, FERMI>, B)), b, 0, s, bs,   \
                       bs.elems, six, gt, pj, B, states, o_rep, o_idx, o_ch, o_nrm, d_err)
#define LSK_AMP_LAUNCH(W)                                                                                                                \
    do {                                                                                                                                 \
        if (bs.chars_pm1) LSK_AMP_KINDS(LSK_AMP_ONE, W, true);                                                                           \
        else LSK_AMP_KINDS(LSK_AMP_ONE, W, false);                                                                                       \
    } while (0)
    if (bs.number_sites <= 32) LSK_AMP_LAUNCH(uint32_t); else LSK_AMP_LAUNCH(uint64_t);
#undef LSK_AMP_LAUNCH
#undef LSK_AMP_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}
template <bool FERMI>
static int orbit_image_launch(char const *who, lsk_basis bs, int64_t n, uint64_t const *reps, int64_t B, int64_t const *rows,
                              int32_t const *elements, uint64_t *out, int *d_err, void *stream) {
    if (B <= 0) return 0;
    if (bs.number_sites < 1 || bs.number_sites > 64 || bs.n_elems < 1 || !bs.elems) { snprintf(g_err, sizeof(g_err), "%s: the basis has no element list", who); return -1; }
    hipStream_t s = (hipStream_t)stream;
    const dim3 b(kBlock);
    if (bs.number_sites <= 32)
        hipLaunchKernelGGL((k_orbit_image<uint32_t, FERMI>), dim3(amp_grid(k_orbit_image<uint32_t, FERMI>, B)), b, 0, s, bs, bs.elems, n, reps, B, rows, elements, out, d_err);
    else
        hipLaunchKernelGGL((k_orbit_image<uint64_t, FERMI>), dim3(amp_grid(k_orbit_image<uint64_t, FERMI>, B)), b, 0, s, bs, bs.elems, n, reps, B, rows, elements, out, d_err);
    LSK_LAUNCH_CHECK();
    return 0;
}
