// k_cross_t.hpp -- the cross-sector pull kernel k_cross_pull as a template header: k_cross.hip instantiates
// it for the bases without permutation signs (FERMI = false), k_cross_fermi.hip for the projected fermionic ones (FERMI = true; the
// plans call that family "k_cross_pull_fermi").  Moved out of k_cross.hip unchanged (the machine code of the 10 spin kinds is the
// same, instruction for instruction); it gained two compile-time switches: the emitting mode of the CSR export (on the word type,
// see cross_emit_w below; instantiated in k_csr.hip), and FERMI, which makes stage B1 project a packet with the signed characters
// chi(g) sign(g, a) of lsk_fermi.hpp (fermi_state_info_w) instead of state_info_w.  Nothing else in the formula changes: chr, chi
// and stab then carry sign(g0, beta) and the signed stabiliser sum, and the zero-norm test drops the orbits whose signed sum
// vanishes (which happens in ANY fermionic sector).  The branch is discarded at compile time by the spin instantiations.
// The header is the root of the include chain of all seven sector kernels, so it also holds what they share as functions
// (cross_wave_slot, sector_project, below cross_index) and, at the end, the launcher of both k_cross_pull units.
#pragma once
#include "lsk_dev.hpp"
#include "lsk_fermi.hpp"

constexpr int kGCCross = 4;                    // flip-mask groups per pass
constexpr int kCapCross = kBlock * kGCCross;   // packets a pass of one tile can generate

// index of state s in an UNPROJECTED source basis, or -1 (the closed forms check membership themselves: the adjoint may leave the
// source's weight sector, which is an error the caller reads back, never an out-of-range load)
__device__ __forceinline__ int64_t cross_index(lsk_index const &ix, uint64_t s) {
    if (ix.kind == LSK_INDEX_IDENTITY) return s < (uint64_t)ix.count ? (int64_t)s : -1;
    if (ix.kind == LSK_INDEX_COMBINADIC) {
        if (__popcll(s) != ix.dir_weight || (ix.dir_sites < 64 && (s >> ix.dir_sites) != 0)) return -1;
        const int64_t r = rank_combinadic(s, ix.binom);
        return r < ix.count ? r : -1;
    }
    if (ix.kind == LSK_INDEX_PRODUCT) {
        const int64_t r = product_index(ix, s, ix.binom);
        return r < ix.count ? r : -1;
    }
    if (ix.count <= 0 || (ix.dir_sites < 64 && (s >> ix.dir_sites) != 0)) return -1; // (SEARCH: the prefix table covers dir_sites bits)
    return search_index(ix, s);
}

// ---- what the seven sector kernels share as functions (k_cross_pull, k_cross_pull_blk, k_cross_project here; k_corr_hop, k_expect,
// k_expect_blk, k_expect_mat through k_corr_t.hpp): the slot allocation of the cross kernels and the core of stage B1 with its
// zero-norm threshold.  With these two every 32-bit instantiation keeps its machine code, instruction for instruction, and every
// 64-bit one its register counts, LDS and occupancy (profiles/sector_stages_resources.txt).  The look-up of stage B2, the ordered compaction
// of k_corr_hop / k_expect* and the emit predicate of k_expect* stay as text in each kernel: as shared functions (the look-up in three
// forms) each of them cost some instantiation 1 - 5 % -- these kernels sit at 106 SGPRs with spills to VGPR lanes, and any change of
// their text moves the allocation (profiles/sector_stages_ab.txt).  Keep the copies equal by hand: the key-width guard gt.L < 64 and
// the out-of-range rule of the look-up are the same in all seven.

// Stage A of the cross kernels: the next slot of the block's packet list for every active lane -- a ballot, one LDS atomicAdd per
// wave, so the slots follow the order in which the waves arrive.  (The value is meaningless for a lane that is not active.)
__device__ __forceinline__ int cross_wave_slot(bool act, int lane, int *s_n) {
    const unsigned long long ball = __ballot(act);
    int base = 0;
    if (lane == 0 && ball) base = atomicAdd(s_n, __popcll(ball));
    base = __shfl(base, 0);
    return base + __popcll(ball & ((1ULL << lane) - 1));
}

// Stage B1, the core: project the image s into the basis (general K4: minimum, character, stabiliser norm) -- its representative,
// the character (chr, chi) of the element g0 that maps s there, and nb = n(rep).  false: zero norm in the sector, the packet
// contributes nothing (with FERMI that happens in ANY sector: the signed stabiliser sum vanishes).  What a kernel multiplies into its
// slot is its own: the roundings differ from kernel to kernel and are part of their results.  FERMI projects with the signed
// characters chi(g) sign(g, s) of lsk_fermi.hpp; `signs` is the run-time half of that switch, which k_cross_project alone needs (its
// FERMI says that EITHER basis is fermionic).
template <typename W, bool PM1, bool FERMI>
__device__ __forceinline__ bool sector_project(lsk_basis const &bs, lsk_group_elem const *__restrict__ elems, W s, W &rep, double &chr,
                                               double &chi, double &nb, bool signs = true) {
    double stab;
    if (FERMI && signs) fermi_state_info_w<W, PM1>(bs, elems, s, rep, chr, chi, stab);
    else state_info_w<W, PM1>(bs, elems, s, rep, chr, chi, stab);
    const double n2 = stab * bs.inv_order;
    if (!(n2 > 1e-12)) return false;
    nb = sqrt(n2);
    return true;
}

// The compile-time mode of the kernel rides on its word type, so that the apply kernels keep their five template arguments, their
// names and their machine code: W = uint32_t / uint64_t multiplies every packet that reached a source row by x and adds it to its
// row of y (or counts the packets, count != NULL); W = cross_emit_w<uint32_t / uint64_t> hands (row, source index, coefficient) out
// instead -- the CSR export of k_csr.hip.  Stages A, B1, B2 are the same text for both.  The emitting mode
// reads its arguments from the same parameter list:
//     x      int64_t const [n_dst + 1]: first raw slot of every target row, then the number of slots; nullptr: the counting pass
//     count  counting pass: int64_t [n_dst], the packets of every target row;  fill: int64_t [slots], the source index of every packet
//     y      fill: the coefficient of every packet, 1 (f64) or 2 (c128) doubles
template <typename T> struct cross_emit_w { using word = T; };
template <typename T> struct cross_word { using word = T; static constexpr bool emit = false; };
template <typename T> struct cross_word<cross_emit_w<T>> { using word = T; static constexpr bool emit = true; };

template <typename WM, bool PM1, bool CPLX, bool REAL, bool FERMI>
__global__ __launch_bounds__(kBlock) void k_cross_pull(int n_groups, lsk_group const *__restrict__ groups,
                                                       lsk_term const *__restrict__ terms, lsk_basis sbs,
                                                       lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                       int64_t n_dst, uint64_t const *__restrict__ dst_reps,
                                                       double const *__restrict__ dst_norms, double const *__restrict__ x,
                                                       double *__restrict__ y, double tiny, unsigned long long *count, int *err) {
    using W = typename cross_word<WM>::word;
    constexpr bool EMIT = cross_word<WM>::emit;
    constexpr bool RC = REAL && PM1; // the coefficient stays real: real terms and +-1 source characters
    // EMIT: a row's packets are numbered in ascending group order whatever slot of the list they took -- the group of every
    // packet (s_g, relative to the pass), the groups of the pass that reached a source row (s_mask, one word per row) and the row's
    // next raw slot (s_base) give packet (row, g) the slot s_base[row] + popcount(s_mask[row] below g): no order of arrival enters
    __shared__ uint8_t s_g[EMIT ? kCapCross : 1];
    __shared__ uint32_t s_mask[EMIT ? kBlock : 1];
    __shared__ int64_t s_base[EMIT ? kBlock : 1];
    int64_t const *const e_off = (int64_t const *)x;
    int64_t *const e_out = (int64_t *)count;
    __shared__ uint64_t s_beta[kCapCross];
    __shared__ double s_coef[kCapCross * (RC ? 1 : 2)];
    __shared__ uint16_t s_row[kCapCross];
    __shared__ double s_acc[kBlock * (CPLX ? 2 : 1)];
    __shared__ int s_n;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool project = sbs.proj != LSK_PROJ_NONE;
    const bool table = gt.entries != nullptr;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock; t0 < n_dst; t0 += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t0 + tid;
        const bool valid = i < n_dst;
        uint64_t a = 0;
        double inv_na = 0.0;
        if (valid) {
            a = dst_reps[i];
            const double na = dst_norms[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
        }
        if constexpr (!EMIT) { if (CPLX) { s_acc[2 * tid] = 0.0; s_acc[2 * tid + 1] = 0.0; } else s_acc[tid] = 0.0; }
        unsigned long long found = 0;
        for (int g0 = 0; g0 < n_groups; g0 += kGCCross) {
            if (tid == 0) s_n = 0;
            if constexpr (EMIT) { // (the fills of the pass before are behind its closing barrier)
                s_base[tid] = g0 == 0 ? (valid && e_off ? e_off[i] : 0) : s_base[tid] + __popc(s_mask[tid]);
                s_mask[tid] = 0;
            }
            __syncthreads();
            // ---- stage A: the adjoint's groups of every row -> packets (state, conj(c) / n2(r'), row) ------------------
            const int g1 = min(g0 + kGCCross, n_groups);
            for (int g = g0; g < g1; ++g) {
                lsk_group const G = groups[g];
                double cr = 0.0, ci = 0.0;
                if (valid) term_sum<REAL>(terms, G.begin, G.end, a, cr, ci);
                // (tiny: the rounding residue of terms that cancel -- sum_j e^{-iqj} sigma^z_j on a state of shorter period -- is no packet)
                const bool act = valid && (fabs(cr) > tiny || (!REAL && fabs(ci) > tiny));
                const int slot = cross_wave_slot(act, lane, &s_n);
                if (act) {
                    s_beta[slot] = a ^ G.x;
                    s_row[slot] = (uint16_t)tid;
                    if constexpr (EMIT) s_g[slot] = (uint8_t)(g - g0);
                    if (RC) s_coef[slot] = cr * inv_na;
                    else { s_coef[2 * slot] = cr * inv_na; s_coef[2 * slot + 1] = -ci * inv_na; }
                }
            }
            __syncthreads();
            const int n = s_n;
            // ---- stage B1: project every packet into the SOURCE basis (general K4: minimum, character, stabiliser norm) --
            if (project) {
                for (int e = tid; e < n; e += kBlock) {
                    W rep; double chr, chi, nb;
                    if (!sector_project<W, PM1, FERMI>(sbs, elems, (W)s_beta[e], rep, chr, chi, nb)) { s_row[e] = 0xffff; continue; }
                    s_beta[e] = (uint64_t)rep;
                    if (RC) s_coef[e] = s_coef[e] * chr * nb;
                    else { // times chi1(g0) = conj(chr, chi), times n1(rep)
                        const double hr = s_coef[2 * e], hi = s_coef[2 * e + 1];
                        s_coef[2 * e] = (hr * chr + hi * chi) * nb;
                        s_coef[2 * e + 1] = (hi * chr - hr * chi) * nb;
                    }
                }
            }
            // ---- stage B2: representative -> source index, then the gathers (a thread's loads issued before any is used) --
            {
                uint64_t key[kGCCross], bucket[kGCCross];
                uint32_t tag[kGCCross];
                ulonglong2 first[kGCCross];
                int64_t idx[kGCCross];
                bool live[kGCCross];
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    const int e = tid + k * kBlock;
                    live[k] = e < n && s_row[e] != 0xffff;
                    key[k] = live[k] ? s_beta[e] : 0;
                    idx[k] = -1;
                    bucket[k] = 0; tag[k] = 0;
                    first[k] = make_ulonglong2(kGtEmpty, kGtEmpty);
                    if (live[k] && table && !(gt.L < 64 && (key[k] >> gt.L) != 0)) {
                        gt_split(gt, key[k], bucket[k], tag[k]);
                        first[k] = *(ulonglong2 const *)(gt.entries + 2 * bucket[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < kGCCross; ++k) {
                    if (!live[k]) continue;
                    if (table) {
                        const uint32_t pay = gt_resolve(gt, gt.entries, bucket[k], tag[k], first[k]);
                        idx[k] = pay == 0xffffffffu ? -1 : (int64_t)pay;
                    } else idx[k] = cross_index(six, key[k]);
                    if (idx[k] < 0 || idx[k] >= six.count) { idx[k] = -1; atomicExch(err, 1); } // an image that is not in the source basis
                    else ++found;
                }
                if constexpr (EMIT) {
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k)
                        if (idx[k] >= 0) atomicOr(&s_mask[s_row[tid + k * kBlock]], 1u << s_g[tid + k * kBlock]);
                    __syncthreads();
                    if (e_off) {
                        const int64_t slots = e_off[n_dst];
#pragma unroll
                        for (int k = 0; k < kGCCross; ++k) {
                            if (idx[k] < 0) continue;
                            const int e = tid + k * kBlock;
                            const int r = s_row[e];
                            const int64_t slot = s_base[r] + __popc(s_mask[r] & ((1u << s_g[e]) - 1u));
                            if (slot < 0 || slot >= slots) { atomicExch(err, 1); continue; } // (the counting pass saw another matrix)
                            e_out[slot] = idx[k];
                            if (CPLX) { y[2 * slot] = RC ? s_coef[e] : s_coef[2 * e]; y[2 * slot + 1] = RC ? 0.0 : s_coef[2 * e + 1]; }
                            else y[slot] = s_coef[e];
                        }
                    }
                } else if (!count) {
                    double xr[kGCCross], xi[kGCCross];
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k) {
                        xr[k] = 0.0; xi[k] = 0.0;
                        if (idx[k] >= 0) {
                            if (CPLX) { xr[k] = x[2 * idx[k]]; xi[k] = x[2 * idx[k] + 1]; } else xr[k] = x[idx[k]];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < kGCCross; ++k) {
                        if (idx[k] < 0) continue;
                        const int e = tid + k * kBlock;
                        double hr, hi = 0.0;
                        if (RC) hr = s_coef[e]; else { hr = s_coef[2 * e]; hi = s_coef[2 * e + 1]; }
                        const int r = s_row[e];
                        if (CPLX) {
                            atomicAdd(&s_acc[2 * r], hr * xr[k] - hi * xi[k]);
                            atomicAdd(&s_acc[2 * r + 1], hr * xi[k] + hi * xr[k]);
                        } else atomicAdd(&s_acc[r], hr * xr[k]);
                    }
                }
            }
            __syncthreads();
        }
        if constexpr (EMIT) { if (valid && !e_off) e_out[i] = s_base[tid] + __popc(s_mask[tid]); }
        else if (count) { if (found) atomicAdd(count, found); }
        else if (valid) {
            if (CPLX) { y[2 * i] = s_acc[2 * tid]; y[2 * i + 1] = s_acc[2 * tid + 1]; } else y[i] = s_acc[tid];
        }
        __syncthreads();
    }
}

// the launch of both units (who: the entry point, for its messages): {32, 64-bit words} x {f64 (real terms, +-1 characters) | c128 x
// {+-1, complex characters} x {real, complex terms}}: 10 kernels per unit.  d_count != NULL: nothing is read from x or written to y;
// the packets that reach a source row are added to *d_count
template <bool FERMI>
static int cross_pull_launch(char const *who, int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src,
                             lsk_index six, lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                             void const *x, void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", who); return -1; }
    if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", who); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
#define LSK_CX_ONE(W, PM1, CPLX, REAL)                                                                                                   \
    do {                                                                                                                                 \
        g.x = resident_grid(k_cross_pull<W, PM1, CPLX, REAL, FERMI>, work_blocks);                                                       \
        hipLaunchKernelGGL((k_cross_pull<W, PM1, CPLX, REAL, FERMI>), g, b, 0, s, n_groups, groups, terms, src, src.elems, six, gt,      \
                           n_dst, dst_reps, dst_norms, (double const *)x, (double *)y, tiny, d_count, d_err);                            \
    } while (0)
#define LSK_CX_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                 \
        if (!cplx) LSK_CX_ONE(W, true, false, true);                                                                                     \
        else if (src.chars_pm1) { if (is_real) LSK_CX_ONE(W, true, true, true); else LSK_CX_ONE(W, true, true, false); }                 \
        else { if (is_real) LSK_CX_ONE(W, false, true, true); else LSK_CX_ONE(W, false, true, false); }                                  \
    } while (0)
    if (src.number_sites <= 32) LSK_CX_LAUNCH(uint32_t); else LSK_CX_LAUNCH(uint64_t);
#undef LSK_CX_LAUNCH
#undef LSK_CX_ONE
    LSK_LAUNCH_CHECK();
    return 0;
}
