// k_cross.hip -- cross-sector operators: y2 = A x1 with x1 indexed by the representatives of a SOURCE basis and y2 by those of a
// TARGET basis (ls_amd_cross, host.c).  Pull form, modelled on k_tile_pull (k_pull.hip): one target row per thread, the adjoint's
// flip-mask groups expanded into an LDS packet list, every packet projected into the source basis and gathered from x1
//     y[r'] = sum_j conj(c+_j) chi1(g0j) n1(r) / n2(r') x[idx1(r)],    r = rep1(r' ^ x_j),  g0j (r' ^ x_j) = r
// (c+_j: coefficient of the adjoint's group j on r').  Only the norms and the look-up differ from the
// projection formula of section 6: they come from two bases.  Groups with flip mask 0 go through the same path -- row i of the
// target is not column i of the source.  No global atomics on y, y is assigned once per row.
#include "lsk_dev.hpp"

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

template <typename W, bool PM1, bool CPLX, bool REAL>
__global__ __launch_bounds__(kBlock) void k_cross_pull(int n_groups, lsk_group const *__restrict__ groups,
                                                       lsk_term const *__restrict__ terms, lsk_basis sbs,
                                                       lsk_group_elem const *__restrict__ elems, lsk_index six, lsk_gtab gt,
                                                       int64_t n_dst, uint64_t const *__restrict__ dst_reps,
                                                       double const *__restrict__ dst_norms, double const *__restrict__ x,
                                                       double *__restrict__ y, double tiny, unsigned long long *count, int *err) {
    constexpr bool RC = REAL && PM1; // the coefficient stays real: real terms and +-1 source characters
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
        if (CPLX) { s_acc[2 * tid] = 0.0; s_acc[2 * tid + 1] = 0.0; } else s_acc[tid] = 0.0;
        unsigned long long found = 0;
        for (int g0 = 0; g0 < n_groups; g0 += kGCCross) {
            if (tid == 0) s_n = 0;
            __syncthreads();
            // ---- stage A: the adjoint's groups of every row -> packets (state, conj(c) / n2(r'), row) ------------------
            const int g1 = min(g0 + kGCCross, n_groups);
            for (int g = g0; g < g1; ++g) {
                lsk_group const G = groups[g];
                double cr = 0.0, ci = 0.0;
                if (valid) term_sum<REAL>(terms, G.begin, G.end, a, cr, ci);
                // (tiny: the rounding residue of terms that cancel -- sum_j e^{-iqj} sigma^z_j on a state of shorter period -- is no packet)
                const bool act = valid && (fabs(cr) > tiny || (!REAL && fabs(ci) > tiny));
                const unsigned long long ball = __ballot(act);
                int base = 0;
                if (lane == 0 && ball) base = atomicAdd(&s_n, __popcll(ball));
                base = __shfl(base, 0);
                if (act) {
                    const int slot = base + __popcll(ball & ((1ULL << lane) - 1));
                    s_beta[slot] = a ^ G.x;
                    s_row[slot] = (uint16_t)tid;
                    if (RC) s_coef[slot] = cr * inv_na;
                    else { s_coef[2 * slot] = cr * inv_na; s_coef[2 * slot + 1] = -ci * inv_na; }
                }
            }
            __syncthreads();
            const int n = s_n;
            // ---- stage B1: project every packet into the SOURCE basis (general K4: minimum, character, stabiliser norm) --
            if (project) {
                for (int e = tid; e < n; e += kBlock) {
                    W rep; double chr, chi, stab;
                    state_info_w<W, PM1>(sbs, elems, (W)s_beta[e], rep, chr, chi, stab);
                    const double n2 = stab * sbs.inv_order;
                    if (!(n2 > 1e-12)) { s_row[e] = 0xffff; continue; } // zero norm in the source sector: contributes nothing
                    const double nb = sqrt(n2);
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
                if (!count) {
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
        if (count) { if (found) atomicAdd(count, found); }
        else if (valid) {
            if (CPLX) { y[2 * i] = s_acc[2 * tid]; y[2 * i + 1] = s_acc[2 * tid + 1]; } else y[i] = s_acc[tid];
        }
        __syncthreads();
    }
}

extern "C" char const *lsk_cross_kernel_name(void) { return "k_cross_pull"; }

// d_count != NULL: nothing is read from x or written to y; the packets that reach a source row are added to *d_count
extern "C" int lsk_cross_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                              lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x,
                              void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream) {
    if (src.fermi) { snprintf(g_err, sizeof(g_err), "%s: no permutation signs on this path (projected fermionic bases)", __func__); return -1; }
    if (n_dst <= 0 || n_groups <= 0) return 0;
    if (!cplx && !(is_real && src.chars_pm1)) { snprintf(g_err, sizeof(g_err), "%s: f64 needs a real operator and +-1 characters", __func__); return -1; }
    if (src.proj == LSK_PROJ_NONE && gt.entries) { snprintf(g_err, sizeof(g_err), "%s: an unprojected source is looked up by its index", __func__); return -1; }
    const int64_t work_blocks = (n_dst + kBlock - 1) / kBlock;
    hipStream_t s = (hipStream_t)stream;
    dim3 g(1), b(kBlock);
#define LSK_CX_ARGS n_groups, groups, terms, src, src.elems, six, gt, n_dst, dst_reps, dst_norms, (double const *)x, (double *)y, tiny, d_count, d_err
#define LSK_CX_ONE(W, PM1, CPLX, REAL)                                                                                                   \
    do { g.x = resident_grid(k_cross_pull<W, PM1, CPLX, REAL>, work_blocks); hipLaunchKernelGGL((k_cross_pull<W, PM1, CPLX, REAL>), g, b, 0, s, LSK_CX_ARGS); } while (0)
    // {32, 64-bit words} x {f64 (real terms, +-1 characters) | c128 x {+-1, complex characters} x {real, complex terms}}: 10 kernels
#define LSK_CX_LAUNCH(W)                                                                                                                 \
    do {                                                                                                                                 \
        if (!cplx) LSK_CX_ONE(W, true, false, true);                                                                                     \
        else if (src.chars_pm1) { if (is_real) LSK_CX_ONE(W, true, true, true); else LSK_CX_ONE(W, true, true, false); }                 \
        else { if (is_real) LSK_CX_ONE(W, false, true, true); else LSK_CX_ONE(W, false, true, false); }                                  \
    } while (0)
    if (src.number_sites <= 32) LSK_CX_LAUNCH(uint32_t); else LSK_CX_LAUNCH(uint64_t);
#undef LSK_CX_LAUNCH
#undef LSK_CX_ONE
#undef LSK_CX_ARGS
    LSK_LAUNCH_CHECK();
    return 0;
}
