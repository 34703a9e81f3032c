// k_pull_t.hpp -- the INDEXED pull kernel of the projected bases (k_pull_t) and what it needs, as a template header: k_pull.hip
// instantiates the spin kinds, k_fermi.hip the fermionic ones (own translation unit, so the hot units keep their device-function
// budget).  Moved out of k_pull.hip; it gained the fermionic K4 branch (discarded at compile time by the spin instantiations, whose
// machine code is unchanged) and pull_kinds the FERMI kinds.  NOTE: source_sha (scripts/kernel_isa_sha.py, bench.py) hashes the
// k_*.hip units, lsk_dev.hpp and lsk.h, not this header nor lsk_fermi.hpp: after an edit here, compare isa_sha, not source_sha.
#pragma once
#include "lsk_dev.hpp"
#include "lsk_fermi.hpp"

constexpr uint32_t kWinAbsent = 0xffffffffu; // offsets >= 2^32 - 1 are treated as "not in the window" (hash path)
__host__ __device__ __forceinline__ uint32_t window_offset(uint64_t rep, uint64_t v0) {
    const uint64_t d = rep - v0; // rep >= v0 inside the window (ascending)
    return d >= (uint64_t)kWinAbsent ? kWinAbsent : (uint32_t)d;
}

// value (and slot) of the key with home bucket b / tag: `cur` / `vals` are the home bucket's two halves, already loaded
__device__ __forceinline__ double vt_resolve(lsk_gtab const &t, uint64_t const *__restrict__ vt, uint64_t b, uint32_t tag, ulonglong2 cur,
                                             double2 vals, uint32_t &slot) {
    const uint64_t bmask = (1ULL << t.bbits) - 1;
    for (int d = 0;; ++d) {
        const uint32_t want = gt_hi(tag, d);
        if ((uint32_t)(cur.x >> 32) == want && cur.x != kGtEmpty) { slot = (uint32_t)cur.x; return vals.x; }
        if ((uint32_t)(cur.y >> 32) == want && cur.y != kGtEmpty) { slot = (uint32_t)cur.y; return vals.y; }
        if (cur.x == kGtEmpty || cur.y == kGtEmpty || d == kGtMaxDist) { slot = 0xffffffffu; return 0.0; }
        b = (b + 1) & bmask;
        cur = *(ulonglong2 const *)(vt + 4 * b);
        vals = *(double2 const *)(vt + 4 * b + 2);
    }
}

// ---------------------------------------------------------------------------------------------
// INDEXED pull kernels of the projected bases (k_pull_t / k_pull_gather).
//
// One block per 256-row tile, the packet list PER WAVE: each wave owns a 256-slot ring of the LDS list and the rows of its
// 64 lanes.  Stage A appends the packets of three flip-mask groups (<= 192) behind what is left in the ring, stage B takes
// full chunks of 64 packets out of it -- K4 with every lane busy -- and leaves the remainder (< 64) for the next round; the
// tile ends with one partial chunk.  No block barrier inside a tile except around the shared near window, so the four waves
// of a block drift apart and the ALU phase (K4) of one overlaps the look-ups of another.
//
// Stage B per packet: K4 (orbit minimum [+ character, norm]) -> SLOT of the representative:
//   near partners: the tile stages the sorted representatives [tile - halo, tile + 256 + halo) as a two-way hash set in LDS
//     (nw_*, below): one ds_read_b64 instead of the 11-step binary search of round 3; global index -> slot (perm[g] or g);
//   far partners: ONE 16-byte bucket of the static index table (lsk_gtab) -> slot.
// What happens with the slot is the SINK:
//   SINK_FUSED   : value = xsrc[slot], ds_add_f64 into the tile's LDS copy of y, y written once;
//   SINK_VALUE   : (round 6; f64, one partition) as FUSED, but a far partner costs ONE fabric request instead of two dependent
//                  ones: the table bucket is 32 bytes -- the two index entries AND the values x[slot] of both (lsk_vtab, below) --
//                  fetched by two 16-byte loads of one 64-byte line; the values are refreshed once per matvec in TABLE order
//                  (k_vtab_refresh: streaming over the table, one random read of x per representative);
//   SINK_RESOLVE : the slot (and, unless every packet has the same real amplitude, its coefficient) is written to the
//                  per-wave packet stream of lsk_pullbuf and NOTHING of x is read -- this half of the matvec runs while the
//                  blocks of x are still on the wire (ls_amd_repl_matvec, dist.c); k_pull_gather then streams the slots,
//                  gathers x and accumulates.  The stream is recomputed every matvec: the path stays matrix-free.
// ---------------------------------------------------------------------------------------------
constexpr int kWvRing = 256; // slots per wave: < 64 left over + 3 groups x 64 lanes
constexpr int kWvGroups = 3;
// what K4 has to deliver (lsk_basis.k4_mode != 0 -> TRIVIAL); the FERMI kinds are PM1 / GENERAL with the permutation sign of the
// state in every character (lsk_fermi.hpp), instantiated in k_fermi.hip only
enum { K4_TRIVIAL = 0, K4_PM1 = 1, K4_GENERAL = 2, K4_FERMI_PM1 = 3, K4_FERMI = 4 };
enum { COEF_UNI = 0, COEF_REAL = 1, COEF_CPLX = 2 };      // per-packet coefficient: none (one real amplitude), f64, 2 x f64
enum { SINK_FUSED = 0, SINK_RESOLVE = 1, SINK_VALUE = 2 };
constexpr uint32_t kNoSlot = 0xffffffffu;

// Near window as a hash set in LDS: kNwSets sets of two 4-byte entries.  h = d * odd constant is a bijection of the 32-bit
// offset d = rep - v0, set = top 10 bits, entry = (low 22 bits of h) << 10 | position in the window (< 1024) -- so set and
// tag together identify d and a match cannot be a false positive.  A set that is already full DROPS the third arrival: the
// window is only an accelerator, whatever it does not answer goes through the static index table (which holds every
// representative).  At <= 768 staged entries ~2 % are dropped.
constexpr int kNwSets = 1024;
constexpr int kNwMaxWin = 1024;
constexpr uint32_t kNwEmpty = 0xffffffffu;
__host__ __device__ __forceinline__ uint32_t nw_mix(uint32_t d) { return d * 0x9E3779B1u; }
__host__ __device__ __forceinline__ uint32_t nw_entry(uint32_t h, int pos) { return (h << 10) | (uint32_t)pos; }
__device__ __forceinline__ void nw_insert(uint32_t *tab, uint32_t d, int pos) {
    const uint32_t h = nw_mix(d), e = nw_entry(h, pos);
    uint32_t *s = tab + 2 * (h >> 22);
    if (atomicCAS(s, kNwEmpty, e) != kNwEmpty) (void)atomicCAS(s + 1, kNwEmpty, e);
}
__host__ __device__ __forceinline__ int nw_match(uint32_t e0, uint32_t e1, uint32_t h) {
    const uint32_t want = h << 10;
    if (((e0 ^ want) >> 10) == 0 && e0 != kNwEmpty) return (int)(e0 & 1023u);
    if (((e1 ^ want) >> 10) == 0 && e1 != kNwEmpty) return (int)(e1 & 1023u);
    return -1;
}
__device__ __forceinline__ int nw_find(uint32_t const *tab, uint32_t d) {
    const uint32_t h = nw_mix(d);
    const uint2 e = *reinterpret_cast<uint2 const *>(tab + 2 * (h >> 22));
    return nw_match(e.x, e.y, h);
}

constexpr int kPullXcdChunk = 256;
static int pull_xcd_chunk() { return kPullXcdChunk; }

template <typename W, int K4M, int COEF, bool CPLX, int SINK>
__global__ __launch_bounds__(kBlock, (COEF == COEF_CPLX ? 4 : 6)) void k_pull_t(lsk_runs runs, int n_groups, lsk_group const *__restrict__ groups,
                                                   lsk_term const *__restrict__ off, int n_diag,
                                                   lsk_term const *__restrict__ diag, lsk_basis bs,
                                                   lsk_group_elem const *__restrict__ elems, int64_t row0, int64_t row1,
                                                   uint64_t const *__restrict__ reps,
                                                   double const *__restrict__ norms_local, lsk_pullidx ix,
                                                   uint64_t const *__restrict__ greps, int64_t n_global,
                                                   double const *__restrict__ xsrc, int halo, double uni_v,
                                                   double *__restrict__ y, lsk_pullbuf buf, int *err, int xcd_chunk) {
    typedef typename ChainX<CPLX>::type X;
    constexpr bool REAL = COEF != COEF_CPLX;
    constexpr bool VALUE = SINK == SINK_VALUE;
    constexpr bool FUSED = SINK == SINK_FUSED || VALUE;
    static_assert(!(VALUE && CPLX), "the value table holds f64 values");
    constexpr int NC = COEF == COEF_UNI ? 0 : (COEF == COEF_REAL ? 1 : 2);
    X const *__restrict__ xv = (X const *)xsrc;
    constexpr int kCap = (kBlock / 64) * kWvRing;
    __shared__ uint32_t s_nw[2 * kNwSets];
    extern __shared__ uint32_t s_nwslot[]; // [kNwMaxWin] when ix.perm != NULL (launch-time size): slot of every window entry
    __shared__ W s_beta[kCap];
    __shared__ double s_coef[NC ? kCap * NC : 1];
    __shared__ uint8_t s_row[kCap]; // row inside the wave (0..63)
    __shared__ double s_acc[FUSED ? kBlock * (CPLX ? 2 : 1) : 1];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int rb = wave * kWvRing; // this wave's ring
    uint64_t const *__restrict__ tab = VALUE ? ix.vtab : ix.tab.entries;
    const int64_t n_tiles = (row1 - row0 + kBlock - 1) / kBlock;
    for (int64_t tb = blockIdx.x; tb < n_tiles; tb += gridDim.x) {
        const int64_t t0 = row0 + pull_tile_of_block(tb, n_tiles, gridDim.x >= n_tiles ? xcd_chunk : 0) * kBlock;
        const int64_t i = t0 + tid;
        const bool valid = i < row1;
        uint64_t a = 0;
        double inv_na = 0.0;
        if (valid) {
            a = reps[i];
            const double na = norms_local[i];
            inv_na = na > 0.0 ? 1.0 / na : 0.0;
        }
        if (FUSED) { if (CPLX) { s_acc[2 * tid] = 0.0; s_acc[2 * tid + 1] = 0.0; } else s_acc[tid] = 0.0; }
        // the diagonal coefficient now, not in the epilogue: the run tables then do not stay in scalar registers across stage B
        double dr = 0.0, di = 0.0;
        if (FUSED && valid && n_diag > 0) diag_coeff<uint64_t, REAL>(runs, n_diag, diag, a, dr, di);
        int64_t gbase = 0;
        int wn = 0;
        uint64_t v0 = 0;
        if (halo > 0) {
            const int64_t ig0 = ix.row_g0 + t0;
            gbase = ig0 > halo ? ig0 - halo : 0;
            const int64_t left = n_global - gbase;
            wn = (int)(left < (int64_t)(kBlock + 2 * halo) ? left : (int64_t)(kBlock + 2 * halo));
            v0 = greps[gbase];
            uint4 *const z = reinterpret_cast<uint4 *>(s_nw);
            for (int w = tid; w < 2 * kNwSets / 4; w += kBlock) z[w] = make_uint4(kNwEmpty, kNwEmpty, kNwEmpty, kNwEmpty);
            __syncthreads();
            for (int w = tid; w < wn; w += kBlock) {
                const uint32_t d = window_offset(greps[gbase + w], v0);
                if (d != kWinAbsent) nw_insert(s_nw, d, w);
                // replicated-x exchange: the slot of a near partner comes out of LDS (a coalesced load per window entry here)
                // instead of one dependent, uncoalesced load of perm[] per near packet
                if (ix.perm) s_nwslot[w] = ix.perm[gbase + w];
            }
        }
        __syncthreads(); // the window is staged
        int head = 0, cnt = 0; // wave-uniform: the ring holds [head, head + cnt) mod kWvRing
        // packet stream of this wave's 64 rows (SINK_RESOLVE)
        const int64_t wg = ((t0 - buf.row0) >> 6) + wave;
        const int64_t sbase = buf.offs ? buf.offs[wg] : wg * buf.cap; // exact layout (slot cache) | `cap` packets of room each
        int emitted = 0;
        // K chunks at once: the packets at ring positions head + 64 k + lane (the last chunk holds m <= 64 of them):
        // K4 -> slot [-> value -> ds_add_f64], the loads of the K packets of a lane issued together
        auto chunks = [&](auto KC, int m) {
            constexpr int K = decltype(KC)::value;
            uint64_t beta[K], bkt[K];
            double hr[K], hi[K];
            int r[K], pos[K];
            bool live[K];
            uint32_t tag[K], slot[K];
            ulonglong2 first[K];
            double2 fval[VALUE ? K : 1]; // SINK_VALUE: the value half of the home bucket
#pragma unroll
            for (int k = 0; k < K; ++k) {
                live[k] = k + 1 < K || lane < m;
                const int e = rb + ((head + 64 * k + lane) & (kWvRing - 1));
                beta[k] = live[k] ? (uint64_t)s_beta[e] : 0;
                hr[k] = 1.0; hi[k] = 0.0;
                if (NC == 1) hr[k] = s_coef[e];
                if (NC == 2) { hr[k] = s_coef[2 * e]; hi[k] = s_coef[2 * e + 1]; }
                r[k] = (int)s_row[e];
            }
            // the three x-independent steps of a chunk: K4, near window (LDS), first-level load (perm entry | home bucket)
            auto step_k4 = [&](int k) {
                if (kAblate && (bs.debug_ablate & 4)) return; // profiling builds: no K4 (the look-ups then mostly miss)
                if (K4M == K4_TRIVIAL) {
                    beta[k] = (uint64_t)rep_trivial<W>(bs, elems, (W)beta[k]); // xsrc is pre-multiplied by norm(rep)
                } else if (live[k]) {
                    W rep; double chr, chi, stab;
                    if constexpr (K4M == K4_FERMI_PM1 || K4M == K4_FERMI) // signed characters: the sign of g0 lands in (chr, chi)
                        fermi_state_info_w<W, K4M == K4_FERMI_PM1>(bs, elems, (W)beta[k], rep, chr, chi, stab);
                    else state_info_w<W, K4M == K4_PM1>(bs, elems, (W)beta[k], rep, chr, chi, stab);
                    const double n2 = stab * bs.inv_order;
                    if (!(n2 > 1e-12)) live[k] = false; // zero-norm orbit: contributes nothing (DMV:110)
                    else {
                        const double nb = sqrt(n2);
                        beta[k] = (uint64_t)rep;
                        const double tr = (hr[k] * chr + hi[k] * chi) * nb, ti = (hi[k] * chr - hr[k] * chi) * nb;
                        hr[k] = tr; hi[k] = ti;
                    }
                }
            };
            auto step_window = [&](int k) { // near window: LDS only
                pos[k] = -1; bkt[k] = 0; tag[k] = 0; slot[k] = kNoSlot;
                first[k] = make_ulonglong2(0, 0);
                if (kAblate && (bs.debug_ablate & 2)) { // profiling builds: K4 kept alive, no look-up, no accumulation
                    if (beta[k] == 0x123456789abcdefULL) atomicExch(err, 2);
                    live[k] = false;
                }
                if (live[k]) {
                    if (wn > 0 && beta[k] >= v0 && !(kAblate && (bs.debug_ablate & 32))) {
                        const uint32_t d = window_offset(beta[k], v0);
                        if (d != kWinAbsent) pos[k] = nw_find(s_nw, d);
                    }
                    if (pos[k] < 0) gt_split(ix.tab, beta[k], bkt[k], tag[k]);
                }
            };
            auto step_first = [&](int k) { // first-level loads: perm entry (near) or home bucket (far)
                if (!live[k]) return;
                if (pos[k] >= 0) slot[k] = ix.perm ? s_nwslot[pos[k]] : (uint32_t)(gbase + pos[k]);
                else if constexpr (VALUE) { // both halves of the 32-byte bucket at once: one line, one fabric request
                    first[k] = *(ulonglong2 const *)(tab + 4 * bkt[k]);
                    fval[k] = *(double2 const *)(tab + 4 * bkt[k] + 2);
                } else first[k] = *(ulonglong2 const *)(tab + 2 * bkt[k]);
            };
            // (step by step over the chunks.  Chunk by chunk instead -- the home-bucket load of chunk k in flight while chunk k + 1 runs
            // its K4 -- measured no different: chain_36_symm 17.61 vs 17.72 ms, chain_40_symm 276.5 vs 277.9 ms,
            // profiles/r5_pull_skew_ab.txt: the kernel is at the fabric's random-request rate, not at a latency it could hide)
#pragma unroll
            for (int k = 0; k < K; ++k) step_k4(k);
#pragma unroll
            for (int k = 0; k < K; ++k) step_window(k);
#pragma unroll
            for (int k = 0; k < K; ++k) step_first(k);
            [[maybe_unused]] double far_val[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                far_val[k] = 0.0;
                if (!live[k] || pos[k] >= 0) continue;
                if constexpr (VALUE) far_val[k] = vt_resolve(ix.tab, tab, bkt[k], tag[k], first[k], fval[k], slot[k]);
                else slot[k] = gt_resolve(ix.tab, tab, bkt[k], tag[k], first[k]);
                if (slot[k] == kNoSlot) { atomicExch(err, 1); live[k] = false; }
            }
            if constexpr (FUSED) {
                X val[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if constexpr (VALUE) { // far partners brought their value with the bucket; near ones read x next to the tile
                        val[k] = !live[k] ? 0.0 : (pos[k] >= 0 ? xv[slot[k]] : far_val[k]);
                    } else val[k] = (live[k] && !(kAblate && (bs.debug_ablate & 64))) ? xv[slot[k]] : cx_zero<X>();
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (!live[k]) continue;
                    const int ra = (wave << 6) + r[k];
                    if constexpr (CPLX) {
                        atomicAdd(&s_acc[2 * ra], hr[k] * val[k].x - hi[k] * val[k].y);
                        atomicAdd(&s_acc[2 * ra + 1], hr[k] * val[k].y + hi[k] * val[k].x);
                    } else if constexpr (NC == 0) {
                        atomicAdd(&s_acc[ra], val[k]);
                    } else {
                        atomicAdd(&s_acc[ra], hr[k] * val[k]);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k + 1 == K && lane >= m) continue;
                    const int64_t o = sbase + emitted + 64 * k + lane;
                    __builtin_nontemporal_store(live[k] ? slot[k] : kNoSlot, buf.slots + o);
                    __builtin_nontemporal_store((uint8_t)r[k], buf.rows + o);
                    if (NC == 1) __builtin_nontemporal_store(hr[k], buf.coefs + o);
                    if (NC == 2) { __builtin_nontemporal_store(hr[k], buf.coefs + 2 * o); __builtin_nontemporal_store(hi[k], buf.coefs + 2 * o + 1); }
                }
                emitted += 64 * (K - 1) + m;
            }
        };
        const W tdiff = (W)a ^ (W)((W)a >> 1); // bit b set: sites b, b + 1 differ (adjacent exchange groups)
        for (int g0 = 0; g0 < n_groups; g0 += kWvGroups) {
            const int g1 = min(g0 + kWvGroups, n_groups);
            for (int g = g0; g < g1; ++g) { // stage A: append
                lsk_group const G = groups[g];
                double cr = 0.0, ci = 0.0;
                bool act;
                if (NC == 0) { // every group is an exchange pair with the amplitude uni_v
                    act = valid && (G.adj >= 0 ? (bool)((tdiff >> G.adj) & 1) : WordTraits<W>::popc((W)a & (W)G.x) == 1);
                } else {
                    if (valid) group_coeff<REAL>(G, off, a, cr, ci);
                    act = valid && (cr != 0.0 || (!REAL && ci != 0.0));
                }
                const unsigned long long ball = __ballot(act);
                if (act) {
                    const int slot = rb + ((head + cnt + __popcll(ball & ((1ULL << lane) - 1))) & (kWvRing - 1));
                    s_beta[slot] = (W)(a ^ G.x);
                    s_row[slot] = (uint8_t)lane;
                    if (NC == 1) s_coef[slot] = cr * inv_na;
                    if (NC == 2) { s_coef[2 * slot] = cr * inv_na; s_coef[2 * slot + 1] = -ci * inv_na; }
                }
                cnt += __popcll(ball);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (kAblate && (bs.debug_ablate & 1)) { head = (head + cnt) & (kWvRing - 1); cnt = 0; } // profiling builds: stage A only
            // stage B on full chunks: two at a time while the ring has them (trivial sectors; the element loops of the other
            // sectors are long enough by themselves, and two chunks of their state do not fit the scalar registers)
            constexpr int KMAX = K4M == K4_TRIVIAL ? 2 : 1;
            while (cnt >= 64 * KMAX) {
                chunks(std::integral_constant<int, KMAX>(), 64);
                head = (head + 64 * KMAX) & (kWvRing - 1);
                cnt -= 64 * KMAX;
            }
            if constexpr (KMAX == 2)
                if (cnt >= 64) {
                    chunks(std::integral_constant<int, 1>(), 64);
                    head = (head + 64) & (kWvRing - 1);
                    cnt -= 64;
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (cnt > 0) chunks(std::integral_constant<int, 1>(), cnt);
        if constexpr (FUSED) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (valid) {
                const int64_t ig = ix.row_g0 + i;
                const uint32_t own = ix.perm ? ix.perm[ig] : (uint32_t)ig;
                const double back = K4M == K4_TRIVIAL ? inv_na : 1.0; // xsrc holds x * norm(rep) in the prescaling K4 modes
                const double sc = NC == 0 ? uni_v * inv_na : 1.0;     // one amplitude for every packet: applied once per row
                if constexpr (CPLX) {
                    const X xo = xv[own];
                    const double xr = xo.x * back, xi = xo.y * back;
                    double yr = dr * xr - di * xi + sc * s_acc[2 * tid], yi = dr * xi + di * xr + sc * s_acc[2 * tid + 1];
                    if (n_diag == 0) { yr += y[2 * i]; yi += y[2 * i + 1]; } // accumulate, DMV:1062-1063
                    y[2 * i] = yr; y[2 * i + 1] = yi;
                } else {
                    double yr = n_diag > 0 ? dr * (xv[own] * back) + sc * s_acc[tid] : sc * s_acc[tid];
                    if (n_diag == 0) yr += y[i];
                    y[i] = yr;
                }
            }
        } else if (lane == 0) buf.counts[wg] = (uint32_t)emitted;
        __syncthreads(); // every wave is done with the window
    }
}

// kind of K4 work and of per-packet coefficient for (operator, basis) -- one decision for the fused, the resolve and the
// gather kernel
static void pull_kinds(lsk_operator const &op, lsk_basis const &bs, int &k4m, int &coef) {
    if (bs.k4_mode != 0) { k4m = K4_TRIVIAL; coef = !op.is_real ? COEF_CPLX : (op.uni ? COEF_UNI : COEF_REAL); }
    else if (bs.chars_pm1) { k4m = bs.fermi ? K4_FERMI_PM1 : K4_PM1; coef = op.is_real ? COEF_REAL : COEF_CPLX; }
    else { k4m = bs.fermi ? K4_FERMI : K4_GENERAL; coef = COEF_CPLX; }
}
template <typename W, int K4M, int COEF, bool CPLX, int SINK>
static void launch_pull_t(lsk_operator const &op, lsk_basis const &bs, int64_t row0, int64_t row1, uint64_t const *reps,
                          double const *norms_local, lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global, void const *xsrc,
                          int halo, void *y, lsk_pullbuf buf, int *d_err, hipStream_t s) {
    const int64_t work_blocks = (row1 - row0 + kBlock - 1) / kBlock;
    dim3 g((unsigned)tile_grid(k_pull_t<W, K4M, COEF, CPLX, SINK>, work_blocks)), b(kBlock);
    const size_t dyn = ix.perm ? sizeof(uint32_t) * kNwMaxWin : 0;
    hipLaunchKernelGGL((k_pull_t<W, K4M, COEF, CPLX, SINK>), g, b, dyn, s, op.runs, op.n_groups, op.groups, op.off, op.n_diag, op.diag, bs,
                       bs.elems, row0, row1, reps, norms_local, ix, reps_global, n_global, (double const *)xsrc, halo, op.uni_v,
                       (double *)y, buf, d_err, pull_xcd_chunk());
}
