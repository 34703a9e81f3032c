/* lsk.h -- internal interface between the C host side (host.c) and the HIP side (k_*.hip: runtime, rows, packets, pull, plan; shared device code in lsk_dev.hpp).
 * "Thin extern-C shim": host.c never includes a HIP header; everything device-related goes through
 * the lsk_* functions declared here.  All structs are plain C PODs passed by value to kernels.
 */
#ifndef LSK_H
#define LSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSK_BENES_STAGES 11 /* distances 32,16,8,4,2,1,2,4,8,16,32 */
#define LSK_BINOM_K 34      /* binomial table is [64][LSK_BINOM_K]: C(n, k), n < 64, k < 34 */
#define LSK_MAX_PARTS 256   /* DMV:664 */

typedef struct lsk_term {
    double v_re, v_im;
    uint64_t m, r, s;
} lsk_term;

/* how the coefficient of a flip-mask group is evaluated */
enum { LSK_GROUP_GENERIC = 0, LSK_GROUP_EXCHANGE = 1,
       /* round 6: a DIRECTED pair, e.g. sigma^+_i sigma^-_j -- coefficient v iff exactly ONE site of the pair is set in alpha and it is
        * the pair's lower (HOP_LO) / upper (HOP_HI) site.  Non-Hermitian hopping then takes the same fast paths as an exchange. */
       LSK_GROUP_HOP_LO = 2, LSK_GROUP_HOP_HI = 3 };

/* one off-diagonal flip-mask group: beta = alpha ^ x, coefficient = sum over terms [begin, end) */
typedef struct lsk_group {
    uint64_t x;
    double v_re, v_im; /* EXCHANGE: coefficient when popcount(alpha & x) == 1, else 0; HOP_*: when alpha & x is the source site alone */
    int32_t begin, end;
    int32_t adj;       /* lo if x == 3 << lo (adjacent pair) else -1 */
    int32_t fast;      /* LSK_GROUP_* */
} lsk_group;

/* Structure the host recognises so that the row kernels can run tight, branch-free inner loops:
 *  - exchange runs: groups [0, n_run_groups) are EXCHANGE groups on adjacent pairs (lo, lo + 1) with
 *    consecutive lo and one common amplitude v  (e.g. the 31 open bonds of the Heisenberg ring);
 *  - zz runs: diagonal terms [0, n_zz_terms) are v * (-1)^popcount(alpha & (3 << lo)) with
 *    consecutive lo and a common real v, whose sum is v * (cnt - 2 * #anti-aligned pairs). */
#define LSK_MAX_RUNS 4
typedef struct lsk_runs {
    int n_runs, n_run_groups;
    int lo0[LSK_MAX_RUNS], cnt[LSK_MAX_RUNS]; /* cnt: pairs in the run | direction << 16 (0: exchange, 1: HOP_LO, 2: HOP_HI groups; k_direct
                                               * decodes it -- the staged chain kernel only ever sees Hermitian operators, i.e. direction 0) */
    double v_re[LSK_MAX_RUNS], v_im[LSK_MAX_RUNS];
    int n_zz, n_zz_terms;
    int zz_lo0[LSK_MAX_RUNS], zz_cnt[LSK_MAX_RUNS];
    double zz_v[LSK_MAX_RUNS];
} lsk_runs;

typedef struct lsk_operator {
    int n_diag, n_off, n_groups, is_real;
    int uni;      /* every off-diagonal group is an exchange pair (LSK_GROUP_EXCHANGE) with ONE real amplitude uni_v: the projected */
    double uni_v; /* pull kernels then keep no coefficient per packet */
    lsk_term const *diag;    /* device [n_diag]; zz-run terms first */
    lsk_term const *off;     /* device [n_off], sorted by group */
    lsk_group const *groups; /* device [n_groups]; exchange-run groups first */
    lsk_runs runs;
} lsk_operator;

enum { LSK_ELEM_BENES = 0, LSK_ELEM_ROT = 1, LSK_ELEM_REVROT = 2 };
/* Elements of a projected spinful-fermion basis that are a ring rotation / reflection of the sites lifted to both species (the
 * state word has 2 h bits: up half = bits 0..h-1, down half = bits h..2h-1): kind = LSK_ELEM_LIFT | flags, k = the site
 * element's rotate-right amount within h bits.  REV: every half is reversed first (as REVROT); SWAP: the halves are exchanged
 * afterwards (the up <-> down flip).  Only the fermionic code knows these kinds (fermi_apply_elem_w / fermi_parity, lsk_fermi.hpp;
 * host_apply_elem, host.c): apply_elem and the spin kernels never see them, and the element keeps its compiled network in `masks`. */
enum { LSK_ELEM_LIFT = 4, LSK_ELEM_LIFT_REV = 1, LSK_ELEM_LIFT_SWAP = 2 };

typedef struct lsk_group_elem {
    int32_t kind;
    int32_t k; /* rotate-right amount within number_sites bits (ROT / REVROT) */
    double ch_re, ch_im;
    uint64_t masks[LSK_BENES_STAGES];
} lsk_group_elem;

enum { LSK_PROJ_NONE = 0, LSK_PROJ_INVERSION = 1, LSK_PROJ_FULL = 2 };

typedef struct lsk_basis {
    int number_sites, hamming_weight, spin_inversion, n_elems, proj;
    int chars_pm1; /* every character is +1 or -1 (integer stabiliser accumulation) */
    /* K4 evaluation mode of the staged kernel:
     *  0 general: orbit minimum + character + stabiliser norm per packet;
     *  1 trivial sector (every character, incl. inversion, is +1): only the orbit minimum is needed,
     *    norm(rep) is read from the owner's per-row norms when the index is looked up;
     *  2 as 1, and the permutation group is the full cyclic (rotation) group of the ring, with
     *    (reflect = 1) or without its reflections: rotations are generated incrementally;
     *  3 as 2, but only the rotations that start at a longest run of zeros are visited;
     *  4 as 1, for a group that contains every translation of a tw x (L / tw) torus (site = y tw + x): G = union of the
     *    right cosets T g_r, so the orbit is { t(g_r(a)) }: n_cosets compiled networks (the point group) and |G| cheap
     *    translation steps (rotate the rows by one site / the word by one row) instead of |G| networks.
     *  5 as 4, when those cosets are (modulo translations) the point group D2 = {1, r, o, r o} of the torus -- r reverses every
     *    row, o the order of the rows -- or, on a square torus, D4 = D2 x {1, transpose}, or a subgroup of it: d4_mask says
     *    which images belong to the group (bits 0-3: 1, r, o, r o of the word; bits 4-7: of its transpose), cosets[0] is the
     *    transpose network -- the only compiled network left -- and trow2 the row table with the fields of the reversed row
     *    in its high half (torus_min_d2, lsk_dev.hpp). */
    int k4_mode, reflect;
    int d4_mask;                    /* mode 5 */
    /* projected fermionic basis (spinless, or spinful over its 2 L modes): every group element carries the permutation sign of the
     * Fock state (include/ls_hs.h);
     * always K4 mode 0, so the mode-5 row table is never read and its pointer slot holds the sign table instead (the layout of
     * this struct, which every kernel receives by value, stays as it was) */
    int fermi;
    union {
        uint64_t const *trow2;      /* mode 5: device [2^tw] */
        uint64_t const *fsign;      /* fermi: device [n_elems][number_sites] -- B_g[i] = the modes j < i that g puts above i */
    };
    int tw, n_cosets;               /* mode 4 / 5 */
    uint64_t tcol0;                 /* mode 4: the bits of column x = 0 */
    lsk_group_elem const *cosets;   /* mode 4: device [n_cosets] */
    uint32_t const *trow;           /* mode 4, tw <= 8: device [2^tw] row table of torus_min (lsk_torus_rowtab), else NULL */
    int debug_ablate; /* LS_AMD_ABLATE bitmask (profiling only): 1 skip stage B, 2 skip lookup+accumulate, 4 skip K4 */
    uint64_t site_mask;
    double inv_order; /* 1 / |G| including the inversion doubling */
    lsk_group_elem const *elems; /* device [n_elems] */
} lsk_basis;

/* PRODUCT: the spinful-fermion basis with fixed (N_up, N_down) on L sites -- index = rank(high L bits) * n_low + rank(low L bits),
 * two colex ranks (prod_* fields of lsk_index); -1 when a half has the wrong weight */
enum { LSK_INDEX_IDENTITY = 0, LSK_INDEX_COMBINADIC = 1, LSK_INDEX_SEARCH = 2, LSK_INDEX_PRODUCT = 3 };

/* Rank directory of a hash partition of an unprojected fixed-weight basis (optional part of a SEARCH index): the global
 * (colex) rank g of a state is closed-form, and the local index is the number of this partition's states below it --
 *     entry = dir[g >> 6];  local = entry.prefix + popcount(entry.bits & below(g));  member <=> bit g of entry.bits
 * one 16-byte load instead of the prefix-table look-up and the 3-4 dependent probes of the binary search. */
typedef struct lsk_rankdir {
    uint64_t bits;   /* bit j: global rank 64 w + j belongs to this partition */
    uint32_t prefix; /* states of this partition with global rank < 64 w */
    uint32_t pad;
} lsk_rankdir;

typedef struct lsk_index {
    int kind;
    int shift;             /* SEARCH: bucket = state >> shift */
    int64_t count;
    uint64_t const *reps;  /* device, ascending */
    uint32_t const *table; /* device [(max_state >> shift) + 2] lower bounds */
    uint64_t const *binom; /* device [64 * LSK_BINOM_K] */
    lsk_rankdir const *dir; /* device [ceil(C(dir_sites, dir_weight) / 64)] or NULL */
    int dir_sites, dir_weight;
    int prod_sites, prod_up, prod_dn; /* PRODUCT: L, weight of the low / high half */
    int64_t prod_na;                  /* PRODUCT: C(L, prod_up) */
} lsk_index;
/* dir[] for the n ascending states `reps` (all of weight `weight` on `sites` sites), entries = ceil(C(sites, weight) / 64); *d_flag is
 * raised if a state has another weight or the directory does not give reps[i] -> i back */
int lsk_rankdir_build(int64_t n, uint64_t const *reps, int sites, int weight, uint64_t const *d_binom, int64_t entries, lsk_rankdir *dir,
                      int *d_flag, void *stream);

/* All-destinations rank directory of the hash partition of an unprojected fixed-weight basis (pre-indexed packets): entry
 * [w * P + d] describes what partition d owns of the global (colex) ranks [64 w, 64 w + 64).  The owner of a state is a hash
 * of the state, so every rank builds the whole table by itself (unrank -> owner, one pass over the basis at plan time).  The
 * PRODUCER of a packet then knows the index of beta inside its destination's block:
 *     idx = e.prefix + popcount(e.bits & below(g)),  e = entries[(g >> 6) * P + owner(beta)],  member <=> bit g & 63 of e.bits
 * and sends (u32 idx, value): 12 instead of 16 bytes per packet, and the consumer is search-free.  P / 4 bytes per basis state. */
typedef struct lsk_gdir {
    lsk_rankdir const *entries; /* device [words * P]; NULL = no directory (packets carry the state) */
    int P, sites, weight;
    int64_t n_ranks;            /* global ranks [0, n_ranks) are basis states (C(sites, weight), or its lower half under inversion) */
} lsk_gdir;
/* entries: ceil(n_ranks / 64) * P, allocated by the caller; synchronises the stream */
int lsk_gdir_build(lsk_gdir gd, lsk_rankdir *entries, uint64_t const *d_binom, void *stream);
/* *d_flag is raised unless the directory gives reps[i] -> (part, i) back for the n ascending states of partition `part` */
int lsk_gdir_check(lsk_gdir gd, int part, int64_t n, uint64_t const *reps, uint64_t const *d_binom, int *d_flag, void *stream);

/* the segments of one fused consumer launch (one round's receive buffer, or the send buffer of a logical partition) */
#define LSK_MAX_SEGS 64
typedef struct lsk_segs {
    int n;
    int64_t start[LSK_MAX_SEGS + 1]; /* exclusive prefix of the packet counts */
    int64_t key_off[LSK_MAX_SEGS];   /* byte offset of the segment's u64 states / u32 indices */
    int64_t val_off[LSK_MAX_SEGS];   /* ... of its values */
    void *y[LSK_MAX_SEGS];           /* the vector the segment accumulates into (all the same with one partition per process) */
    uint8_t part[LSK_MAX_SEGS];      /* lsk_scatter_parts: the partition (entry of the context array) the segment belongs to */
} lsk_segs;
/* what a consumer needs to know of a destination partition: all partitions of one process (lsk_scatter_parts) */
/* static index table {state -> payload} (k_pull.hip; look-up: lsk_dev.hpp) */
typedef struct lsk_gtab {
    uint64_t const *entries; /* device [2 << bbits] */
    int L, bbits, tbits;
} lsk_gtab;
typedef struct lsk_part_ctx {
    lsk_index ix;
    double const *norms; /* per-row norms multiplied in (K4 modes that prescale), else NULL */
    lsk_gtab gt;         /* entries != NULL: {representative -> index} of the partition -- one 16-byte probe instead of the prefix table
                          * and the binary search (round 6; searched indexes, i.e. projected bases) */
} lsk_part_ctx;
/* every packet of every segment: y[seg][idx] += value; pre-indexed packets (u32 idx) */
int lsk_scatter_idx(int cplx, lsk_segs const *segs, void const *base, void *stream);
/* state-carrying packets whose segments belong to DIFFERENT partitions of this process (logical partitions on one device): the
 * index / norms of segment s are d_parts[segs->part[s]] (device array); all partitions share sites / weight of the rank directory */
int lsk_scatter_parts(lsk_part_ctx const *d_parts, lsk_index any, int cplx, lsk_segs const *segs, void const *base, int *d_err, void *stream);
/* the same for packets that carry the state: ONE index (all segments belong to the same destination partition) */
int lsk_scatter_segs(lsk_index ix, lsk_gtab gt, int cplx, lsk_segs const *segs, void const *base, double const *norms, int *d_err, void *stream);

/* per-round send layout: byte offsets of the beta / value arrays of every destination segment */
typedef struct lsk_round_layout {
    int64_t beta_off[LSK_MAX_PARTS];
    int64_t val_off[LSK_MAX_PARTS];
} lsk_round_layout;

/* Tile map of the row kernels: entry = first row | number of rows (<= 256) << 48.  The map holds 8 lists of
 * slots_per_xcd entries, one per XCD (block b of the launch runs on XCD b % 8 and walks list b % 8);
 * empty slots have a zero row count.  Every row appears in exactly one tile. */
typedef struct lsk_tilemap {
    uint64_t const *entries; /* device [8 * slots_per_xcd] */
    int64_t slots_per_xcd;
} lsk_tilemap;

/* runtime ---------------------------------------------------------------------------------- */
char const *lsk_last_error(void);
int lsk_ablate_mask(void); /* profiling builds (make ablate): the LS_AMD_ABLATE stage switches; the shipped library returns 0 */
int lsk_device_count(void);
int lsk_set_device(int device);
int lsk_malloc(void **p, size_t bytes);
int lsk_free(void *p);
int lsk_mem_info(size_t *free_bytes, size_t *total_bytes);
int lsk_h2d(void *dst, void const *src, size_t bytes);
int lsk_d2h(void *dst, void const *src, size_t bytes);
int lsk_d2d_async(void *dst, void const *src, size_t bytes, void *stream);
int lsk_memset_async(void *p, int value, size_t bytes, void *stream);
int lsk_sync(void *stream);
int lsk_device_sync(void);
/* dst[i * dst_stride] = src[i * src_stride] for i < n, elements of elt_size bytes (strides in elements) */
int lsk_copy_strided(int64_t n, int elt_size, void const *src, int64_t src_stride, void *dst, int64_t dst_stride, void *stream);

/* host <-> HBM staging of the host-pointer entry points (stage.cpp) ---------------------------- */
enum { LSK_PTR_PAGEABLE = 0, LSK_PTR_PINNED = 1, LSK_PTR_DEVICE = 2,
       LSK_PTR_MANAGED = 3 /* hipMallocManaged: fine-grained unless advised otherwise -- never used in place (the push kernels'
                            * global_atomic_add_f64 is specified for coarse-grained memory only); staged by one DMA like pinned memory */ };
char const *lsk_stage_last_error(void);
int lsk_pointer_kind(void const *p); /* hipPointerGetAttributes: device, managed, pinned or registered host, anything else */
int lsk_host_register(void *p, size_t bytes);
int lsk_host_unregister(void *p);
typedef struct lsk_stager lsk_stager;
int lsk_stager_create(lsk_stager **out, size_t chunk_bytes, int threads /* <= 0: min(16, cores / 4) */);
void lsk_stager_destroy(lsk_stager *st);
int lsk_stager_threads(lsk_stager const *st);
size_t lsk_stager_chunk(lsk_stager const *st);
/* one upload and one download at the same time (either may have 0 bytes); *_kind = LSK_PTR_PAGEABLE (double-buffered pinned
 * bounce chunks, host copies by the stager's thread pool) or LSK_PTR_PINNED (one DMA); returns when both are complete */
int lsk_stage_run(lsk_stager *st, void *d_up, void const *h_up, size_t up_bytes, int up_kind, void *h_down, void const *d_down,
                  size_t down_bytes, int down_kind);

/* events (kernel timing on the launch stream) */
int lsk_event_create(void **ev);
int lsk_event_destroy(void *ev);
int lsk_event_record(void *ev, void *stream);
int lsk_event_elapsed_ms(void *start, void *stop, float *ms);

/* deterministic test / bench vectors keyed by the basis state: x_i = u(hash(state_i, seed)) - 0.5 */
int lsk_fill_random(int64_t n, uint64_t const *states, uint64_t seed, int cplx, void *out, void *stream);

/* hot path --------------------------------------------------------------------------------- */
/* y[i] = d(reps[i]) * x[i] */
int lsk_diag(lsk_operator op, int cplx, int64_t n, uint64_t const *reps, void const *x, void *y,
             void *stream);
/* fused single-partition kernel without permutation symmetries (row per lane).
 * pull == 0: y[idx(beta)] += c x[i] (atomics; y must already hold the diagonal part)
 * pull == 1: y[i] = d x[i] + sum conj(c) x[idx(beta)] */
/* plan-time check of a pull plan over a non-Hermitian operator: raises *d_err when the row expansion of some basis state leaves the basis */
int lsk_direct_validate(lsk_operator op, lsk_basis bs, lsk_index ix, int64_t n, uint64_t const *reps, int *d_err, void *stream);
int lsk_direct(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, int pull, lsk_tilemap tm,
               uint64_t const *reps, void const *x, void *y, int *d_err, void *stream);
/* staged row kernel (k_chain_t): pull, real Hermitian operator, the full fixed-Hamming-weight basis without symmetries
 * (<= 64 sites; f64 or c128 vectors).  The tile map must have been built with lsk_chain_tile_rows(cplx)-row tiles.  The n
 * rows (reps, cache, y) are the global rows [row0, row0 + n) of the basis; x is the whole vector of n_x elements.
 * wide_ranks != 0: ranks (cache entries, indices into x) are 64-bit (bases with >= 2^32 states).
 * wave_plan (<= 32 sites with 32-bit ranks, else NULL): the word table + wave headers of lsk_chain_headers; wave-rows with a header read
 * it instead of their records. */
int lsk_chain_tile_rows(int cplx);
int lsk_chain(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, int wide_ranks, int fused_records, lsk_tilemap tm,
              int64_t n, uint64_t const *reps, int64_t row0, int64_t n_x, void const *x, void *y, int n_cached,
              void const *cache, double cv0, double cv1, void const *wave_plan, void *stream);
/* The paired launch (k_chain_pair_t) next to lsk_chain() of a plan with 32-bit states and ranks, f64 vectors, fused records and wave
 * headers, row0 == 0 and n_x == n.  tm_pair holds TWO u64 per slot (8 lists of 2 * slots_per_xcd words): the entry of the tile -- its
 * first row i0 in bits 0..31, its range in bits 32..47, 1024 rows; 0 = empty slot -- and d | h << 32 | bond << 59: the rows
 * [i0, i0 + 512) and [i0 + d, i0 + d + 512) are mapped onto each other row by row by `bond`, a far pair (>= 12) inside one of the
 * operator's runs, and the wave headers of rows i0 + d ... are entries h ... of hdr_b (8 bytes each; h < 2^27).  hdr_b = the
 * lsk_chain_headers of every range's second segments, each made from that range's first such row on (they lie off the 64-row grid of
 * the plan's headers).  The plan's other tile map leaves all those rows out. */
int lsk_chain_paired(lsk_operator op, lsk_basis bs, lsk_tilemap tm_pair, int64_t n, uint64_t const *records, void const *x, void *y,
                     int n_cached, double cv0, void const *wave_plan, void const *hdr_b, void *stream);
/* ---- staged row kernel for arbitrary exchange pairs (k_pairs_t, k_rows.hip): Heisenberg / XXZ on any lattice -------------
 * pairs are sorted by class: [0, n_near) both sites below bit 11, [n_near, n_near + n_str) i < 11 <= j, then both >= 11 */
#define LSK_MAX_PAIRS 128
#define LSK_PAIR_KC 20 /* columns of the binomial table: weight + 2 <= 20, i.e. hamming weight <= 18 (32 sites: 16) */
typedef struct lsk_pair {
    uint8_t i, j, pad[6]; /* i < j */
    double v;             /* exchange amplitude: coefficient of |..0_i..1_j..><..1_i..0_j..| + h.c. */
    double vz;            /* diagonal: vz (-1)^{[bits i, j differ]} */
} lsk_pair;
/* the same pair as the one-row-per-lane variant reads it (k_pairs_row): the masks its rank shift needs, ready-made */
typedef struct lsk_pair_row {
    uint64_t between; /* sites strictly between i and j */
    double v, vz;
    int i, j;         /* i < j */
} lsk_pair_row;
/* ... and as the one-row-per-lane variant that walks the PARTICLES of a row reads it (k_pairs_site): one table of 32-bit words,
 *   [n_sites][degree / 4]  the neighbours of every site, one byte each (slots past the degree of a site hold the site itself:
 *                          never active, it is occupied)
 *   [n_sites][degree / 4]  the amplitude class of every slot, one byte each
 *   [n_classes] x {double v, vz}   (starts on a 16-byte boundary)
 * n_classes == 1 -- one J for all bonds -- keeps v and vz in scalar registers and never reads the class words. */
#define LSK_PAIR_SITE_MAX_DEGREE 8
#define LSK_PAIR_SITE_MAX_CLASSES 64
typedef struct lsk_pairplan {
    int n_near, n_str, n_high;
    lsk_pair const *pairs;     /* device [n_near + n_str + n_high] */
    uint16_t const *rank_low;  /* device [2048]: rank of an 11-bit word among the words of its weight */
    uint32_t const *binom;     /* device [32 | 64][LSK_PAIR_KC] */
    void const *states;        /* device [n]: u32 low words of the representatives (the plan's 4-byte copy), or, wide, the u64 representatives */
    int wide;                  /* 33..64 sites: 8-byte states (ranks stay 32-bit) */
    double dsum;               /* sum of vz over all pairs */
    lsk_pair_row const *rows;  /* device [n_near + n_str + n_high], or NULL: the one-row-per-lane variant (far from half filling) */
    uint32_t const *sites;     /* device: the neighbour table above, or NULL: ... walking particles instead of pairs (weight x degree < pairs) */
    int n_sites, degree;       /* degree: slots per site, 4 or 8 */
    int n_classes, site_words; /* amplitude classes; 32-bit words of the whole table */
} lsk_pairplan;
/* staged push (k_push_t): LDS window of y per tile for near targets + the diagonal part; y cleared by the caller when n_diag > 0 */
int lsk_push_tile_rows(int cplx);
int lsk_push_staged(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, lsk_tilemap tm, int64_t n, uint64_t const *reps,
                    void const *x, void *y, int *d_err, void *stream);
int lsk_pairs_tile_rows(int cplx);
int lsk_pairs(lsk_pairplan pp, int hamming_weight, int cplx, lsk_tilemap tm, int64_t n, void const *x, void *y, void *stream);
/* ---- species-split row kernel (k_hubbard, k_rows.hip): pull over the spinful product basis, every off-diagonal term inside one
 * species half.  Row i = b * n_a + a (a: colex rank of the up word, b: of the down word); per species a neighbour table in
 * [slot][rank] layout -- partner rank (u32) and the matrix element <row|H|partner> (f64, or (re, im) pairs when cplx_coef) --
 * padded with zero amplitudes to `deg` slots; words[] are the species words by rank.  Diagonal terms come from op. */
typedef struct lsk_species {
    int64_t n;                  /* C(L, weight) */
    int deg;                    /* slots per word */
    uint32_t const *words;      /* device [n] */
    uint32_t const *rank;       /* device [deg][n] */
    double const *coef;         /* device [deg][n] (x2 when cplx_coef) */
} lsk_species;
typedef struct lsk_hubbard {
    int L, cplx_coef;
    lsk_species up, dn;
} lsk_hubbard;
int lsk_hubbard_apply(lsk_hubbard hb, lsk_operator op, int cplx, lsk_tilemap tm, void const *x, void *y, void *stream);
int lsk_narrow_states(int64_t n, uint64_t const *reps, uint32_t *out, void *stream);

/* fused_records != 0 (32-bit states and ranks): `reps` is out[] of lsk_chain_pack -- state | partner rank of the first
 * cached pair << 32 (cache == NULL: no cached pair) -- and `cache` only holds a second cached pair at cache + n */
int lsk_chain_pack(int64_t n, uint64_t const *reps, void const *cache, uint64_t *out, void *stream);
/* wave headers of the staged kernel (13..32 sites, 32-bit ranks): out[w] (8 bytes) describes rows 64 w .. 64 w + 63 when they
 * share every bit >= 12, else it is all ones and *d_n_plain (a zeroed device word) counts it.  high_site: the site >= 12 of the
 * cached pair, < 0 without one.  headed == 0 (any plan): all ones everywhere -- every wave-row on its records.  lsk_chain() expects the headers lsk_chain_words() 4-byte words past the start of wave_plan,
 * behind the word table: entry t = the t-th 12-bit word in (weight, value) order | in-class rank of word ^ low site << 16 |
 * the word's bit at the low site << 31. */
int lsk_chain_headers(lsk_basis bs, lsk_index ix, int64_t n, uint64_t const *reps, int headed, int high_site, void *out,
                      unsigned long long *d_n_plain, void *stream);
int lsk_chain_words(void);
/* partner ranks of a non-adjacent exchange pair for every row (u32, or u64 when wide_ranks); *d_flag is raised if a
 * partner leaves the basis */
int lsk_chain_cache(lsk_basis bs, lsk_index ix, int64_t n, uint64_t const *reps, uint64_t xmask, void *out, int wide_ranks,
                    int *d_flag, void *stream);
/* staged kernel (LDS term lists): rows [row0, row1) of partition `me`.
 * count_only != 0: adds the number of packets per destination to d_counts[P] and does nothing else.
 * otherwise: local packets -> index + atomic add into y; remote packets -> d_send according to
 * *d_layout using the per-destination cursors d_cursors[P] (must be zero on entry). */
int lsk_tile(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, int count_only, int P, int me,
             int64_t row0, int64_t row1, uint64_t const *reps, double const *norms, void const *x,
             void *y, unsigned long long *d_cursors, lsk_round_layout const *d_layout, void *d_send,
             unsigned long long *d_counts, int *d_err, void *stream);
/* the same producer with per-wave packet rings and a send layout fixed by the plan (P <= lsk_tile_wv_max_parts()):
 * count_only: d_wtab[wave][P] <- packets of every (wave of 64 rows counted from row0, destination); otherwise d_wtab holds
 * the exclusive offsets of every (wave, destination) inside the round's segments of *d_layout.  No cursors, no atomics on
 * the send side; the packet order does not depend on the block schedule. */
int lsk_tile_wv_max_parts(void);
/* gd.entries != NULL: pre-indexed packets -- every packet's local index at its destination comes out of the all-destinations
 * directory (own-partition packets included: ix is not used), and the send segments hold u32 indices instead of u64 states */
int lsk_tile_wv(lsk_operator op, lsk_basis bs, lsk_index ix, lsk_gdir gd, int cplx, int count_only, int P, int me,
                int64_t row0, int64_t row1, uint64_t const *reps, double const *norms, void const *x, void *y,
                uint32_t *d_wtab, lsk_round_layout const *d_layout, void *d_send, int *d_err, lsk_gtab own_gt, void *stream);
/* Packets in SORTED STREAMS (k_packets.hip, k_tile_st / k_window): unprojected fixed-weight bases, operators whose off-diagonal
 * groups are all exchange pairs.  stream = 2 * group + (bit of alpha at the pair's lower site); along a stream beta - alpha is a
 * constant, so the packets of one (destination, stream) -- written in row order -- carry ASCENDING destination indices, and the
 * consumer adds a window of y at a time in LDS instead of one fabric atomic per packet.
 * lsk_tile_st: rows [row0, row1) of one partition; tile t = rows [row0 + t tile_rows, ...), walked by one wave.  count_only:
 * d_ttab[tile][P * S] <- packets of every (tile, class = destination * S + stream); otherwise d_ttab holds the position of the
 * tile's first packet of every class inside the destination's segment of *d_layout (u32 keys, then values), and every packet --
 * the own partition's too -- goes to d_send as (u32 index at the destination, value). */
int lsk_tile_st_max_classes(void);
int lsk_tile_st(lsk_operator op, lsk_gdir gd, uint64_t const *d_binom, int cplx, int count_only, int P, int S, int tile_rows,
                int64_t row0, int64_t row1, uint64_t const *reps, void const *x, uint32_t *d_ttab,
                lsk_round_layout const *d_layout, void *d_send, int *d_err, void *stream);
/* one (source -> destination) segment as the consumer sees it */
typedef struct lsk_wsrc {
    uint32_t const *keys; /* device: indices at the destination, ascending inside every stream */
    double const *vals;   /* device: the values (re, im interleaved for c128) */
    uint32_t const *soff; /* device [S + 1]: stream s = packets [soff[s], soff[s + 1]) of the segment */
} lsk_wsrc;
/* the destinations of one consumer launch (passed by value): y[d] has count[d] rows and is served by the blocks
 * [first_block[d], first_block[d + 1]), wpb windows of lsk_window_rows(cplx) rows per block */
typedef struct lsk_wdests {
    int n;
    int64_t count[LSK_MAX_SEGS];
    int64_t first_block[LSK_MAX_SEGS + 1];
    void *y[LSK_MAX_SEGS];
    /* GLOBAL-RANK keys (round 6; dir[d] != NULL): a key is the colex rank of beta among ALL states of the weight, not its index at
     * the destination -- the producer needs no all-destinations directory (P / 4 bytes per global state on every rank), the
     * consumer turns a key into a row of y[d] with destination d's OWN rank directory (lsk_rankdir: 1 / 4 byte per global state,
     * whatever P) and finds its windows by the ranks of their first rows */
    lsk_rankdir const *dir[LSK_MAX_SEGS];
    uint64_t const *reps[LSK_MAX_SEGS]; /* the destination's ascending representatives (window bounds) */
    uint64_t const *binom;              /* device [64 * LSK_BINOM_K] */
    int64_t n_ranks;
    int weight;
    int *err;                           /* raised when a key is not a state of its destination (DMV:115-118) */
} lsk_wdests;
int lsk_window_rows(int cplx);
/* y[d][key] += value over all packets of the n_src source segments of every destination d (d_srcs: device [dests->n][n_src]) */
int lsk_window(int cplx, lsk_wdests const *dests, lsk_wsrc const *d_srcs, int n_src, int S, int wpb, void *stream);
/* replicated-x pull (Hermitian operators): rows of ONE partition against the whole vector in global
 * ascending order.  ix_global indexes the global basis; row_gidx[i] = global index of local row i
 * (may be NULL for lsk_direct_gx with closed-form indices, and for lsk_tile_pull when local == global). */
int lsk_direct_gx(lsk_operator op, lsk_basis bs, lsk_index ix_global, int cplx, lsk_tilemap tm,
                  uint64_t const *reps, int64_t const *row_gidx, void const *x_global, void *y, int *d_err,
                  void *stream);
/* hash table {rep -> x * norm(rep)} of the staged pull kernel: 2^bits entries of 16 (f64) / 32 (c128)
 * bytes; build once (keys + slot_of[i]), fill the values every matvec (norms NULL: unscaled) */
int lsk_hash_build(int cplx, int64_t n, uint64_t const *reps, int bits, void *tab, uint32_t *slot_of, void *stream);
int lsk_hash_fill(int cplx, int64_t n, uint32_t const *slot_of, void const *x, double const *norms, void *tab,
                  void *xs /* NULL, or the same scaled values in index order (near window of lsk_tile_pull) */, void *stream);
/* halo > 0: partners within `halo` (<= 512) entries of the tile in the sorted global representatives are resolved in an
 * LDS window and read from xs_global (= what the table holds, in index order); halo == 0: every partner through the table */
int lsk_tile_pull(lsk_operator op, lsk_basis bs, lsk_index ix_global, int cplx, int64_t row0, int64_t row1,
                  uint64_t const *reps, double const *norms_local, double const *norms_global,
                  int64_t const *row_gidx, void const *tab, int tab_bits, uint64_t const *reps_global,
                  int64_t n_global, void const *xs_global, int halo, void const *x_global, void *y,
                  int *d_err, void *stream);
/* Static index table {representative -> 32-bit payload} of the staged pull kernel's INDEXED mode (lsk_tile_pull_idx): built
 * once per basis, never refreshed.  Open addressing over 16-byte buckets of two 8-byte entries (one 16-byte request per
 * probe).  The key itself is not stored: h = an L-bit bijection of the state, bucket = its top `bbits` bits, and the entry
 * keeps the other L - bbits bits (tag), its displacement from the home bucket (8 bits) and the payload:
 *     entry = tag << 40 | displacement << 32 | payload,   empty = ~0
 * so 2^(bbits + 1) entries of 8 bytes serve n <= 2^bbits keys at load <= 0.5 (half the bytes of a {key, value} table, and
 * nothing to rewrite per matvec).  Needs tbits = L - bbits <= 24 and payloads < 2^32 - 1. */
/* choose bbits for n keys of L bits (returns -1 when no admissible size exists below max_bytes) */
int lsk_gtab_bits(int L, int64_t n, int64_t max_bytes);
/* fills entries (device, 16 << bbits bytes, allocated by the caller) with reps[i] -> payload[i] (payload NULL: i);
 * *d_flag is raised when a key cannot be placed within 255 buckets of its home */
int lsk_gtab_build(lsk_gtab t, uint64_t *entries, int64_t n, uint64_t const *reps, uint32_t const *payload, int *d_flag,
                   void *stream);
/* host-side mirror of the device lookup on a host copy of the entries (tests): payload or -1 */
int64_t lsk_test_gtab_find(lsk_gtab t, uint64_t const *h_entries, uint64_t key);
int lsk_test_gtab_build_host(lsk_gtab t, uint64_t *h_entries, int64_t n, uint64_t const *reps, uint32_t const *payload);
/* out[i] = lookup(keys[i]) or 0xffffffff (tests / plan-time checks) */
int lsk_gtab_lookup(lsk_gtab t, int64_t n, uint64_t const *keys, uint32_t *out, void *stream);

/* INDEXED mode of the staged pull kernel: the table yields a SLOT and the value is xsrc[slot] -- xsrc is x (times norm(rep) in
 * the K4 modes that prescale) in whatever order the caller holds it: index order on one device (perm == NULL, slot = global
 * index), or the received blocks of the replicated-x exchange as they arrive, owner-major (perm[g] = slot of global row g).
 * Rows are the contiguous global rows [row_g0 + row0, row_g0 + row1). */
typedef struct lsk_pullidx {
    lsk_gtab tab;
    uint32_t const *perm; /* device [n_global] or NULL */
    int64_t row_g0;
    uint64_t const *vtab; /* NULL, or the VALUE table of the same shape (k_pull.hip, lsk_vtab_*): 32-byte buckets {entry0, entry1, x[slot0],
                           * x[slot1]} -- one fabric request per far partner; f64 vectors of one partition, refreshed per matvec */
} lsk_pullidx;
/* value table: 32 << bbits bytes (allocated by the caller) copied from the index table `t`; refresh = x[slot] of every entry, in table order */
int lsk_vtab_build(lsk_gtab t, uint64_t *vtab, void *stream);
int lsk_vtab_refresh(lsk_gtab t, uint64_t *vtab, void const *xsrc, void *stream);
int lsk_tile_pull_idx(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                      double const *norms_local, lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global,
                      void const *xsrc, int halo, void *y, int *d_err, void *stream);
int lsk_pull_max_halo(void); /* largest near window (entries either side of a tile) the LDS hash set of the kernels takes */
/* The same matvec in TWO kernels, for the replicated-x exchange (dist.c): RESOLVE = stage A + K4 + slot look-ups, everything
 * that does not need x, writes one 4-byte slot per packet (+ its row inside the wave, + its coefficient unless the operator
 * has one real amplitude) to a per-wave packet stream; GATHER streams that, reads xsrc[slot] and writes y.  RESOLVE runs
 * while the blocks of x are on the wire.  Stream w belongs to rows [row0 + 64 w, row0 + 64 w + 64): `cap` packets of room
 * each (lsk_pullbuf_cap: 64 x number of flip-mask groups, the most 64 rows can generate), counts[w] of them valid. */
typedef struct lsk_pullbuf {
    uint32_t *slots;  /* device [streams * cap]; 0xffffffff = dead packet (zero-norm orbit) */
    uint8_t *rows;    /* device [streams * cap] */
    double *coefs;    /* device [streams * cap * lsk_pullbuf_coef_doubles] or NULL */
    uint32_t *counts; /* device [streams] */
    int64_t cap, row0;
    int64_t const *offs; /* NULL: stream w starts at w * cap; else device [streams + 1] exact offsets (lsk_tile_pull_stream_offsets) */
} lsk_pullbuf;
int lsk_tile_pull_stream_offsets(lsk_operator op, lsk_basis bs, int64_t row0, int64_t row1, uint64_t const *reps, int64_t *out,
                                 void *stream);
int64_t lsk_pullbuf_cap(lsk_operator op);
int lsk_pullbuf_coef_doubles(lsk_operator op, lsk_basis bs);
int lsk_tile_pull_resolve(lsk_operator op, lsk_basis bs, int64_t row0, int64_t row1, uint64_t const *reps,
                          double const *norms_local, lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global, int halo,
                          lsk_pullbuf buf, int *d_err, void *stream);
int lsk_tile_pull_gather(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                         double const *norms_local, lsk_pullidx ix, void const *xsrc, lsk_pullbuf buf, void *y, void *stream);
/* ---- block matvec (ls_amd_matvec_block): K columns per pass, one partition.  Element (i, k) of x is at x[i * xr + k * xc], y alike
 * (strides in elements of the vector type); y is assigned.
 * k_direct_blk: the pull form of k_direct on an unprojected basis (any operator), u64 states, tile map of <= 256-row tiles */
int lsk_direct_blk(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, lsk_tilemap tm, uint64_t const *reps, int K,
                   void const *x, int64_t xr, int64_t xc, void *y, int64_t yr, int64_t yc, int *d_err, void *stream);
/* k_pull_gather_blk: rows [row0, row1) of a projected one-partition plan from the packet streams lsk_tile_pull_resolve wrote into
 * buf (slot = global index); norms = the per-row norms (multiplied in for the K4 modes that prescale) */
int lsk_pull_gather_blk(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                        double const *norms, lsk_pullbuf buf, int K, void const *x, int64_t xr, int64_t xc, void *y,
                        int64_t yr, int64_t yc, void *stream);
/* ---- Chebyshev step (ls_amd_matvec_block_axpby; k_cheb.hip): Y <- alpha H X + beta X + gamma Y, K <= 64 columns, strides as above;
 * <X_k|X_k> is ADDED to d_dots[k] and Re <X_k|Y_k> (the new Y) to d_dots[K + k] (NULL: no dots); gamma == 0: Y is not read.
 * lsk_direct_cheb / lsk_pull_gather_cheb: the row loops of the two block kernels with that update where they store Y */
int lsk_direct_cheb(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, lsk_tilemap tm, uint64_t const *reps, int K,
                    void const *x, int64_t xr, int64_t xc, void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma,
                    double *d_dots, int *d_err, void *stream);
int lsk_pull_gather_cheb(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                         double const *norms, lsk_pullbuf buf, int K, void const *x, int64_t xr, int64_t xc, void *y,
                         int64_t yr, int64_t yc, double alpha, double beta, double gamma, double *d_dots, void *stream);
/* the epilogue pass alone: Y <- alpha W + beta X + gamma Y (n rows, K columns, own strides); the dots are ADDED to d_xx[k], d_xy[k] */
int lsk_axpby_dots(int cplx, int64_t n, int K, void const *w, int64_t wr, int64_t wc, void const *x, int64_t xr, int64_t xc,
                   void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma, double *d_xx, double *d_xy,
                   void *stream);
/* ---- Gram matrices of blocks (ls_amd_block_gram, ls_amd_matvec_block_axpby_gram; k_gram.hip):
 *     out[(ket Ka + a) Kb + b] = sum_r conj(A[r][a]) B_ket[r][b],  ket < nket (1 or 2; b2 is not read when nket == 1),
 * ASSIGNED, in elements of the vector type; strides in elements.  mfma != 0: k_block_gram_mfma, for which every block must have
 * column stride 1 (or one column) and a row stride equal to its width; else k_block_gram, any strides.  partial: the caller's
 * scratch of lsk_block_gram_blocks(n, Ka, Kb, cplx) x nket Ka Kb elements.  No floating-point atomics. */
int lsk_block_gram_blocks(int64_t n, int Ka, int Kb, int cplx);
char const *lsk_block_gram_kernel_name(int mfma);
int lsk_block_gram(int cplx, int64_t n, int Ka, void const *a, int64_t a_row, int64_t a_col, int Kb, int nket, void const *b1,
                   int64_t b1_row, int64_t b1_col, void const *b2, int64_t b2_row, int64_t b2_col, int mfma, double *partial,
                   double *out, void *stream);
/* ---- accumulate step of Chebyshev time evolution (ls_amd_matvec_block_axpby_acc; k_evolve.hip): the Chebyshev step above, and
 * Z[i, k] += (c_re + i c_im) Y[i, k] with the new Y where it is stored.  Z: K columns of its own strides (in ITS elements), c128 when
 * z_cplx != 0, else f64 (then c_im == 0 and f64 vectors).  The row kernels want a c128 Z 16-byte aligned. */
int lsk_direct_evolve(lsk_operator op, lsk_basis bs, lsk_index ix, int cplx, lsk_tilemap tm, uint64_t const *reps, int K,
                      void const *x, int64_t xr, int64_t xc, void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma,
                      void *z, int64_t zr, int64_t zc, int z_cplx, double c_re, double c_im, double *d_dots, int *d_err, void *stream);
int lsk_pull_gather_evolve(lsk_operator op, lsk_basis bs, int cplx, int64_t row0, int64_t row1, uint64_t const *reps,
                           double const *norms, lsk_pullbuf buf, int K, void const *x, int64_t xr, int64_t xc, void *y,
                           int64_t yr, int64_t yc, double alpha, double beta, double gamma, void *z, int64_t zr, int64_t zc, int z_cplx,
                           double c_re, double c_im, double *d_dots, void *stream);
/* the epilogue pass alone: Y <- alpha W + beta X + gamma Y, Z += c Y; the dots are ADDED to d_xx[k], d_xy[k] */
int lsk_axpby_acc(int cplx, int64_t n, int K, void const *w, int64_t wr, int64_t wc, void const *x, int64_t xr, int64_t xc,
                  void *y, int64_t yr, int64_t yc, double alpha, double beta, double gamma, void *z, int64_t zr, int64_t zc,
                  int z_cplx, double c_re, double c_im, double *d_xx, double *d_xy, void *stream);
/* out[i] = x[i] * norms[i] (f64 / c128): the owner-side prescaling of the indexed mode */
int lsk_scale(int cplx, int64_t n, void const *x, double const *norms, void *out, void *stream);
/* dst[perm[g] - base] = src[g] for every g with base <= perm[g] < base + count (8-byte elements): the rows one owner holds,
 * out of the global array, in its own (ascending) order */
int lsk_scatter_owned(int64_t n, uint32_t const *perm, int64_t base, int64_t count, uint64_t const *src, uint64_t *dst,
                      void *stream);

/* host-side check of the window search of the value-table kernel (tests, no device): position of `key` among the ascending
 * reps[0, n), n <= 1280, or -1 */
int lsk_test_window_find(uint64_t const *reps, int n, uint64_t key);
/* ... and of the LDS hash set of the indexed kernels (n <= 1024): position, or -1 when the window does not answer (absent,
 * or dropped from a full set -- such a partner goes through the static index table) */
int lsk_test_nw_find(uint64_t const *reps, int n, uint64_t key);
/* block -> tile of the pull kernels and of k_scatter (C consecutive tiles per XCD): host mirror for the tests */
int64_t lsk_test_pull_tile_of_block(int64_t b, int64_t n_tiles, int C);
int lsk_test_chain_near_table(int elem, int ldsp, int16_t *out);
uint64_t lsk_test_rep_trivial_dihedral(uint64_t a, int L, int inv, int reflect);
/* K4 mode 4: the row table of torus_min (out[2^tw], tw <= 8) and the minimum of v (and, with inv, of its complement) over the
 * translations of the tw x (L / tw) torus, starting from `best` (host mirrors of the device code) */
int lsk_torus_rowtab(int tw, uint32_t *out);
int lsk_torus_rowtab2(int tw, uint64_t *out); /* mode 5: rowtab[r] | rowtab[reversed r] << 32 */
uint64_t lsk_test_torus_min_d2(uint64_t v, int L, int tw, int inv, int present, uint64_t const *rowtab2, uint64_t best);
uint64_t lsk_test_torus_min(uint64_t v, int L, int tw, int inv, uint32_t const *rowtab, uint64_t best);
int lsk_bench_k4(int L, int inv, int reflect, int variant, int64_t n, uint64_t const *reps, uint64_t *out, void *stream);
/* n packets -> y[idx(beta)] += value */
int lsk_scatter(lsk_index ix, int cplx, int64_t n, uint64_t const *betas, void const *vals, void *y,
                double const *norms /* NULL, or per-row norms multiplied in (K4 modes 1, 2) */, int *d_err,
                void *stream);

/* projected fermionic bases (k_fermi.hip): the sign-aware K4 of enumeration, norms, state_info and the pull kernel ----- */
/* parity of sign(g, a) for element e with sign-table row tab[number_sites] (host mirror of the device code; table != 0 forces the
 * table form for ROT / REVROT elements as well) */
int lsk_test_fermi_parity(lsk_group_elem e, uint64_t const *tab, uint64_t a, int L, int table);
/* host mirror of the device code's application of a LSK_ELEM_LIFT element to a word of L = 2 h modes */
uint64_t lsk_test_fermi_apply_lift(lsk_group_elem e, uint64_t x, int L);
int lsk_fermi_enum_flags(lsk_basis bs, uint64_t const *d_binom, int64_t n_cand, int64_t n_threads, int chunk, uint64_t *flags,
                         int64_t *counts, void *stream);
int lsk_fermi_norms(lsk_basis bs, int64_t n, uint64_t const *reps, double *norms, void *stream);
int lsk_fermi_state_info(lsk_basis bs, int64_t n, uint64_t const *alphas, uint64_t *betas, double *characters, double *norms,
                         void *stream);
/* enumeration of a projected spinful (N_up, N_down) basis: the candidates are the product set in the order of lsk_enumerate_product,
 * kept by the signed test of lsk_fermi_enum_flags; bs.number_sites = 2 L */
int lsk_fermi_enumerate_product(lsk_basis bs, int n_up, int n_dn, uint64_t const *d_binom, uint64_t **d_states, int64_t *count, void *stream);
/* k_pull_t for bs.fermi: wide = 64-bit words, sink = 0 fused / 1 resolve (the value table is refused) */
int lsk_fermi_pull(lsk_operator op, lsk_basis bs, int wide, int cplx, int sink, int64_t row0, int64_t row1, uint64_t const *reps,
                   double const *norms_local, lsk_pullidx ix, uint64_t const *reps_global, int64_t n_global, void const *xsrc, int halo,
                   void *y, lsk_pullbuf buf, int *d_err, void *stream);

/* cross-sector operators (k_cross.hip): y[r'] = sum over the packets of the target rows r' = dst_reps[0, n_dst) -- the adjoint's
 * flip-mask groups (groups / terms: device arrays, the x = 0 group included) applied to r', projected into the SOURCE basis `src`
 * (always the general K4: orbit minimum, character, stabiliser norm), looked up there (gt.entries != NULL: the static index table
 * of the source's representatives; else `six`, whose dir_sites / dir_weight hold the source's bits and Hamming weight) -- of
 * conj(c) chi1(g0) n1(rep) / dst_norms[r'] x[index].  y is assigned.  *d_err is raised by a packet with non-zero source norm that
 * is not in the source basis.  A group whose summed coefficient on a row is at most `tiny` in both parts is no packet (rounding
 * residue of cancelling terms).  d_count != NULL: count the packets that reach a source row instead (x, y untouched). */
char const *lsk_cross_kernel_name(void);
int lsk_cross_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                   lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x, void *y,
                   double tiny, unsigned long long *d_count, int *d_err, void *stream);
/* the same for a projected fermionic source (k_cross_fermi.hip, k_cross_pull_fermi: the packets are projected with the signed
 * characters chi(g) sign(g, a) of lsk_fermi.hpp); lsk_cross_pull hands src.fermi here.  Always the static index table. */
char const *lsk_cross_fermi_kernel_name(void);
int lsk_cross_fermi_pull(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                         lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, void const *x, void *y,
                         double tiny, unsigned long long *d_count, int *d_err, void *stream);
/* the block form (k_cross_blk.hip, k_cross_pull_blk): y[r', k] for the K columns (1 <= K <= 64) of the blocks x
 * (source rows) and y (target rows), element strides (row, column) -- (K, 1) interleaved is the fast layout.  The other arguments
 * are those of lsk_cross_pull, the stages and the error flag too; y is assigned, one plain store per (row, column).  No counting
 * pass.  LS_AMD_CROSS_BLOCKS=<k>, read at every launch, caps the row blocks of the grid (a test hook).  lsk_cross_pull_blk hands
 * src.fermi to lsk_cross_fermi_pull_blk (k_cross_blk_fermi.hip, k_cross_pull_blk_fermi). */
char const *lsk_cross_blk_kernel_name(void);
int lsk_cross_pull_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                       lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, int K, void const *x,
                       int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny, int *d_err, void *stream);
char const *lsk_cross_blk_fermi_kernel_name(void);
int lsk_cross_fermi_pull_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                             lsk_gtab gt, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, int K, void const *x,
                             int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny, int *d_err, void *stream);
/* the projecting form (k_cross_project.hip, k_cross_project: DESIGN.md section 6b, groups = "project"): the sum over the elements of
 * the target group `dst` (chi2(g), the orbit sign of a projected fermionic target, the flipped images of a spin target with the
 * inversion) outside the stages of k_cross_pull, so that y = B2+ A B1 x for any operator and any two groups.  The other arguments
 * are those of lsk_cross_pull; f64 needs +-1 characters on dst as well.  lsk_cross_project hands a pair with a projected fermionic
 * basis on either side to lsk_cross_project_fermi (k_cross_project_fermi.hip, k_cross_project_fermi). */
char const *lsk_cross_project_kernel_name(void);
int lsk_cross_project(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                      lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                      void const *x, void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream);
char const *lsk_cross_project_fermi_kernel_name(void);
int lsk_cross_project_fermi(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                            lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                            void const *x, void *y, double tiny, unsigned long long *d_count, int *d_err, void *stream);
/* the block form of the projecting kernel (k_cross_project_blk.hip, k_cross_project_blk; DESIGN.md sections 6b, 6h): y[r', k] for the
 * K columns (1 <= K <= 64) of the blocks x and y, element strides (row, column) as for lsk_cross_pull_blk, whose chunks of 8 columns,
 * grid and LS_AMD_CROSS_BLOCKS cap it shares.  The stages of lsk_cross_project run once per chunk; a row's sums live in registers and
 * are stored once, one plain store per (row, column), in a fixed order of summation.  No counting pass; the error flag keeps its
 * meaning.  lsk_cross_project_blk hands a pair with a projected fermionic basis on either side to lsk_cross_project_blk_fermi
 * (k_cross_project_blk_fermi.hip, k_cross_project_blk_fermi). */
char const *lsk_cross_project_blk_kernel_name(void);
int lsk_cross_project_blk(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                          lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, int K,
                          void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny, int *d_err,
                          void *stream);
char const *lsk_cross_project_blk_fermi_kernel_name(void);
int lsk_cross_project_blk_fermi(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six,
                                lsk_gtab gt, lsk_basis dst, int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms,
                                int K, void const *x, int64_t x_row, int64_t x_col, void *y, int64_t y_row, int64_t y_col, double tiny,
                                int *d_err, void *stream);

/* the matrix of a cross-sector plan in CSR form (k_csr.hip).  lsk_cross_emit runs stages A, B1, B2 of
 * k_cross_pull (the arguments of lsk_cross_pull; either family) and, instead of gathering from x, hands every packet that reached a
 * source row out: off == NULL counts them per target row (cnt[i], i < n_dst); otherwise (off: n_dst + 1 entries, the exclusive scan
 * of the counts and their sum) packet k of row i -- k counts the row's packets in ascending group order -- is stored as
 * col[off[i] + k] = source index, val[off[i] + k] = its coefficient (1 or 2 doubles).  Plain stores, every slot written once; a
 * slot at or beyond off[n_dst] raises *d_err and is not stored. */
int lsk_cross_emit(int n_groups, lsk_group const *groups, lsk_term const *terms, int is_real, lsk_basis src, lsk_index six, lsk_gtab gt,
                   int cplx, int64_t n_dst, uint64_t const *dst_reps, double const *dst_norms, double tiny, int64_t const *off,
                   int64_t *cnt, int64_t *col, void *val, int *d_err, void *stream);
/* one wave per row over the raw entries [off[i], off[i + 1]): the first entry of every column receives the sum of the column's
 * entries, added in ascending position; every other entry, and a sum with |sum| <= 1e-12 sum |s|, is marked col = -2 - col.
 * cnt[i] = the entries left. */
int lsk_csr_merge(int cplx, int64_t n_rows, int64_t const *off, int64_t *col, void *val, int64_t *cnt, void *stream);
/* the entries lsk_csr_merge left, in ascending column order: entry of rank k of row i -> out[row_ptr[i] + k] */
int lsk_csr_write(int cplx, int64_t n_rows, int64_t const *off, int64_t const *col, void const *val, int64_t const *row_ptr,
                  int64_t *out_col, void *out_val, void *stream);

/* sector-state expansion (k_expand.hip): the vector psi on the representatives reps[0, n) of a spin basis, scattered over the orbits
 * of the representatives into the matrix M[a, b] = <a, b|psi> of a bipartition -- the image s = g r of row r
 * under group element g (and its flipped image under the spin inversion) receives conj(chi(g)) norms[r] psi[r], at
 *     fixed weight:  tab[n_A] + rank(a) * tab[LSK_EXPAND_MAX_NA + n_A] + rank(b),  n_A = popcount(a)   (one block per n_A)
 *     otherwise:     a * cols + b                                                                       (one block)
 * where a / b are the bits of s on the sites of mask_a / on the other sites, compacted in ascending site order.  Plain stores, no
 * atomics (equal targets receive equal values); `out` is cleared by the caller.  Images with n_A outside [na_lo, na_hi] are
 * skipped.  *d_err is raised by a row or an image that is not a state of the basis (wrong weight, bits above number_sites);
 * nothing is stored for it. */
#define LSK_EXPAND_MAX_NA 65 /* n_A = 0 .. 64 */
enum { LSK_SPLIT_LOW = 0 /* A = sites [0, n_a) */, LSK_SPLIT_HIGH = 1 /* A = sites [n_b, n_a + n_b) */, LSK_SPLIT_GATHER = 2 };
typedef struct lsk_expand {
    uint64_t mask_a;    /* the sites of A */
    int n_a, n_b;       /* |A|, |B| */
    int split;          /* LSK_SPLIT_* */
    int na_lo, na_hi;   /* fixed weight: the blocks to write */
    int64_t const *tab; /* fixed weight: device [2 * LSK_EXPAND_MAX_NA] -- first element of block n_A (-1: no such block), then its columns */
    int64_t cols;       /* no fixed weight: 2^n_b */
} lsk_expand;
char const *lsk_expand_kernel_name(void);
int lsk_expand_push(lsk_basis bs, lsk_expand ex, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps, double const *norms,
                    void const *psi, void *out, int *d_err, void *stream);

/* the same for fermionic bases (k_expand_fermi.hip, k_expand_push_fermi): the image s = g r receives
 *     sigma(s) conj(chi(g)) sign(g, r) norms[r] psi[r]
 * with sign(g, r) of lsk_fermi.hpp (projected bases; a basis without a group has the identity alone) and sigma(s) the sign of
 * carrying the modes of A in front of those of B (fermi_split_parity).  No spin inversion.  Block layouts:
 *     ALL:      no fixed particle number -- a * cols + b                                                       (one block)
 *     FIXED:    the table and the formula of lsk_expand                                                         (one block per n_A)
 *     PRODUCT:  the spinful (N_up, N_down) basis over 2 `half` modes, A = `au` up modes + `ad` down modes       (one block per (n_up, n_dn))
 *               a = a_dn << au | a_up, b = b_dn << (half - au) | b_up;  tab[n_up * (ad + 1) + n_dn] + row * cols + col,
 *               row = rank(a_dn) C(au, n_up) + rank(a_up),  col = rank(b_dn) C(half - au, N_up - n_up) + rank(b_up),
 *               cols = C(half - au, N_up - n_up) C(half - ad, N_dn - n_dn)
 * Images whose block key (n_A; n_up * (ad + 1) + n_dn) is outside [lo, hi] are skipped.  *d_err is raised by a row or an image that is
 * not a state of the basis (bits above the modes, another particle number in the word or in one of its halves); nothing is stored
 * for it. */
enum { LSK_EXPAND_FERMI_ALL = 0, LSK_EXPAND_FERMI_FIXED = 1, LSK_EXPAND_FERMI_PRODUCT = 2 };
#define LSK_EXPAND_FERMI_TAB (33 * 33) /* PRODUCT: n_up, n_dn = 0 .. 32 */
typedef struct lsk_expand_fermi {
    uint64_t mask_a, mask_b; /* the modes of A, and all the others */
    int n_a, n_b;            /* |A|, |B| */
    int split;               /* LSK_SPLIT_* */
    int kind;                /* LSK_EXPAND_FERMI_* */
    int lo, hi;              /* the block keys to write */
    int half, au, ad;        /* PRODUCT: L; the up / down modes of A */
    int n_up, n_dn;          /* PRODUCT: the particle numbers of the halves */
    int64_t const *tab;      /* FIXED: as lsk_expand.tab; PRODUCT: device [(au + 1) * (ad + 1)] first elements (-1: no such block) */
    int64_t cols;            /* ALL: 2^n_b */
} lsk_expand_fermi;
char const *lsk_expand_fermi_kernel_name(void);
int lsk_expand_fermi_push(lsk_basis bs, lsk_expand_fermi ex, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                          double const *norms, void const *psi, void *out, int *d_err, void *stream);
/* parity of sigma(n) (host run of the device code) */
int lsk_test_fermi_split_parity(uint64_t n, uint64_t mask_a, uint64_t mask_b);

/* projection into a sector (k_project.hip, k_project_fermi.hip on k_project_t.hpp): the adjoint of the two
 * expansions above with A = every site -- for the rows reps[0, n) and the K columns of phi,
 *     out[i, c] = (|G| norms[i])^-1 sum_g chi(g) [sign(g, r_i)] phi[index(g r_i), c]        (norms[i] > 0; otherwise 0)
 * summed over the permutation elements and, on a spin basis with the inversion, their flipped images with chi(g) inv.  index = the
 * position among the ascending states of the basis without symmetries: the word (ALL), its combinadic rank (FIXED), or
 * rank(high half) * n_low + rank(low half) (PRODUCT: the spinful (N_up, N_down) basis over 2 `half` modes) -- always < full.
 * phi[j, c] = phi[j * phi_s0 + c * phi_s1], out[i, c] = out[i * out_s0 + c * out_s1] in ELEMENTS of the dtype.  Plain stores, one
 * per (row, column); no atomics on the output.  *d_err is raised by a row or an image that is not a state of the basis; such an
 * image is never ranked or loaded, such a row reads 0. */
enum { LSK_PROJECT_ALL = 0, LSK_PROJECT_FIXED = 1, LSK_PROJECT_PRODUCT = 2 };
#define LSK_PROJECT_MAX_K 64 /* the library's MAX_COLUMNS */
#define LSK_PROJECT_COLS 8   /* columns per block of the K > 1 kernels */
typedef struct lsk_project {
    int kind;              /* LSK_PROJECT_* */
    int half, n_up, n_dn;  /* PRODUCT: L and the particle numbers of the halves */
    int64_t n_low;         /* PRODUCT: C(half, n_up) */
    int64_t full;          /* F: the states of the basis without symmetries */
    int K;                 /* columns, 1 .. LSK_PROJECT_MAX_K */
    int64_t phi_s0, phi_s1, out_s0, out_s1;
} lsk_project;
char const *lsk_project_kernel_name(void);
char const *lsk_project_fermi_kernel_name(void);
int lsk_project_pull(lsk_basis bs, lsk_project pj, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps, double const *norms,
                     void const *phi, void *out, int *d_err, void *stream);
int lsk_project_pull_fermi(lsk_basis bs, lsk_project pj, uint64_t const *d_binom, int cplx, int64_t n, uint64_t const *reps,
                           double const *norms, void const *phi, void *out, int *d_err, void *stream);

/* amplitudes of sector states on a batch of product states, and orbit images (k_amplitude.hip, k_amplitude_fermi.hip on
 * k_amplitude_t.hpp).  For the B words states[0, B), in any order, duplicates allowed, and the K columns of psi,
 *     out[j, c] = conj(character(s_j)) n(rep_j) psi[index(rep_j), c]        (state_info(s_j) = (rep_j, character, n); signed on
 *                                                                            projected fermionic bases; psi[index(s_j), c] unprojected)
 * and 0 for a word that is no state of the basis without symmetries (pj.kind and its numbers: the membership of lsk_project; pj.full is
 * not read) or lies on a zero-norm orbit.  index: gt (projected bases: the static index table of the array) or six (unprojected).
 * psi[i, c] = psi[i * pj.phi_s0 + c * pj.phi_s1], out[j, c] = out[j * pj.out_s0 + c * pj.out_s1] in ELEMENTS of the dtype, K = pj.K.
 * Plain stores; d_err[0] is raised by a representative inside the conserved numbers that is missing from the array (it reads 0).
 * _info: the same stages without psi -- rep, index (-1 where the amplitude reads 0), character (re, im: 2 B doubles) and n per state;
 * any output may be NULL.  lsk_orbit_image: out[j] = g_e reps[rows[j]], e = elements[j] over the effective group (spin inversion:
 * element 2 p = permutation p, 2 p + 1 = permutation p then ^ site_mask); d_err[1] is raised by a row or element out of range (out 0).
 * The _fermi forms take projected fermionic bases (bs.fermi), the plain ones every other basis. */
#define LSK_AMP_COLS 8 /* columns per chunk of k_amplitude_pull */
char const *lsk_amplitude_kernel_name(void);
char const *lsk_amplitude_fermi_kernel_name(void);
int lsk_amplitude_pull(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int cplx, int64_t B, uint64_t const *states,
                       void const *psi, void *out, int *d_err, void *stream);
int lsk_amplitude_pull_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int cplx, int64_t B, uint64_t const *states,
                             void const *psi, void *out, int *d_err, void *stream);
int lsk_amplitude_info(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int64_t B, uint64_t const *states, uint64_t *reps_out,
                       int64_t *index, double *characters, double *norms, int *d_err, void *stream);
int lsk_amplitude_info_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_project pj, int64_t B, uint64_t const *states,
                             uint64_t *reps_out, int64_t *index, double *characters, double *norms, int *d_err, void *stream);
int lsk_orbit_image(lsk_basis bs, int64_t n, uint64_t const *reps, int64_t B, int64_t const *rows, int32_t const *elements, uint64_t *out,
                    int *d_err, void *stream);
int lsk_orbit_image_fermi(lsk_basis bs, int64_t n, uint64_t const *reps, int64_t B, int64_t const *rows, int32_t const *elements,
                          uint64_t *out, int *d_err, void *stream);

/* two-point correlation matrices of a sector state (k_corr.hip, k_corr_fermi.hip): sums over the
 * representatives reps[0, n) alone -- the host averages them over the group afterwards.  A pair is the 16-bit word i | j << 8 of
 * two bits of the state word.  Both routines reduce in two steps without floating-point atomics: one partial per (block, pair) in
 * `partial`, then a sum over the blocks in ascending order into `out` (device; n_pairs values of 1 (f64) or, for the hoppings of a
 * c128 vector, 2 doubles); the grid is a function of n and of the kernel's residency on the device, so equal inputs give equal bytes.
 * `partial` holds lsk_corr_blocks(n) * n_pairs values (the most blocks either kernel launches). */
int lsk_corr_blocks(int64_t n);
/* densities: out[p] = sum_r |psi_r|^2 [bits i and j of reps[r] set]  (k_corr_diag; i == j: the one-point function) */
char const *lsk_corr_diag_kernel_name(void);
int lsk_corr_diag(int modes, int n_pairs, uint16_t const *pairs, int cplx, int64_t n, uint64_t const *reps, void const *psi,
                  double *partial, double *out, void *stream);
/* hoppings: out[p] = sum over the rows r with bit i set and bit j clear of
 *     conj(psi_r) / norms[r] * [jw: (-1)^popcount(r & between(i, j))] * chi(g0) [sign(g0, s)] n(rep s) psi[index(rep s)],  s = r ^ 1 << i ^ 1 << j,
 * the matrix element of k_cross_pull (stages B1 / B2; bs, six, gt as there: gt.entries != NULL looks the representative up in the
 * static index table, else `six` does) between the row and its image.  Images of zero norm contribute nothing; an image of
 * non-zero norm that is not among reps raises *d_err and contributes nothing.  bs.fermi runs k_corr_hop_fermi. */
char const *lsk_corr_hop_kernel_name(void);
char const *lsk_corr_hop_fermi_kernel_name(void);
int lsk_corr_hop(lsk_basis bs, lsk_index six, lsk_gtab gt, int jw, int n_pairs, uint16_t const *pairs, int cplx, int64_t n,
                 uint64_t const *reps, double const *norms, void const *psi, double *partial, double *out, int *d_err, void *stream);
int lsk_corr_hop_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, int jw, int n_pairs, uint16_t const *pairs, int cplx, int64_t n,
                       uint64_t const *reps, double const *norms, void const *psi, double *partial, double *out, int *d_err, void *stream);
/* out[q] = partial[q] + partial[m + q] + ... over `blocks` rows of m values, in that order */
int lsk_corr_sum(int blocks, int m, double const *partial, double *out, void *stream);

/* expectation values of arbitrary operators on a sector state (k_expect.hip, k_expect_fermi.hip): for every
 * unique device term u = (m, r, s) of a flip-mask group x -- row-wise orientation, coefficient 1 --
 *     out[u] = sum over the rows a with a & m == r of (-1)^popcount(a & s) conj(psi_a) / norms[a] * <a ^ x|psi>,
 * <.|psi> the matrix element of lsk_corr_hop (x == 0: |psi_a|^2, no look-up).  The image a ^ x of a row is projected and looked up
 * once per group; a row takes part in a group when a & cm == cr (the mask bits all terms of the group agree on) and the image keeps
 * the conserved numbers `cons`; an image that leaves them contributes exactly zero, an image of non-zero norm inside them that is
 * not among reps raises *d_err.  One call handles the groups [0, n_groups) of `groups`, whose terms (begin / end index `terms`) are
 * terms[term0, term0 + n_terms), n_terms <= LSK_EXPECT_CHUNK: `partial` holds lsk_corr_blocks(n) * n_terms values, `out` n_terms
 * (1 double for f64, 2 for c128).  No floating-point atomics: the reduction of lsk_corr_hop. */
#define LSK_EXPECT_CHUNK 4096
typedef struct lsk_expect_term { uint64_t m, r, s; } lsk_expect_term;
typedef struct lsk_expect_group {
    uint64_t x, cm, cr;
    int32_t begin, end;
} lsk_expect_group;
typedef struct lsk_expect_cons {
    int weight;           /* popcount of every state word, or -1 */
    int half, n_up, n_dn; /* half > 0: the (N, N_up) basis -- popcounts of the bits below / from `half` */
} lsk_expect_cons;
char const *lsk_expect_kernel_name(void);
char const *lsk_expect_fermi_kernel_name(void);
int lsk_expect(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
               lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps, double const *norms,
               void const *psi, double *partial, double *out, int *d_err, void *stream);
int lsk_expect_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                     lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps, double const *norms,
                     void const *psi, double *partial, double *out, int *d_err, void *stream);
/* the block form (k_expect_blk.hip, k_expect_blk_fermi.hip): lsk_expect for the K columns, 1 <= K <= 64, of
 * the (n, K) block psi with element strides (p_row, p_col) -- out[(u K + c)] (1 double for f64, 2 for c128) is out[u] above of
 * column c.  The packets, their projection and their look-up are shared by a chunk of 8 columns.  n_terms * K <= 8 LSK_EXPECT_CHUNK;
 * `partial` holds lsk_corr_blocks(n) * n_terms * K values, `out` n_terms * K.  No floating-point atomics. */
char const *lsk_expect_blk_kernel_name(void);
char const *lsk_expect_blk_fermi_kernel_name(void);
int lsk_expect_blk(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                   lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps, double const *norms,
                   int K, void const *psi, int64_t p_row, int64_t p_col, double *partial, double *out, int *d_err, void *stream);
int lsk_expect_blk_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                         lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                         double const *norms, int K, void const *psi, int64_t p_row, int64_t p_col, double *partial, double *out,
                         int *d_err, void *stream);
/* matrix elements between two blocks (k_expect_mat.hip, k_expect_mat_fermi.hip): lsk_expect_blk with a bra
 * block phi (n, Ka; strides a_row, a_col) and a ket block psi (n, Kb; strides k_row, k_col), 1 <= Ka, Kb <= 64 --
 *     out[(u Ka + a) Kb + b] = sum over the rows r with r & m == r_u of (-1)^popcount(r & s) conj(phi[r, a]) / norms[r] * <r ^ x|psi[:, b]>
 * (1 double for f64, 2 for c128).  The packets, their projection and their look-up are shared by a chunk of 8 bra x 8 ket columns.
 * n_terms * Ka * Kb <= 8 LSK_EXPECT_CHUNK; `partial` holds lsk_corr_blocks(n) * n_terms * Ka * Kb values, `out` n_terms * Ka * Kb.  Both
 * blocks are only read and may be the same memory.  No floating-point atomics. */
char const *lsk_expect_mat_kernel_name(void);
char const *lsk_expect_mat_fermi_kernel_name(void);
int lsk_expect_mat(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                   lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps, double const *norms,
                   int Ka, void const *phi, int64_t a_row, int64_t a_col, int Kb, void const *psi, int64_t k_row, int64_t k_col,
                   double *partial, double *out, int *d_err, void *stream);
int lsk_expect_mat_fermi(lsk_basis bs, lsk_index six, lsk_gtab gt, lsk_expect_cons cons, int n_groups, lsk_expect_group const *groups,
                         lsk_expect_term const *terms, int term0, int n_terms, int cplx, int64_t n, uint64_t const *reps,
                         double const *norms, int Ka, void const *phi, int64_t a_row, int64_t a_col, int Kb, void const *psi,
                         int64_t k_row, int64_t k_col, double *partial, double *out, int *d_err, void *stream);

/* plan-time helpers -------------------------------------------------------------------------- */
/* norms[i] = sqrt(stab(reps[i]) / |G|) */
int lsk_norms(lsk_basis bs, int64_t n, uint64_t const *reps, double *norms, void *stream);
/* *d_flag = 1 unless reps[i] == unrank(i) for all i (full fixed-Hamming prefix) */
int lsk_check_combinadic(lsk_index ix, int hamming_weight, int64_t n, uint64_t const *reps,
                         int *d_flag, void *stream);
/* SEARCH prefix table: table[b] = lower_bound(reps, b << shift), b in [0, nbuckets] */
int lsk_build_table(int64_t n, uint64_t const *reps, int shift, int64_t nbuckets, uint32_t *table,
                    void *stream);

/* batched externs (device pointers) ---------------------------------------------------------- */
int lsk_state_info(lsk_basis bs, int64_t n, uint64_t const *alphas, uint64_t *betas,
                   double *characters /* (re, im) */, double *norms, void *stream);
int lsk_state_index(lsk_index ix, int64_t n, uint64_t const *spins, int64_t *indices, void *stream);
/* counts[i] = number of non-zero off-diagonal groups of alphas[i] */
int lsk_offdiag_counts(lsk_operator op, int64_t n, uint64_t const *alphas, int64_t *counts,
                       void *stream);
/* writes (beta, c [* xs[i]]) of row i at offsets[i]...; xs may be NULL */
int lsk_offdiag_fill(lsk_operator op, int64_t n, uint64_t const *alphas, int64_t const *offsets,
                     uint64_t *betas, double *coeffs /* (re, im) */, double const *xs, void *stream);
/* ys[i] = d(alphas[i]) [* xs[i]] (real part) */
int lsk_diag_coeffs(lsk_operator op, int64_t n, uint64_t const *alphas, double *ys, double const *xs,
                    void *stream);
int lsk_exclusive_scan_i64(int64_t n, int64_t const *in, int64_t *out, void *stream);

/* enumeration + layout ------------------------------------------------------------------------ */
/* number of candidate states (fixed-Hamming rank space or 2^L), given the top-bit cut */
int lsk_enumerate(lsk_basis bs, uint64_t const *d_binom, int64_t n_candidates, uint64_t **d_states,
                  int64_t *count, void *stream);
/* the spinful product basis in ascending order: state = unrank(b, n_dn) << L | unrank(a, n_up), b outer, a inner */
int lsk_enumerate_product(int L, int n_up, int n_dn, uint64_t const *d_binom, uint64_t **d_states, int64_t *count, void *stream);
/* *d_flag = 1 unless reps[i] is the i-th state of the product basis of ix (PRODUCT index) for all i < n */
int lsk_check_product(lsk_index ix, int64_t n, uint64_t const *reps, int *d_flag, void *stream);
int lsk_masks(int64_t n, uint64_t const *states, int P, uint8_t *masks, void *stream);
int lsk_mask_counts(int64_t n, uint8_t const *masks, int P, int64_t *h_counts, void *stream);
int lsk_block_to_hashed(int64_t n, uint8_t const *masks, int P, int elt_size, void const *src,
                        void *const *h_dest, void *stream);
int lsk_hashed_to_block(int64_t n, uint8_t const *masks, int P, int elt_size,
                        void const *const *h_src, void *dest, void *stream);

/* out[i] = src[perm[i]], elements of 8 or 16 bytes, perm int32 or int64 */
int lsk_gather_perm(int64_t n, void const *perm, int perm_is_64, int elt_size, void const *src, void *out, void *stream);
/* repl.hip: the same over up to 64 index ranges [lo_k, hi_k) of perm / out in ONE launch (the rows of one chunk of y, grouped by
 * owner: one range per owner), and the event helpers of the chunked return / the adaptive split */
typedef struct lsk_ranges { int n; int64_t lo[64], hi[64]; } lsk_ranges;
int lsk_gather_perm_ranges(lsk_ranges const *ranges, void const *perm, int perm_is_64, int elt_size, void const *src, void *out, void *stream);
int lsk_event_query(void *ev);                      /* 0 complete, 1 not yet, -1 error */
int lsk_stream_wait_event(void *stream, void *ev);  /* work queued on `stream` after this call waits for `ev` */
char *lsk_error_buffer(size_t *capacity);           /* k_runtime.hip: the thread's error message buffer (lsk_last_error) */
/* bitmap bit (index of partner >> shift) <- 1 for every off-diagonal partner of the rows alphas[0, n) (u32 words, device): the
 * blocks of 2^shift rows of the global vector those rows read */
int lsk_reach_blocks(lsk_operator op, lsk_index ix_global, int64_t n, uint64_t const *alphas, int shift, uint32_t *bitmap, void *stream);

int lsk_iota_i64(int64_t n, int64_t base, int64_t *out, void *stream);
int lsk_narrow_i32(int64_t n, int64_t const *in, int32_t *out, void *stream);
int lsk_add_into(int cplx, int64_t n, void const *a, void *y, void *stream); /* y += a */

/* RCCL (comm.cpp) ------------------------------------------------------------------------------ */
typedef struct lsk_comm lsk_comm;
char const *lsk_comm_last_error(void);
int lsk_comm_available(void);
int lsk_comm_unique_id(void *id128);
int lsk_comm_create(lsk_comm **out, int size, int rank, void const *id128);
int lsk_comm_create_local(lsk_comm **out /* [size] */, int size); /* loop-back group: one process, one device, one thread per rank */
void lsk_comm_destroy(lsk_comm *c);
int lsk_comm_size(lsk_comm const *c);
int lsk_comm_rank(lsk_comm const *c);
int lsk_comm_rccl_count(lsk_comm const *c); /* ncclCommCount; 0 = loop-back group, -1 = error */
int lsk_comm_allreduce(lsk_comm *c, void *d_buf, int64_t count, int dtype /* 0 f64, 1 f32, 2 i64 */, int op /* 0 sum, 1 max */,
                       void *stream);
int lsk_comm_broadcast(lsk_comm *c, void *d_buf, int64_t bytes, int root, void *stream);
int lsk_comm_allgather(lsk_comm *c, void const *d_send, void *d_recv, int64_t bytes_per_rank, void *stream);
/* double-buffered all-to-all-v on the exchange stream (see comm.cpp) */
int lsk_comm_exchange_begin(lsk_comm *c, int slot, void *compute_stream);
int lsk_comm_alltoallv(lsk_comm *c, void const *d_send, int64_t const *send_off, int64_t const *send_bytes, void *d_recv,
                       int64_t const *recv_off, int64_t const *recv_bytes);
int lsk_comm_exchange_end(lsk_comm *c, int slot);
/* the same grouped send/recv on a stream of the caller's (no second stream, no events) */
/* K segments per peer in one grouped exchange: entry [k * size + p] = segment k for / from peer p */
int lsk_comm_alltoallv_multi_on(lsk_comm *c, void *stream, int K, void const *d_send, int64_t const *send_off,
                                int64_t const *send_bytes, void *d_recv, int64_t const *recv_off, int64_t const *recv_bytes);
int lsk_comm_alltoallv_on(lsk_comm *c, void *stream, void const *d_send, int64_t const *send_off, int64_t const *send_bytes,
                          void *d_recv, int64_t const *recv_off, int64_t const *recv_bytes);
int lsk_comm_exchange_wait(lsk_comm *c, int slot, void *compute_stream);
/* never hang (comm.cpp): what the next exchange is, for the watchdog's message; a deadline wait on `stream` + the exchange stream
 * (rc -1 with a message instead of a hung hipStreamSynchronize); the collective set-up cross-check of an exchange layout
 * ([K][size] byte counts: what s sends to d == what d expects from s, on every rank alike); test hook: stall the exchange stream */
int lsk_comm_exchange_ms(lsk_comm *c, int slot, float *ms); /* duration of the slot's last completed exchange; 1 = none yet; never blocks */
void lsk_comm_set_tag(lsk_comm *c, char const *what);
int lsk_comm_wait(lsk_comm *c, void *stream, double timeout_s);
int lsk_comm_check_counts(lsk_comm *c, int K, int64_t const *send_bytes, int64_t const *recv_bytes, char const *what, void *stream);
int lsk_comm_test_stall(lsk_comm *c, double seconds);

#ifdef __cplusplus
}
#endif
#endif /* LSK_H */
