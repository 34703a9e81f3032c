/* ls_amd.h -- device-level C ABI of the MI355X-native matvec: plain pointers and sizes only.
 *
 * This is the surface the reference's Chapel-level entry matrixVectorProduct(H, x, y,
 * representatives) (/root/reference/src/DistributedMatrixVector.chpl:1072-1093) maps onto:
 * x, y and representatives are hash-partitioned, per-partition ascending arrays
 * (partition of sigma = hash64_01(sigma) % P, /root/reference/src/StatesEnumeration.chpl:122-136)
 * that live in HBM.  Pointers named d_* are DEVICE pointers (hipMalloc / torch allocations);
 * `stream` is a hipStream_t passed as void* (NULL = the library's default stream).
 *
 * Two ways to run the off-diagonal exchange (DMV:856-1053 replaced):
 *   - all P partitions in this process on one device  -> ls_amd_matvec (logical partitions; the
 *     "exchange" is a pointer hand-off), and
 *   - one partition per process / GPU               -> ls_amd_dist_matvec (generate + RCCL all-to-all-v
 *     + scatter inside the library), or the three stages separately (ls_amd_generate, an exchange of
 *     the caller's, ls_amd_scatter).
 * All functions return 0 on success or a negative error code; ls_amd_last_error() explains.
 */
#ifndef LS_AMD_H
#define LS_AMD_H

#include "ls_hs.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { LS_AMD_F64 = 0, LS_AMD_C128 = 1 } ls_amd_dtype;

/* how y is produced when P == 1 and the operator is Hermitian */
typedef enum {
    LS_AMD_MODE_AUTO = 0, /* pull when the operator is Hermitian, else push (LS_AMD_MODE env: "push" | "pull") */
    LS_AMD_MODE_PUSH = 1, /* y[idx(beta)] += c x[i]   -- atomic scatter (ConcurrentAccessor) */
    LS_AMD_MODE_PULL = 2  /* y[i] = d x[i] + sum conj(c) x[idx(beta)]  -- gather, no atomics  */
} ls_amd_mode;

typedef struct ls_amd_plan ls_amd_plan;

/* error plumbing ------------------------------------------------------------------------- */
char const *ls_amd_last_error(void);
typedef void (*ls_amd_error_handler)(char const *message);
/* handler used by the halting ls_chpl_* / ls_hs_* entry points; NULL restores print+abort */
void ls_amd_set_error_handler(ls_amd_error_handler handler);

/* device helpers (thin wrappers so that a C / ctypes caller needs no HIP headers) ---------- */
int ls_amd_device_count(void);
int ls_amd_set_device(int device);
int ls_amd_malloc(void **d_ptr, size_t bytes);
int ls_amd_free(void *d_ptr);
int ls_amd_memcpy_h2d(void *d_dst, void const *h_src, size_t bytes);
int ls_amd_memcpy_d2h(void *h_dst, void const *d_src, size_t bytes);
int ls_amd_memcpy_d2d(void *d_dst, void const *d_src, size_t bytes, void *stream); /* async */
int ls_amd_memset(void *d_ptr, int value, size_t bytes, void *stream);
int ls_amd_synchronize(void *stream);

/* a plain streaming copy (16 bytes per lane): the device copy kernel the attainable HBM rate of the box is measured with
 * (SURVEY.md 8(d)); bytes is rounded down to a multiple of 16 */
int ls_amd_stream_copy(void *d_dst, void const *d_src, int64_t bytes, void *stream);
/* the read-only counterpart: every thread reads `per_thread` 16-byte elements and keeps an xor of them (d_sink: 4 bytes of device
 * memory, practically never written): the attainable READ rate of the box, the line the pull kernels' traffic (> 90 % reads)
 * is held against */
int ls_amd_stream_read(void const *d_src, int64_t bytes, int per_thread, void *d_sink, void *stream);

/* Eigensolver callers (Diagonalize.chpl:174-225 hands H to PRIMME; its Lanczos / Davidson steps orthogonalise one vector against
 * a block of basis vectors).  One sweep over the block V (m <= ls_amd_orth_max_rows() rows of n f64, row stride ldv) and w:
 *     if d_h_in:  w <- w - sum_k h_in[k] V[k];    out[k] = <V[k], w> (k < m, over the updated w);    out[m] = <w, w>
 * d_out: device [m + 1].  Pass 1 (h_in NULL) -> coefficients and norm; pass 2 (h_in = them) applies them and returns the remaining
 * overlaps in the same sweep, so classical Gram-Schmidt "twice" reads V two times instead of four when they are at rounding
 * level.
 * Requirements (not validated beyond the sizes): V and w are f64, each row of V and w contiguous, w does not alias any row of
 * V, d_out / d_h_in do not alias V or w.  Failures return -1 with a message in ls_amd_last_error(). */
int ls_amd_orth_max_rows(void);
int ls_amd_orth_pass(int m, int64_t n, double const *d_V, int64_t ldv, double *d_w, double const *d_h_in, double *d_out, void *stream);
/* thick restart of such a solver: V[:m_out] <- S^T V[:m_in] in place (d_S: m_in x m_out, row-major; m_out <= m_in <= max rows) */
int ls_amd_basis_rotate(int m_in, int m_out, int64_t n, double *d_V, int64_t ldv, double const *d_S, void *stream);
/* Block eigensolvers (block Lanczos: diagonalize.py lanczos_block_smallest; the reference's kMaxBlockSize, Diagonalize.chpl:172,192).
 * One sweep over the basis V (m rows of n f64, row stride ldv) and a block W (K rows, row stride ldw):
 *     if d_H_in (m x K, row-major):  W_c <- W_c - sum_k H_in[k][c] V_k
 *     d_out[k*K + c] = <V_k, W_c>  (k < m, over the updated W);    d_out[m*K + c*K + c'] = <W_c, W_c'>
 * d_out: device [m*K + K*K].  m = 0 returns the Gram matrix of W alone (d_V may then be NULL).  One launch reads V once and W once,
 * and writes W once when updating.  Limits: 0 <= m <= ls_amd_orth_block_max_rows() (128), 1 <= K <= 16, ldv >= n (m > 0),
 * ldw >= n.  Requirements (not validated): W shares no element with V, d_out / d_H_in alias neither.  Bad arguments return -1
 * with a message in ls_amd_last_error() and launch nothing. */
int ls_amd_orth_block_max_rows(void);
int ls_amd_orth_block_pass(int m, int K, int64_t n, double const *d_V, int64_t ldv, double *d_W, int64_t ldw, double const *d_H_in,
                           double *d_out, void *stream);
/* V[:m_out] <- S^T V[:m_in] in place (d_S: m_in x m_out, row-major, device; 1 <= m_out <= m_in <= ls_amd_orth_block_max_rows()):
 * the thick restart of a block solver and the normalisation W <- W R^-1 of its Cholesky-QR.  Reads m_in rows once and writes m_out
 * rows once, with no temporary in HBM. */
int ls_amd_block_rotate(int m_in, int m_out, int64_t n, double *d_V, int64_t ldv, double const *d_S, void *stream);

/* ------------------------------------------------------------------------------------------
 * The host-pointer boundary: ls_chpl_matrix_vector_product (DMV:1095-1110) and ls_chpl_primme_matvec (Diagonalize.chpl:134-162)
 * take `double *` as the reference's do.  What a call costs is decided by where that memory lives:
 *   LS_AMD_PTR_DEVICE    device memory (hipMalloc, a torch CUDA tensor): used in place, ZERO copies -- a GPU-resident
 *                        eigensolver can call the reference's entry points as they are
 *   LS_AMD_PTR_MANAGED   hipMallocManaged memory: fine-grained unless advised otherwise, and the push kernels' hardware f64 atomics
 *                        are specified for coarse-grained memory only -- never used in place: staged through the plan's own
 *                        hipMalloc vectors by one DMA per direction.  (The device-pointer entries -- ls_amd_matvec,
 *                        ls_amd_dist_matvec -- REFUSE a managed y for plans that accumulate with atomics.)
 *   LS_AMD_PTR_PINNED    hipHostMalloc'ed memory, or memory registered with ls_amd_host_register (once per workspace: PRIMME
 *                        reuses its vectors): one DMA per direction at the PCIe rate
 *   LS_AMD_PTR_PAGEABLE  anything else: double-buffered pinned bounce chunks filled by a small pool of host threads, upload
 *                        and download at the same time
 * The device copies of x / y persist with the cached plan (no hipMalloc / hipFree per call), y is uploaded only when the
 * operator has no diagonal terms (else it is assigned, DMV:1062-1063), and the columns of a PRIMME block share one pipeline
 * (column k + 1 goes up and column k - 1 comes down while column k computes).  Knobs: LS_AMD_STAGE=0 (plain synchronous
 * hipMemcpy), LS_AMD_STAGE_CHUNK_KB (32768), LS_AMD_STAGE_THREADS (min(16, cores / 4)). */
enum { LS_AMD_PTR_PAGEABLE = 0, LS_AMD_PTR_PINNED = 1, LS_AMD_PTR_DEVICE = 2, LS_AMD_PTR_MANAGED = 3 };
int ls_amd_pointer_kind(void const *p);
/* (Register long-lived, page-aligned workspaces.  On ROCm 7.x without XNACK, registering small malloc'ed heap blocks, unregistering
 * and freeing them, and letting the allocator reuse those addresses for pageable buffers of later hipMemcpy calls ended in GPU
 * memory faults of those later copies -- tests/test_gpu_matvec.py::test_host_pointer_boundary_memory_kinds, round 6.) */
int ls_amd_host_register(void *p, size_t bytes);   /* hipHostRegister: the caller keeps the memory alive until ... */
int ls_amd_host_unregister(void *p);               /* ... this */
struct ls_amd_boundary_stats {
    int64_t calls, columns;        /* entries into the boundary, vectors applied */
    int64_t bytes_h2d, bytes_d2h;  /* bytes that crossed PCIe */
    int64_t device_x, device_y;    /* columns whose x / y was device memory (used in place) */
};
void ls_amd_boundary_stats_get(struct ls_amd_boundary_stats *out, int reset);

/* hash64_01 / localeIdxOf on the host (StatesEnumeration.chpl:122-136) */
uint64_t ls_amd_hash64_01(uint64_t x);
int ls_amd_locale_idx_of(uint64_t basis_state, int num_locales);

/* ------------------------------------------------------------------------------------------
 * Objects built by somebody else (the real lattice-symmetries-haskell, /root/reference/src/FFI.chpl:94-119).
 * This library keeps everything it knows beyond the reference's struct prefix in a side table keyed by the object's
 * address, never in the struct: a foreign ls_hs_basis / ls_hs_operator only has to be registered once.
 *   ls_amd_adopt_basis     reads number_sites, number_up (Hamming weight or -1), spin_inversion, requires_projection and
 *                          `representatives` from the prefix; the symmetry generators are not part of the prefix and are
 *                          passed in the convention of ls_hs_create_spin_basis (0 generators for an unsymmetrised basis);
 *                          spinless-fermion prefixes (particle_type, number_sites, number_particles) take generators too, with
 *                          the permutation signs of ls_hs_create_spinless_fermion_basis; spinful prefixes with a fixed
 *                          number_up take SITE generators (ls_hs_create_spinful_fermion_basis), with number_up == -1 none
 *   ls_amd_adopt_spinful_fermion_basis  the same for a spinful prefix, with the up <-> down flip (spin_flip = 0, +1, -1),
 *                          which is not part of the prefix either
 *   ls_amd_adopt_operator  rebuilds the term / flip-mask-group tables from off_diag_terms / diag_terms
 *                          (ls_hs_nonbranching_terms with number_bits <= 64); its basis must be known
 *   ls_amd_release         forgets an adopted object and frees its tables (the foreign struct is left alone)
 * After that every entry point (ls_chpl_matrix_vector_product, plans, ls_chpl_primme_matvec, ...) accepts the foreign
 * pointers.  An unknown pointer halts with a message naming these functions.
 */
int ls_amd_adopt_basis(ls_hs_basis const *basis, int number_generators, int const *permutations, int const *sectors);
int ls_amd_adopt_spinful_fermion_basis(ls_hs_basis const *basis, int spin_flip, int number_generators, int const *permutations,
                                       int const *sectors);
int ls_amd_adopt_operator(ls_hs_operator const *op);
void ls_amd_release(void const *object);

/* ------------------------------------------------------------------------------------------
 * One locale per process / GPU: the inter-GPU exchange lives in the C host (RCCL over xGMI).
 *
 * Replaces /root/reference/src/DistributedMatrixVector.chpl:313-853 (GlobalPtrStore, _LocalBuffer /
 * _RemoteBuffer mailboxes with one-sided PUTs and remote flag stores, Producer / Consumer tasks,
 * three barriers per matvec) by bulk-synchronous rounds:
 *     generate(r)  ->  ONE grouped ncclSend / ncclRecv with the plan's exact per-round byte counts
 *                      (all-to-all-v of (sigma_j, c_j x_i) packets; every GPU pair uses its own xGMI link)
 *                  ->  scatter(r)
 * double-buffered over two HIP streams: the exchange of round r overlaps generate(r + 1) and scatter(r - 1).
 * librccl is loaded at run time (dlopen); the bootstrap of the 128-byte unique id is the caller's
 * (MPI_Bcast, a file, torch.distributed's store, ...), exactly like ncclGetUniqueId / ncclCommInitRank.
 * rank == locale index == hash64_01(sigma) % size (StatesEnumeration.chpl:133-136).
 */
typedef struct ls_amd_comm ls_amd_comm;
#define LS_AMD_UNIQUE_ID_BYTES 128
int ls_amd_comm_available(void);                 /* 1 when librccl can be loaded */
int ls_amd_comm_unique_id(void *id /* [LS_AMD_UNIQUE_ID_BYTES], written on the calling rank */);
int ls_amd_comm_create(ls_amd_comm **comm, int size, int rank, void const *id);
void ls_amd_comm_destroy(ls_amd_comm *comm);
/* Loop-back group (test infrastructure): `size` communicators inside this process on the current device, one per host
 * thread; every ls_amd_comm_* / ls_amd_dist_* / ls_amd_repl_* call works on them unchanged, the transport being
 * device-to-device copies behind a barrier.  The way to run more than one rank on a one-GPU box (RCCL refuses that). */
int ls_amd_comm_create_local(ls_amd_comm **comms /* [size] */, int size);
int ls_amd_comm_size(ls_amd_comm const *comm);
int ls_amd_comm_rank(ls_amd_comm const *comm);
/* the communicator size as RCCL itself reports it (ncclCommCount): what `bench.py --gpus N` prints as `rccl.comm_count` so that
 * a multi-GPU number carries evidence of the transport it ran on; 0 = loop-back group (test transport), -1 = error */
int ls_amd_comm_rccl_count(ls_amd_comm const *comm);
/* in-place collectives on device buffers (ordered on `stream`) */
int ls_amd_comm_allreduce_sum_f64(ls_amd_comm *comm, double *d_buf, int64_t count, void *stream);
int ls_amd_comm_allreduce_max_i64(ls_amd_comm *comm, int64_t *d_buf, int64_t count, void *stream);
int ls_amd_comm_broadcast(ls_amd_comm *comm, void *d_buf, int64_t bytes, int root, void *stream);
/* the communicator primmeGlobalSumReal / primmeBroadcastReal / ls_chpl_primme_matvec use when
 * primme->commInfo is NULL (the reference's PRIMME callbacks are collective over all locales,
 * /root/reference/src/PRIMME.chpl:267-373); NULL = single process */
void ls_amd_set_default_comm(ls_amd_comm *comm);
ls_amd_comm *ls_amd_default_comm(void);

/* matrixVectorProduct for this rank's block of the hashed vectors (DMV:1072-1093, one locale per process).
 * d_reps_local: this rank's representatives (ascending, device, borrowed for the lifetime of the object).
 * num_rounds <= 0: agreed on collectively (max local count / LS_AMD_ROWS_PER_ROUND, default 2^24 rows). */
typedef struct ls_amd_dist ls_amd_dist;
int ls_amd_dist_create(ls_amd_dist **dist, ls_amd_comm *comm, ls_hs_operator const *op, ls_amd_dtype dtype,
                       uint64_t const *d_reps_local, int64_t count_local, int num_rounds, void *stream);
void ls_amd_dist_destroy(ls_amd_dist *dist);
/* y <- H x (y is assigned by the diagonal pass, then accumulated into; untouched first when the operator has
 * no diagonal terms, DMV:1062-1063).  Collective: every rank of the communicator must call it. */
int ls_amd_dist_matvec(ls_amd_dist *dist, void const *d_x, void *d_y, void *stream);
ls_amd_plan *ls_amd_dist_plan(ls_amd_dist *dist);          /* timing, check, nnz, kernel name */
int64_t ls_amd_dist_exchange_bytes(ls_amd_dist const *dist); /* bytes this rank sends per matvec */
int ls_amd_dist_num_rounds(ls_amd_dist const *dist);

/* The cheaper exchange for Hermitian operators: replicate x instead of sending packets (N w bytes instead of
 * nnz (8 + w): ~30x fewer on the chains).  x, y and the representatives stay hash-partitioned at the interface; per matvec
 * every rank's block of x goes to every peer (one grouped send/recv), one permutation pass built from `masks` puts the
 * blocks into global ascending order (arrFromHashedToBlock, HashedToBlock.chpl:67-153), the pull kernels compute the
 * contiguous global rows [N r / P, N (r + 1) / P) with no atomics, and the results return to their owners with one
 * all-to-all-v (arrFromBlockToHashed restricted to the range).  Needs N w (+ the global representatives, and for projected
 * bases the hash table) of HBM per rank.
 * d_reps_global: the whole basis in ascending order; d_masks[i] = owner of state i (ls_amd_enumerate_states); both borrowed. */
typedef struct ls_amd_repl ls_amd_repl;
int ls_amd_repl_create(ls_amd_repl **repl, ls_amd_comm *comm, ls_hs_operator const *op, ls_amd_dtype dtype,
                       uint64_t const *d_reps_global, uint8_t const *d_masks, int64_t count_global, void *stream);
void ls_amd_repl_destroy(ls_amd_repl *repl);
/* y_local <- (H x)_local for this rank's blocks of the hashed vectors; collective */
int ls_amd_repl_matvec(ls_amd_repl *repl, void const *d_x_local, void *d_y_local, void *stream);
ls_amd_plan *ls_amd_repl_plan(ls_amd_repl *repl);
int64_t ls_amd_repl_exchange_bytes(ls_amd_repl const *repl);
/* bytes of x this rank receives per matvec.  Projected bases: every peer's block.  Unprojected bases: the contiguous rows of a
 * rank read only their own neighbourhood and the partner blocks of the top bonds, kept as <= 16 intervals of global rows; an
 * owner's elements are ascending in global rank, so each interval is one contiguous piece of every owner's block and is sent
 * as it lies (chain_32 at 8 ranks: 44 % of the vector; LS_AMD_REPL_REACH=0: the whole vector). */
int64_t ls_amd_repl_x_in_bytes(ls_amd_repl const *repl);
/* Fault injection (test hooks of the self-verification of `bench.py --gpus N`, tests/test_gpu_loopback.py): shift ONE segment
 * offset of the exchange layout by one element, memory-safely (the segment shrinks by the same element), so that the exchange
 * still completes but delivers misplaced data.  Return 1 when a segment was corrupted, 0 when the layout has none to corrupt
 * (e.g. a packet plan with a single rank: nothing leaves the GPU). */
int ls_amd_test_corrupt_dist(ls_amd_dist *dist);
/* test hook (thread-local): plans created afterwards consume their sorted packet streams with n windows of y per block (n > 1:
 * the run of a stream in one window starts where its run in the previous window ended); 0 = the plan decides */
void ls_amd_test_set_stream_windows_per_block(int n);
/* test hook (thread-local): the per-source stream buffers of ls_amd_matvec plans "do not fit" -- such a plan must come back with one
 * shared buffer and the atomic consumers instead of failing */
void ls_amd_test_fail_stream_buffers(int on);
/* ... and the set-up of the sorted streams fails on the calling rank of ls_amd_dist_create: ALL ranks must come back with the atomic
 * consumers and the default rows per round (the verdict of every set-up step is collective) */
void ls_amd_test_fail_dist_streams(int on);
int ls_amd_test_corrupt_repl(ls_amd_repl *repl);
/* Never hang (csrc/comm.cpp).  Every exchange layout is cross-checked between all ranks at set-up (what s sends to d == what d
 * expects from s; ls_amd_dist_create / ls_amd_repl_create fail on EVERY rank with the segment, the two ranks and both byte counts).
 * At run time a watchdog thread per RCCL communicator ends the process (exit code 86, message on stderr: rank, what was in
 * flight, for how long) when a collective or an exchange has not completed LS_AMD_COMM_WATCHDOG_S seconds (default 300, 0 = off)
 * after it was issued -- a dead peer or mismatched counts would otherwise leave every rank in a stream synchronisation for ever;
 * loop-back groups meet at a rendezvous with the same deadline.  ls_amd_comm_wait is the polite form: it waits until `stream` and
 * the communicator's exchange stream have drained, or returns -1 (message in ls_amd_last_error) after timeout_s (<= 0: the
 * watchdog's deadline). */
int ls_amd_comm_wait(ls_amd_comm *comm, void *stream, double timeout_s);
/* test hooks: rank `rank` sends delta_bytes more (less) to its right neighbour than that one expects -- late == 0: in the layout the
 * set-up check sees, late == 1: after it (a run-time fault); rank < 0 switches it off.  ls_amd_comm_test_stall: the exchange
 * stream of an RCCL communicator stalls for `seconds` behind an armed watchdog item. */
void ls_amd_test_skew_exchange(int rank, int64_t delta_bytes, int late);
int ls_amd_comm_test_stall(ls_amd_comm *comm, double seconds);
/* ... and the one-GPU counterpart (`bench.py --inject-fault` at N = 1): the row kernel of a plan whose partitions all live in this
 * process skips one row of the first tile (memory-safe); 1 when a tile was shortened, 0 when the plan has no tile map. */
int ls_amd_test_corrupt_plan(ls_amd_plan *plan);

/* ------------------------------------------------------------------------------------------
 * Plans.  A plan binds an operator to the partition layout and owns every per-basis device table:
 * term tables, symmetry-group networks, per-row norms, index prefix tables, per-round send counts.
 *
 *   num_partitions   P >= 1 (<= 256, DMV:664)
 *   my_partition     -1: all P partitions live in this process (counts[P], d_reps[P]);
 *                    p >= 0: this process owns only partition p (counts[0], d_reps[0] describe it)
 *   d_reps           device pointers to the ascending representatives of each owned partition;
 *                    borrowed -- must outlive the plan
 *   num_rounds       rows of a partition are processed in this many bulk-synchronous rounds
 *                    (0 = choose from LS_AMD_ROWS_PER_ROUND, default 2^24 rows)
 * ------------------------------------------------------------------------------------------ */
int ls_amd_plan_create(ls_amd_plan **plan, ls_hs_operator const *op, ls_amd_dtype dtype,
                       int num_partitions, int my_partition, uint64_t const *const *d_reps,
                       int64_t const *counts, int num_rounds, ls_amd_mode mode, void *stream);
void ls_amd_plan_destroy(ls_amd_plan *plan);

int ls_amd_plan_num_rounds(ls_amd_plan const *plan);
/* which kernel family the plan selected: "direct-push", "direct-pull", "tile", "tile-pull",
 * "replicated-direct-pull", "replicated-tile-pull" */
char const *ls_amd_plan_kernel_name(ls_amd_plan const *plan);
/* number of (beta, value) packets partition `my_partition` sends to every destination in `round`
 * (counts[P]; the own slot is 0 because local contributions are scattered in place) */
int ls_amd_plan_send_counts(ls_amd_plan const *plan, int round, int64_t *counts);
/* bytes of one packet segment entry: 8 (beta) + 8 or 16 (value) */
int ls_amd_plan_packet_bytes(ls_amd_plan const *plan);
/* bytes of per-row plan / basis data the dominant kernel streams next to x and y (8-byte fused record of the staged row
 * kernel, state words + cached partner ranks, state + norm for projected bases): compulsory traffic = rows (this + 2 w) */
int ls_amd_plan_row_bytes(ls_amd_plan const *plan);
/* total off-diagonal non-zeros generated per matvec by the owned partitions (from the count pass;
 * 0 when the plan runs a direct kernel and never counted) */
int64_t ls_amd_plan_nnz(ls_amd_plan const *plan);

/* Slot cache of the projected-basis pull path (opt-in; NOT matrix-free).  The indexed pull kernel spends ~80 % of a matvec
 * on work that does not depend on x: term expansion (BatchedOperator.chpl:163-213), the orbit minimum of every generated state
 * and the look-up of its representative (ls_hs_state_index, DMV:102) -- per non-zero one 4-byte slot + one row byte (+ the
 * coefficient unless every packet has the same real amplitude).  A plan that is applied many times (Diagonalize / PRIMME)
 * can keep those streams in HBM: the first matvec resolves them, every later one only gathers x[slot] and accumulates.
 * max_bytes = ceiling for the streams (<= 0: whatever the device can allocate).  Returns the number of rows whose streams
 * are kept -- every row, or the longest prefix of whole 256-row tiles that fits (the rows behind it keep the fused kernel);
 * 0 = nothing cached, the plan stays matrix-free (unprojected bases, value-table mode, no room). */
int64_t ls_amd_plan_cache_slots(ls_amd_plan *plan, int64_t max_bytes);
/* rows covered by the slot cache and the HBM it holds (0 / 0 when off) */
int ls_amd_plan_slot_cache_rows(ls_amd_plan const *plan, int64_t *rows, int64_t *bytes);

/* matrixVectorProduct(H, x, y, representatives), all partitions in this process
 * (DMV:1072-1093).  d_x[p], d_y[p]: device arrays of counts[p] elements of the plan's dtype.
 * Asynchronous on `stream`; call ls_amd_plan_check to synchronise and collect the
 * "invalid index" condition the reference halts on (DMV:115-118). */
int ls_amd_matvec(ls_amd_plan *plan, void const *const *d_x, void *const *d_y, void *stream);

/* Block matvec: Y[:, k] <- H X[:, k] for k < K (1 <= K <= 64).  Element (i, k) of X is at d_x[i*x_row + k*x_col] (elements of the
 * plan's dtype, not bytes); the same for Y.  (x_row, x_col) = (K, 1): interleaved (torch (N, K) contiguous), the fast layout;
 * (1, ld): column-major (PRIMME, orth_pass).  Strides are non-negative and nested -- row stride >= K * column stride, or column
 * stride >= N * row stride -- so that no two (i, k) share an element.  One-partition plans only (ls_amd_plan_create with P = 1,
 * my_partition = -1).  Y is assigned, not accumulated (DMV:1062-1063).  X and Y must not overlap.  Asynchronous on `stream`;
 * ls_amd_plan_check collects the "invalid index" condition as after ls_amd_matvec.  The plan's single-vector state (slot cache,
 * split form) is left as it is; a valid slot cache is read for the rows it covers.
 * LS_AMD_BLOCK=auto|kernel|columns (read at every call): `columns` runs ls_amd_matvec once per column (a strided column goes
 * through one column of scratch), `kernel` takes the block kernel wherever one applies, `auto` (default) the rule of
 * ls_amd_plan_block_kernel_name.  LS_AMD_BLOCK_RESOLVE_BYTES caps the packet buffer of the projected block path (default 1 GiB;
 * allocated on first use, freed with the plan). */
int ls_amd_matvec_block(ls_amd_plan *plan, int K, void const *d_x, int64_t x_row, int64_t x_col,
                        void *d_y, int64_t y_row, int64_t y_col, void *stream);
/* which path a block of K columns takes on this plan now: "k_direct_blk", "k_pull_gather_blk" or "columns" (NULL plan or K out of
 * range: NULL, with ls_amd_last_error set) */
char const *ls_amd_plan_block_kernel_name(ls_amd_plan const *plan, int K);

/* Chebyshev / Lanczos step on a block (the kernel polynomial method, distributed_matvec_amd.kpm):
 * Y[:,k] <- alpha * (H X)[:,k] + beta * X[:,k] + gamma * Y[:,k]   for k < K (1 <= K <= 64), strides as ls_amd_matvec_block.
 * d_dots: NULL, or 2K doubles on the device, ASSIGNED: [k] = <X_k|X_k>, [K + k] = Re <X_k|Y_k> with the new Y.
 * gamma == 0: Y is not read.  X and Y must not overlap.  One-partition plans only.  Asynchronous on `stream`;
 * ls_amd_plan_check as after ls_amd_matvec_block.
 * Where ls_amd_matvec_block would run k_direct_blk / k_pull_gather_blk, the same row loop runs with the update and the two sums in
 * place of its store (k_direct_cheb / k_pull_gather_cheb: Y is read and written once, nothing else is added to the matvec's
 * traffic); everywhere else each column goes through ls_amd_matvec into one column of scratch and one streaming pass finishes it
 * ("epilogue").  LS_AMD_BLOCK and LS_AMD_BLOCK_RESOLVE_BYTES apply as they do to ls_amd_matvec_block. */
int ls_amd_matvec_block_axpby(ls_amd_plan *plan, int K, void const *d_x, int64_t x_row, int64_t x_col,
                              void *d_y, int64_t y_row, int64_t y_col, double alpha, double beta, double gamma,
                              double *d_dots, void *stream);
/* "k_direct_cheb", "k_pull_gather_cheb" or "epilogue" (block matvec into scratch, then k_axpby_dots) */
char const *ls_amd_plan_axpby_kernel_name(ls_amd_plan const *plan, int K);
/* the epilogue alone, no plan: Y <- alpha W + beta X + gamma Y and the same two dots (W, X, Y: K columns of n rows, own strides;
 * cplx != 0: c128 elements, else f64).  W and Y, X and Y must not overlap. */
int ls_amd_block_axpby_dots(int cplx, int64_t n, int K, void const *d_w, int64_t w_row, int64_t w_col, void const *d_x, int64_t x_row,
                            int64_t x_col, void *d_y, int64_t y_row, int64_t y_col, double alpha, double beta, double gamma,
                            double *d_dots, void *stream);
/* The Gram matrix of two blocks of vectors, no plan (k_gram.hip):
 *     d_out[a * Kb + b] = sum_r conj(A[r, a]) * B[r, b],   a < Ka, b < Kb,
 * in elements of the vector type (cplx != 0: c128, else f64), ASSIGNED.  A: Ka columns of n rows, B: Kb columns of n rows, strides
 * in elements as everywhere; 1 <= Ka, Kb <= 64.  d_work: device scratch of at least ls_amd_block_gram_work_bytes(n, Ka, Kb, cplx)
 * bytes (that figure has room for the two ket blocks of ls_amd_matvec_block_axpby_gram; one suffices here and half of it is
 * accepted).  Blocks with column stride 1 and row stride K can go through the f64 MFMA (k_block_gram_mfma: the memory layout is the
 * operand layout); any other strides go through k_block_gram on the vector ALU.  LS_AMD_GRAM, read at every call: `mfma` takes the
 * MFMA form wherever it applies, `valu` never, `auto` (the default) where it applies and min(Ka, Kb) >= 8 -- below that the
 * vector-ALU form measured faster.
 * Rows are dealt to workgroups and waves by a fixed function of n, waves are summed in wave order and workgroups in block order:
 * no floating-point atomics, and two calls return equal bytes.  Refused before any launch: NULL pointers, Ka or Kb outside
 * [1, 64], n < 0, strides that make two elements share storage, too little work, an output or work buffer that overlaps A or B. */
int ls_amd_block_gram(int cplx, int64_t n, int Ka, void const *d_a, int64_t a_row, int64_t a_col, int Kb, void const *d_b,
                      int64_t b_row, int64_t b_col, void *d_work, int64_t work_bytes, void *d_out, void *stream);
int64_t ls_amd_block_gram_work_bytes(int64_t n, int Ka, int Kb, int cplx); /* -1: refused */
/* "k_block_gram_mfma" or "k_block_gram": the form a call with these widths and strides takes under the current LS_AMD_GRAM */
char const *ls_amd_block_gram_kernel_name(int cplx, int Ka, int64_t a_row, int64_t a_col, int Kb, int64_t b_row, int64_t b_col);
/* The Chebyshev step with matrix-valued dots: ls_amd_matvec_block_axpby with d_dots = NULL on whatever path it takes (Y is
 * bit-identical to that call's), then ONE Gram launch over X and the new Y,
 *     d_gram[a * K + b]         = sum_r conj(X[r, a]) * X[r, b],
 *     d_gram[K * K + a * K + b] = sum_r conj(X[r, a]) * Y[r, b],
 * 2 K K elements of the plan's type, assigned; X is read once by it.  The partials of the launch live in a buffer the plan
 * allocates on first use and frees with itself.  Refused before any launch: what ls_amd_matvec_block_axpby refuses (a NULL plan,
 * K outside [1, 64], a plan of more than one partition, NULL pointers, aliasing strides, X and Y that overlap), and a d_gram that
 * is NULL or overlaps X or Y. */
int ls_amd_matvec_block_axpby_gram(ls_amd_plan *plan, int K, void const *d_x, int64_t x_row, int64_t x_col,
                                   void *d_y, int64_t y_row, int64_t y_col, double alpha, double beta, double gamma,
                                   void *d_gram, void *stream);
/* The accumulate step of Chebyshev time evolution: ls_amd_matvec_block_axpby, and the running sum of the series where the new Y
 * is stored,
 *     Z[i,k] <- Z[i,k] + (c_re + i c_im) * Y[i,k]   (the new Y),
 * so that e^{-iHt} psi = sum_n c_n T_n(H~) psi costs one pass per order.  Z: K columns of n rows with strides of its own (in its
 * own elements), c128 when z_cplx != 0, else f64.  Element types (X / Y, Z): (f64, f64) with c_im == 0, (f64, c128), (c128, c128);
 * an f64 Z on a c128 plan is refused.  Z must not overlap X or Y; under LS_AMD_ACC=fused a c128 Z on a row-kernel path is 16-byte aligned.  Y, the dots, gamma == 0, the
 * paths and the environment exactly as ls_amd_matvec_block_axpby. */
int ls_amd_matvec_block_axpby_acc(ls_amd_plan *plan, int K, void const *d_x, int64_t x_row, int64_t x_col,
                                  void *d_y, int64_t y_row, int64_t y_col, double alpha, double beta, double gamma,
                                  void *d_z, int64_t z_row, int64_t z_col, int z_cplx, double c_re, double c_im,
                                  double *d_dots, void *stream);
/* "epilogue" (matvec into scratch, then k_axpby_acc); on the two row-kernel paths LS_AMD_ACC=fused gives "k_direct_evolve" /
 * "k_pull_gather_evolve" (Z accumulated inside the row kernel), LS_AMD_ACC=split "k_direct_cheb+k_axpby_acc" /
 * "k_pull_gather_cheb+k_axpby_acc" (the Chebyshev kernel, then one accumulate pass); unset: split, the faster one as measured */
char const *ls_amd_plan_acc_kernel_name(ls_amd_plan const *plan, int K);
/* the epilogue alone, no plan: Y <- alpha W + beta X + gamma Y, Z <- Z + c Y, and the two dots.  Z must not overlap W, X or Y. */
int ls_amd_block_axpby_acc(int cplx, int z_cplx, int64_t n, int K, void const *d_w, int64_t w_row, int64_t w_col, void const *d_x,
                           int64_t x_row, int64_t x_col, void *d_y, int64_t y_row, int64_t y_col, void *d_z, int64_t z_row,
                           int64_t z_col, double alpha, double beta, double gamma, double c_re, double c_im, double *d_dots,
                           void *stream);
/* A whole Chebyshev series on a block (polynomial filters: distributed_matvec_amd.kpm.chebyshev_series, the interior eigensolver):
 *     Z <- sum_{n = 0..N} c_n T_n((H - b) / a) X,    a = (hi - lo) / 2, b = (hi + lo) / 2,
 * one ls_amd_matvec_block_axpby_acc per order (alpha = 1/a, beta = -b/a, gamma = 0 first; then 2/a, -2b/a, -1) between two work
 * blocks that ping-pong.  X (any strides) is copied, not written; Z is ASSIGNED.  coeffs: N + 1 (re, im) pairs on the HOST.
 * d_work: two blocks of n x K elements of the plan's type on the device, or NULL: the plan allocates them (and keeps them until
 * it is destroyed or a larger K asks for more).  Element types (X, Z), the refusals, the paths and the environment are those of
 * ls_amd_matvec_block_axpby_acc; refused in addition: N < 0, coeffs == NULL, an imaginary part next to an f64 Z, bounds that are
 * not finite or not lo < hi, work that overlaps X or Z.
 * The dots of every order land in a device array that is read back every 64 orders -- the only synchronisations of `stream`, the
 * last one before the function returns -- for the guard <v_n|v_n> <= (1 + 1e-6) <v_0|v_0>: bounds that do not enclose the
 * spectrum return non-zero with a message that names lo, hi and the order (Z is then undefined).
 * A PRIMME matrixMatvec made of this call (the delta filter of kpm.delta_filter, negated) turns primme_smallest into the levels
 * nearest a target energy: INTEGRATION.md. */
int ls_amd_matvec_block_series(ls_amd_plan *plan, int K, int N, double const *coeffs, double lo, double hi,
                               void const *d_x, int64_t x_row, int64_t x_col, void *d_z, int64_t z_row, int64_t z_col, int z_cplx,
                               void *d_work, void *stream);
/* the row path of every order: what ls_amd_plan_axpby_kernel_name returns ("k_direct_cheb", "k_pull_gather_cheb", "epilogue") */
char const *ls_amd_plan_series_kernel_name(ls_amd_plan const *plan, int K);
int ls_amd_plan_check(ls_amd_plan *plan, void *stream);

/* ------------------------------------------------------------------------------------------
 * Replicated-x plans (Hermitian operators, one partition per process).  Instead of exchanging
 * (sigma_j, c_j x_i) packets, every rank holds the whole x in global ascending ("block") order --
 * the caller all-gathers it, nnz / N ~ 16 times fewer bytes than the packets -- and computes y for
 * its own rows by the pull formulation  y_r = d x_r + sum conj(c) x[idx_global(beta)].
 * d_reps_global: all representatives, ascending (borrowed, like d_reps_local).
 * ------------------------------------------------------------------------------------------ */
int ls_amd_plan_create_replicated(ls_amd_plan **plan, ls_hs_operator const *op, ls_amd_dtype dtype,
                                  int num_partitions, int my_partition, uint64_t const *d_reps_local,
                                  int64_t count_local, uint64_t const *d_reps_global,
                                  int64_t count_global, void *stream);
int ls_amd_matvec_replicated(ls_amd_plan *plan, void const *d_x_global, void *d_y_local, void *stream);

/* Kernel timing with HIP events recorded on the launch stream, around every launch of the plan's
 * dominant kernel (direct-push/direct-pull: the fused row kernel; tile: the staged kernel).
 * enable with max_samples > 0 (ring of that many event pairs; 0 disables); read back after
 * ls_amd_plan_check / a stream sync.  *count receives the number of samples written (<= capacity)
 * and the ring is reset. */
int ls_amd_plan_enable_timing(ls_amd_plan *plan, int max_samples);
/* Stage timers: the reference's --kDisplayTimings tree (DMV:1028-1052), HIP events around every stage launch on the
 * launch stream.  stages: 0 localDiagonal, 1 preparation of x (value-table refresh / x n(rep) / hashed -> block permutation),
 * 2 row kernel (fused paths), 3 producers (k_tile), 4 exchange (wait on the compute stream; replicated-x: the all-to-all of x),
 * 5 consumers (k_scatter), 6 replicated-x: y rows grouped by owner and returned.  max_events = capacity of the event pool
 * between two reads (0 disables). */
#define LS_AMD_NUM_STAGES 7
int ls_amd_plan_enable_stage_timing(ls_amd_plan *plan, int max_events);
int ls_amd_plan_stage_times(ls_amd_plan *plan, double *ms /* [LS_AMD_NUM_STAGES] totals */, int64_t *calls /* [LS_AMD_NUM_STAGES] */, int64_t *matvecs);
int ls_amd_plan_timing_report(ls_amd_plan *plan, char *buf, size_t capacity); /* the tree as text, per matvec */
int ls_amd_plan_kernel_times(ls_amd_plan *plan, float *ms, int capacity, int *count);

/* x[i] = u(hash(states[i], seed)) - 0.5 (re and im for c128): deterministic vectors keyed by the
 * basis state, identical for every partitioning (tests / bench input) */
int ls_amd_fill_random(int64_t n, uint64_t const *d_states, uint64_t seed, ls_amd_dtype dtype,
                       void *d_out, void *stream);

/* one-partition-per-process building blocks -------------------------------------------------
 * ls_amd_diag      y = d(sigma) x           (localDiagonal, DMV:59-71; no-op without diag terms)
 * ls_amd_generate  rows of `round` -> term expansion, projection, hash bucketing; packets for
 *                  remote owners are packed into d_send as P segments in destination order,
 *                  segment d = [beta x count_d][value x count_d] with count_d from
 *                  ls_amd_plan_send_counts; packets owned by this partition are indexed and
 *                  atomically added into d_y directly   (Producer.run, DMV:663-734)
 * ls_amd_scatter   n received packets (beta at d_betas, values at d_values) -> local index ->
 *                  atomic y[idx] += value                 (Consumer.run / localProcess, DMV:73-127)
 * ------------------------------------------------------------------------------------------ */
int ls_amd_diag(ls_amd_plan *plan, void const *d_x, void *d_y, void *stream);
int ls_amd_generate(ls_amd_plan *plan, int round, void const *d_x, void *d_y, void *d_send,
                    void *stream);
int ls_amd_scatter(ls_amd_plan *plan, int64_t n, uint64_t const *d_betas, void const *d_values,
                   void *d_y, void *stream);
/* Packet layout.  A segment of c packets is [key x c (padded to 8 bytes)][value x c]:
 *   ls_amd_plan_key_bytes == 8   the key is the state beta (u64) and the consumer ranks / searches it (every projected basis)
 *   ls_amd_plan_key_bytes == 4   PRE-INDEXED packets (hash partitions of unprojected fixed-weight bases): the key is the u32
 *                                index of beta inside the destination's block -- the producer reads it off an
 *                                all-destinations rank directory every rank derives alone (the owner of a state is a hash of
 *                                the state): 12 instead of 16 bytes per f64 packet on the wire and a search-free consumer, for
 *                                P / 4 bytes of HBM per basis state (ls_amd_plan_packet_index_bytes); taken while that fits
 *                                LS_AMD_PACKET_INDEX_MAX (default: a quarter of the free HBM), LS_AMD_PACKET_INDEX=0: never
 * ls_amd_plan_segment_bytes(c) = bytes of such a segment (what the all-to-all-v moves per (round, peer));
 * ls_amd_plan_segment_value_offset(c) = where its values start; ls_amd_plan_packet_bytes = key + value bytes (nominal).
 * ls_amd_scatter takes either kind (d_betas = the segment's key array).  ls_amd_scatter_round consumes ALL segments of a
 * round's receive buffer in one launch: segment s = counts[s] packets at d_recv + offsets[s].
 *
 * SORTED STREAMS (round 5; drivers that own both ends of the exchange: ls_amd_matvec over the partitions of one process and
 * ls_amd_dist_matvec with >= 2 ranks; csrc/k_packets.hip, k_tile_st / k_window).  When every off-diagonal term of the operator is
 * an exchange pair and the basis is an unprojected fixed-weight one, the pre-indexed packets of a segment are written as
 * 2 x (number of pairs) STREAMS, one per (pair, pattern of alpha on the pair): along a stream beta = alpha + constant, so --
 * the producer's rows and the destination's states both ascending -- the keys of a stream ASCEND.  The consumer then owns a
 * window of 2048 rows of y, finds every stream's sub-run for the window by binary search, adds those packets into an LDS copy of
 * the window and writes y once: no atomic, no fabric request per packet (chain_28 over 8 partitions 21.7 -> 10.8 ms, c128 42.8 ->
 * 14.7 ms; profiles/r5_packets_streams_ab.txt).  The own partition's packets take the same way (a segment of the send buffer).
 * Layout on the wire is unchanged (12-byte packets, keys then values); the stream starts of every segment are exchanged once at
 * set-up.  LS_AMD_PACKET_STREAMS=0: the atomic consumers above (A/B).  A plan driven through ls_amd_generate / ls_amd_scatter by a
 * foreign exchange never writes streams. */
int ls_amd_plan_key_bytes(ls_amd_plan const *plan);
int64_t ls_amd_plan_segment_bytes(ls_amd_plan const *plan, int64_t count);
int64_t ls_amd_plan_segment_value_offset(ls_amd_plan const *plan, int64_t count);
int64_t ls_amd_plan_packet_index_bytes(ls_amd_plan const *plan);
int ls_amd_scatter_round(ls_amd_plan *plan, int num_segments, int64_t const *counts, int64_t const *offsets,
                         void const *d_recv, void *d_y, void *stream);

/* ------------------------------------------------------------------------------------------
 * Basis construction on the device (enumerateStates, StatesEnumeration.chpl:516-585) and the
 * block <-> hashed layout converters (BlockToHashed.chpl:87-208, HashedToBlock.chpl:67-153).
 * ------------------------------------------------------------------------------------------ */
/* Enumerates all representatives in ascending order into a freshly allocated device array
 * (*d_states, ls_amd_free it) and, when d_masks != NULL, the owner hash64_01 % num_locales of each
 * state in the same (global ascending, "block") order. */
int ls_amd_enumerate_states(ls_hs_basis const *basis, int num_locales, uint64_t **d_states,
                            uint8_t **d_masks, int64_t *count, void *stream);
/* counts[p] = number of masks equal to p */
/* d_out[i] = d_src[d_perm[i]] (elements of 8 or 16 bytes; perm int32 or int64): the permutation pass of the replicated-x
 * exchange -- the received blocks (hashed order) into global ascending order, i.e. arrFromHashedToBlock
 * (HashedToBlock.chpl:67-153) with the permutation precomputed from `masks` */
int ls_amd_gather(int64_t n, void const *d_perm, int perm_is_64, int elt_size, void const *d_src, void *d_out, void *stream);
int ls_amd_mask_counts(int64_t n, uint8_t const *d_masks, int num_locales, int64_t *counts,
                       void *stream);
/* stable partition of a block-order array (elt_size 8 or 16 bytes) into P hashed parts */
int ls_amd_block_to_hashed(int64_t n, uint8_t const *d_masks, int num_locales, int elt_size,
                           void const *d_src, void *const *d_dest, void *stream);
/* inverse: k-way unmerge by masks */
int ls_amd_hashed_to_block(int64_t n, uint8_t const *d_masks, int num_locales, int elt_size,
                           void const *const *d_src, void *d_dest, void *stream);

/* cross-sector operators ------------------------------------------------------------------------------------------------------
 * An operator A that does not map a symmetry sector into itself -- S^z_q = sum_j e^{-iqj} sigma^z_j takes momentum k to k + q,
 * S^+_q changes the Hamming weight, c+ the particle numbers -- is applied BETWEEN two bases: x is indexed by the representatives
 * of the operator's own (source) basis, y by those of a target basis.  With the projector P = |G|^-1 sum_g conj(chi(g)) U_g, the
 * basis vectors |r> = P|r> / n(r), n(r)^2 = |G|^-1 sum_{g in Stab(r)} chi(g), and A|r> = sum_j c_j |b_j>,
 *     <r'|_2 A |r>_1 = sum_{j : rep(b_j) = r'} c_j conj(chi2(g0j)) n2(r') / n1(r),     g0j b_j = r'
 * provided A is COVARIANT: U_g A U_g^-1 = chi2(g) conj(chi1(g)) A for every generator g and for the spin inversion (then
 * P2 A = A P1).  The kernel (k_cross_pull, csrc/k_cross.hip) evaluates the pull form -- one target row per thread, the adjoint A+
 * applied to the target representative, every image projected into the source basis with the general orbit loop and looked up
 * there -- so y is assigned without atomics.  DESIGN.md section 6b.
 *
 * Scope: spin-1/2 bases, projected or not, on both sides, with the SAME generator permutations in the same order (any sectors,
 * any inversion characters, any Hamming weights); the unprojected fermionic bases of ls_hs_create_basis (spinless N -> N',
 * spinful (N, N_up) -> (N', N_up'); the Jordan-Wigner signs are in the terms' sign masks); and the PROJECTED fermionic bases
 * (spinless, spinful with spin_flip) with the same generators on both sides, up to 60 modes: their permutation signs enter the
 * projection of every image (k_cross_pull_fermi, csrc/k_cross_fermi.hip: the same kernel body with fermi_state_info_w) and the
 * covariance rule (ls_amd_operator_maps_sector_signed).  One partition.  Refused with their own messages: bases of different
 * number_sites, particle types or generators, spin inversion on one side only, projected fermionic bases above 60 modes. */
typedef struct ls_amd_cross ls_amd_cross;
/* A new operator on the same basis whose terms are the conjugate transpose: (v, m, r, x, s) becomes
 * (conj(v) (-1)^popcount(x & s), m, r ^ (x & m), x, s).  Host only (no device).  Release with ls_hs_destroy_operator.  NULL on
 * error. */
ls_hs_operator *ls_amd_operator_adjoint(ls_hs_operator const *op);
/* 0 when `op` (on its own basis, the source) maps the source sector into the sector of `target_basis`, i.e. when it is covariant
 * as above; -1 otherwise, with a message that names the offending generator ("generator g" in the order the bases were created
 * with, or "spin inversion").  Exact and host only: the term tables are written out on their full supports m | x | s (sigma^z as a
 * sign mask and as two projector terms are the same operator), transformed by every generator -- a permutation relabels the
 * sites of m, r, x, s as (g.w)[i] = w[g[i]]; the inversion sends r to r ^ m and multiplies v by (-1)^popcount(s) -- and compared
 * to 1e-12 max|v|.  No state is sampled.  Hamming weights and particle numbers are NOT examined (ls_amd_cross_check reports an
 * image outside the source basis at run time).  The refusals listed under Scope above come back as -1 with their own messages. */
int ls_amd_operator_maps_sector(ls_hs_operator const *op, ls_hs_basis const *target_basis);
/* The same question with PERMUTATION SIGNS: for bases without them (spins, unprojected fermions) exactly
 * ls_amd_operator_maps_sector; for projected fermionic bases (spinless, or spinful over their 2 L modes, where the lifted site
 * generators and the half swap of spin_flip are the generators) the covariance under U_g|a> = sign(g, a)|g.a>.  Both bases must
 * have the same particle type, number_sites and generator permutations in the same order; sectors, particle numbers and
 * number_up may differ; at most 64 modes.  Exact and host only, no state is sampled: a term (v, m, r, x, s) with x inside m is
 * conjugated inside the term format -- ((-1)^c v, g.m, g.r, g.x, g.(s ^ lin)), lin and c from the sign table of g (host.c) -- and
 * compared in a canonical form that absorbs the Jordan-Wigner string J(x) = XOR_{j in x} ((1 << j) - 1) of its flip mask, so that
 * c+_k over 64 modes costs one entry per site.  -1 with a message that names the generator as above, or "flips modes outside its
 * projector mask" (x not inside m), or "not a fermionic operator" (a sign mask that differs from J(x) on more than 12 modes
 * outside m).  ls_amd_cross_create runs this rule. */
int ls_amd_operator_maps_sector_signed(ls_hs_operator const *op, ls_hs_basis const *target_basis);
/* The plan of y = A x: `op_on_source` is A on the source basis, d_src_reps / d_dst_reps the ascending representatives of the
 * source / target basis in HBM (borrowed until ls_amd_cross_destroy).  Creation runs ls_amd_operator_maps_sector_signed, builds the
 * adjoint's device term groups (terms without a flip are a group like any other: row i of the target is not column i of the
 * source), the norms of the target rows, and the source look-up: the static index table of a projected source (shared with
 * matvec plans over the same array), the closed-form index of a complete unprojected one (identity, combinadic, product) or a
 * searched index.  LS_AMD_F64 needs a real operator and +-1 characters on both bases; anything else must be LS_AMD_C128. */
int ls_amd_cross_create(ls_amd_cross **out, ls_hs_operator const *op_on_source, ls_hs_basis const *target_basis, ls_amd_dtype dtype,
                        uint64_t const *d_src_reps, int64_t n_src, uint64_t const *d_dst_reps, int64_t n_dst, void *stream);
/* Bases with DIFFERENT symmetry groups.  ls_amd_cross_create refuses them; here they are opt-in by `mode`:
 *   LS_AMD_CROSS_SAME      exactly ls_amd_cross_create (its rule, its refusals, its kernel).
 *   LS_AMD_CROSS_RESTRICT  the target group G2 is a SUBGROUP of the source group G1 and A is covariant under G2: A psi then lies in
 *                          the target sector already and <r'|_2 A|psi> = (A psi^)(r') / n2(r'), which is what k_cross_pull evaluates
 *                          from the source's orbits and the target's norms -- host work only, the existing kernels, the CSR export
 *                          unchanged (its matrix is <r'|_2 A|r>_1).  Admitted by ls_amd_operator_maps_subgroup_sector.  A target
 *                          without symmetries is always a subgroup: the result is A B1 x on the plain basis.  With the same
 *                          generators on both sides the plan and its results are those of LS_AMD_CROSS_SAME, byte for byte.
 *   LS_AMD_CROSS_PROJECT   any two bases of one particle type and number_sites, ANY operator, no covariance check:
 *                              y[r'] = (|G2| n2(r'))^-1 sum_{g in G2} chi2(g) [sign(g, r')] (A B1 x)(g r')
 *                          (a spin target with the inversion adds the images g r' ^ mask with chi2(g) inv) -- the component of
 *                          A B1 x in the target sector, B2+ A B1 x, in the conventions and the normalisation of ls_amd_project; no
 *                          full-basis vector exists at any time.  With A = 1 this moves a state between the sectors of two groups.
 *                          The kernel is k_cross_project (k_cross_project_fermi when either basis is a projected fermionic one;
 *                          csrc/k_cross_project_t.hpp): the loop over the target's elements outside the stages of k_cross_pull, so
 *                          the cost is |G2| (2 |G2| with the inversion) times that of a restricted plan.  ls_amd_cross_nnz counts
 *                          the packets gathered per apply, over all elements; ls_amd_cross_csr refuses such a plan by name.
 * LS_AMD_F64 needs a real operator and +-1 characters on both bases in every mode.  One partition; projected fermionic sources up
 * to 60 modes.  Everything else is as for ls_amd_cross_create. */
enum { LS_AMD_CROSS_SAME = 0, LS_AMD_CROSS_RESTRICT = 1, LS_AMD_CROSS_PROJECT = 2 };
int ls_amd_cross_create_groups(ls_amd_cross **out, ls_hs_operator const *op_on_source, ls_hs_basis const *target_basis, ls_amd_dtype dtype,
                               int mode, uint64_t const *d_src_reps, int64_t n_src, uint64_t const *d_dst_reps, int64_t n_dst, void *stream);
/* The rule of LS_AMD_CROSS_RESTRICT, exact and host only.  0 when (1) both bases have one particle type and number_sites, (2) every
 * generator of the target is an ELEMENT of the source group -- looked up in the closure of the source's generators (for spinful
 * bases: of the lifted permutations), which also yields chi1(h) -- (3) a spin inversion / spin_flip of the target is one of the
 * source (the source may have one the target lacks), and (4) U_h A U_h^-1 = chi2(h) conj(chi1(h)) A for every generator h of the
 * TARGET and for its inversion: the plain rule of ls_amd_operator_maps_sector, or the signed rule of
 * ls_amd_operator_maps_sector_signed when either basis is a projected fermionic one.  -1 otherwise; the message names the target's
 * generator ("generator g") or the inversion, and points to LS_AMD_CROSS_PROJECT when the target group is no subgroup. */
int ls_amd_operator_maps_subgroup_sector(ls_hs_operator const *op, ls_hs_basis const *target_basis);
/* y <- A x (d_x: n_src, d_y: n_dst elements of the plan's dtype); y is ASSIGNED.  Asynchronous on `stream`. */
int ls_amd_cross_apply(ls_amd_cross *plan, void const *d_x, void *d_y, void *stream);
/* Y[:, k] <- A X[:, k] for the K columns of the blocks X (n_src rows) and Y (n_dst rows) of the plan's dtype, 1 <= K <= 64; Y is
 * ASSIGNED.  x_row / x_col, y_row / y_col: ELEMENT strides between rows and between columns, as in ls_amd_matvec_block -- any
 * non-negative pair that puts no two (row, column) on one element; interleaved (K, 1) is the fast layout (one image's columns are
 * consecutive memory), (1, n) the column-major one.  X and Y must not overlap.  Asynchronous on `stream`.  Plans of mode
 * LS_AMD_CROSS_SAME and LS_AMD_CROSS_RESTRICT run the block kernel (csrc/k_cross_blk.hip): the term sums, the
 * projection of every image and its look-up in the source basis are done once per chunk of 8 columns, not once per column.  Plans
 * of mode LS_AMD_CROSS_PROJECT have two paths.  The default, "columns", loops ls_amd_cross_apply over the columns, through
 * contiguous scratch columns that the plan owns where a row stride is not 1: byte for byte the K single applies.  "kernel" runs the
 * block form of k_cross_project (csrc/k_cross_project_blk.hip, k_cross_project_blk[_fermi]; DESIGN.md sections 6b, 6h): the
 * target's element loop, the term sums, the projection and the look-up once per chunk of 8 columns, every (row, column) summed in
 * registers in a fixed order (two calls return the same bytes; they differ from the column loop's in the last bits).
 * LS_AMD_CROSS_PROJECT_BLOCK=columns|kernel, read at every call, chooses (unset: columns; any other value is refused by name); it
 * has no effect on the other two modes.  A = 0 or an empty source clears Y.  The error flag is that of ls_amd_cross_apply: ls_amd_cross_check
 * serves both.  -1 with a message: K outside 1...64, NULL X or Y, strides that make elements share storage, overlapping X and Y.
 * Environment: LS_AMD_CROSS_BLOCKS=<k>, read at every launch, caps the row blocks of the block kernel's grid (a test hook: a
 * workgroup then walks several tiles). */
int ls_amd_cross_apply_block(ls_amd_cross *plan, int K, void const *d_x, int64_t x_row, int64_t x_col,
                             void *d_y, int64_t y_row, int64_t y_col, void *stream);
/* the path ls_amd_cross_apply_block takes for K columns: "k_cross_pull_blk", "k_cross_pull_blk_fermi" for a projected fermionic
 * source; for LS_AMD_CROSS_PROJECT "columns", or "k_cross_project_blk" / "k_cross_project_blk_fermi" (either basis a projected
 * fermionic one) under LS_AMD_CROSS_PROJECT_BLOCK=kernel.  NULL with a message: NULL plan, K outside 1...64. */
char const *ls_amd_cross_block_kernel_name(ls_amd_cross const *plan, int K);
/* The same two with the path of a LS_AMD_CROSS_PROJECT plan as an argument: _AUTO follows LS_AMD_CROSS_PROJECT_BLOCK (the two
 * functions above are these with _AUTO), _COLUMNS and _KERNEL choose whatever the environment says.  On LS_AMD_CROSS_SAME and
 * LS_AMD_CROSS_RESTRICT plans every path is the one block kernel.  An unknown path is refused by name; the path and K are checked
 * before the plan. */
enum { LS_AMD_CROSS_BLOCK_AUTO = 0, LS_AMD_CROSS_BLOCK_COLUMNS = 1, LS_AMD_CROSS_BLOCK_KERNEL = 2 };
int ls_amd_cross_apply_block_path(ls_amd_cross *plan, int path, int K, void const *d_x, int64_t x_row, int64_t x_col,
                                  void *d_y, int64_t y_row, int64_t y_col, void *stream);
char const *ls_amd_cross_block_kernel_name_path(ls_amd_cross const *plan, int path, int K);
/* synchronises `stream` and reports the device error flag: -1 ("... not in the source basis") when an image of A+ with non-zero
 * source norm was not found among the source's representatives -- A leaves the target's weight sector, say; y is then not A x.
 * The run-time counterpart of ls_amd_plan_check's "invalid index". */
int ls_amd_cross_check(ls_amd_cross *plan, void *stream);
char const *ls_amd_cross_kernel_name(ls_amd_cross const *plan); /* "k_cross_pull"; "k_cross_pull_fermi" for projected fermionic bases; "k_cross_project[_fermi]" for LS_AMD_CROSS_PROJECT */
/* the (target row, flip mask) pairs that contribute: a coefficient of A+ above the rounding residue of cancelling terms
 * (1e-13 sum |v|) whose image has non-zero norm in the source sector */
int64_t ls_amd_cross_nnz(ls_amd_cross const *plan);
void ls_amd_cross_destroy(ls_amd_cross *plan);

/* The matrix of a plan, M[i, j] = the number ls_amd_cross_apply multiplies x[j] by in row i (y = M x; rows: the target's
 * representatives, columns: the source's), as canonical CSR in library-owned device arrays:
 *     d_row_ptr  int64 [rows + 1]   d_row_ptr[0] = 0, d_row_ptr[rows] = nnz; row i holds the entries [d_row_ptr[i], d_row_ptr[i + 1])
 *     d_col      int64 [nnz]        strictly ascending inside every row, 0 <= col < cols
 *     d_val      dtype [nnz]        double, or (re, im) pairs of doubles
 * (d_col and d_val are allocated, never NULL, when nnz = 0).  The packets of a row that reach the same source state are summed in
 * ascending order of the adjoint's flip-mask groups, and a sum that cancels -- |sum s| <= 1e-12 sum |s| -- is no entry, so
 * nnz <= ls_amd_cross_nnz.  No atomics, no order of arrival: two exports of one plan are the same bytes.  Built in O(nnz) by the
 * plan's own kernel in an emitting mode and two per-row passes (csrc/k_csr.hip); synchronises `stream`. */
typedef struct ls_amd_csr {
    int64_t rows, cols, nnz;
    ls_amd_dtype dtype;
    int64_t *d_row_ptr, *d_col;
    void *d_val;
} ls_amd_csr;
/* upper bound of the peak device bytes of ls_amd_cross_csr -- the raw and the final entries, the row offsets -- from
 * ls_amd_cross_nnz, the number of target rows and the dtype; needs no device.  -1: NULL plan. */
int64_t ls_amd_cross_csr_bytes(ls_amd_cross const *plan);
/* Fills *out (cleared first).  -1 with a message that names both numbers, before anything is allocated, when
 * ls_amd_cross_csr_bytes exceeds max_bytes; -1 with the message of ls_amd_cross_check when an image of A+ with non-zero source norm
 * is not in the source basis (nothing is left allocated).  Release with ls_amd_csr_free. */
int ls_amd_cross_csr(ls_amd_cross *plan, int64_t max_bytes, ls_amd_csr *out, void *stream);
void ls_amd_csr_free(ls_amd_csr *m); /* frees the three arrays and clears *m; NULL and cleared structs are fine */

/* sector-state expansion and bipartitions -----------------------------------------------------------------------------------------
 * A state psi on the representatives of a symmetry sector (an eigenvector, say), expanded to its amplitudes on product states:
 * with the basis vectors |r~> = P|r> / |P|r>| of the projector above and state_info(s) = (rep, character, norm) of a full-basis state s,
 *     <s|psi> = conj(character(s)) norm(rep) psi[index(rep)]
 * evaluated in the push form (k_expand_push, csrc/k_expand.hip): the image s = g r of representative r under group element g --
 * a permutation, or a permutation times the global flip with character chi(g) inv -- receives conj(chi(g)) n(r) psi[r].  Plain
 * stores: elements that reach the same s write the same value.  States of zero-norm orbits read 0.  DESIGN.md section 6c.
 *
 * Layout.  The subsystem A is the set of sites in `subsystem_mask`, B the other sites; a = the bits of s on the sites of A compacted
 * in ascending site order, b likewise on B.  On a basis with fixed Hamming weight w the matrix M[a, b] = <a, b|psi> is block-diagonal
 * in n_A = popcount(a): block n_A has C(|A|, n_A) rows and C(|B|, w - n_A) columns, row-major, row = the combinadic rank of a, column
 * = that of b (ascending integer order on both sides).  Empty blocks are omitted; the blocks lie one after another in ONE buffer of
 * ls_amd_expand_total elements, ordered by n_A.  Without a fixed weight there is a single 2^|A| x 2^|B| block, row a, column b
 * (its n_A is reported as -1).  A = every site gives one block of one column: the vector over the ascending states of the same
 * basis without symmetries.  M M+ is the reduced density matrix of A.
 *
 * Scope: ONE partition (the whole sector on this device; up to 40 sites without a fixed weight).  ls_amd_expand_create takes
 * spin-1/2 bases, projected or not, and refuses with their own messages fermionic bases of any kind (the partial trace of fermions
 * needs mode-ordering signs: ls_amd_fermi_expand_create below carries them) and a mask with bits outside the sites. */
typedef struct ls_amd_expand ls_amd_expand;
/* d_reps: the n ascending representatives of `basis` in HBM (borrowed until ls_amd_expand_destroy).  Builds the norms n(r) -- by the
 * routine of the matvec and cross-sector plans -- and the block table; synchronises `stream`. */
int ls_amd_expand_create(ls_amd_expand **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, uint64_t subsystem_mask,
                         void *stream);
int ls_amd_expand_num_blocks(ls_amd_expand const *plan);
/* block i (ordered by n_A): its n_A, shape, and the offset of its first element in the buffer (in elements); NULL outputs are skipped */
int ls_amd_expand_block(ls_amd_expand const *plan, int i, int *n_a, int64_t *rows, int64_t *cols, int64_t *offset);
int64_t ls_amd_expand_total(ls_amd_expand const *plan); /* elements of the whole buffer */
/* d_out: the WHOLE buffer (ls_amd_expand_total elements of `dtype`); blocks [first_block, first_block + num_blocks) are cleared and
 * ASSIGNED, every other element is left as it is.  d_psi: n elements of `dtype`.  LS_AMD_F64 needs +-1 characters (the rule of
 * ls_amd_cross_create); anything else must be LS_AMD_C128.  Asynchronous on `stream`. */
int ls_amd_expand_apply(ls_amd_expand *plan, ls_amd_dtype dtype, void const *d_psi, void *d_out, int first_block, int num_blocks,
                        void *stream);
/* synchronises `stream` and reports the device error flag: -1 when a representative or one of its images was not a state of the
 * basis (another Hamming weight, bits above number_sites) -- such images are never stored */
int ls_amd_expand_check(ls_amd_expand *plan, void *stream);
char const *ls_amd_expand_kernel_name(ls_amd_expand const *plan); /* "k_expand_push"; "k_expand_push_fermi" for a fermionic plan */
void ls_amd_expand_destroy(ls_amd_expand *plan);
/* Host-only test hook (no device): the block table of `basis` and `subsystem_mask` -- up to `capacity` entries of every non-NULL
 * array, *total = the elements of the buffer; returns the number of blocks, -1 on the refusals above */
int ls_amd_test_expand_layout(ls_hs_basis const *basis, uint64_t subsystem_mask, int capacity, int *n_a, int64_t *rows, int64_t *cols,
                              int64_t *offsets, int64_t *total);


/* Fermionic bases (k_expand_push_fermi, csrc/k_expand_fermi.hip): spinless fermions, spinful fermions with N alone fixed (spinless
 * over their 2 L modes), and the spinful (N, N_up) product basis, each projected or not, with or without the up <-> down flip.  The
 * subsystem is a set of MODES (bits of the state word: mode (i, up) = bit i, mode (i, down) = bit i + L).  Two signs enter:
 *   the orbit sign -- U_g |r> = sign(g, r) |g r> (include/ls_hs.h), so the image s = g r receives conj(chi(g)) sign(g, r) n(r) psi[r];
 *     elements that reach the same s still store the same value (n(r) > 0 forces chi(g) sign(g, r) = 1 on the stabiliser);
 *   the bipartition sign -- with |n> = c+_{k1} ... c+_{kN} |0>, k1 < ... < kN, and |a>_A |b>_B := (prod_{k in A, ascending} c+_k)
 *     (prod_{k in B, ascending} c+_k) |0>, the modes of A in front:  |n> = sigma(n) |a>|b>,
 *         sigma(n) = (-1)^#{(i, j): i in A, j in B, both occupied, j < i},     M[a, b] = sigma(n) <n|psi>.
 *     M M+ is then the fermionic reduced density matrix: Tr(rho_A O_A) = <psi|O_A|psi> for every operator on A written by
 *     Jordan-Wigner over A's own modes (in ascending order).
 * Layout.  Spinless bases, and spinful ones with N alone fixed: the layout above over the modes -- one block per n_A at fixed N, one
 * 2^|A| x 2^|B| block otherwise (up to 40 modes).  The product basis: A = A_up (its modes below L) + A_dn; one block per
 * (n_up, n_dn) = the particles on A_up and A_dn, ordered lexicographically, empty blocks omitted, all in one buffer:
 *     rows C(|A_up|, n_up) C(|A_dn|, n_dn),   columns C(L - |A_up|, N_up - n_up) C(L - |A_dn|, N_dn - n_dn),
 * rows and columns in ascending integer order of the compacted words a and b (modes in ascending order, so the up modes are low):
 * rank_dn C(|A_up|, n_up) + rank_up on each side.  A = every mode gives the vector over the ascending states of the unprojected
 * basis.  An image that is not a state of the basis (a half with another particle number) raises the error flag and is dropped.
 * The handle works with ls_amd_expand_apply / _check / _num_blocks / _block / _total / _kernel_name / _destroy; on a product plan
 * ls_amd_expand_block reports n_a = n_up + n_dn.  LS_AMD_F64 needs +-1 characters.  Spin-1/2 bases are refused by name. */
int ls_amd_fermi_expand_create(ls_amd_expand **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, uint64_t mode_mask,
                               void *stream);
/* block i of a fermionic plan: (n_up, n_dn) on the product layout; n_up = n_A (-1 without a fixed number) and n_dn = -1 on the others */
int ls_amd_fermi_expand_block(ls_amd_expand const *plan, int i, int *n_up, int *n_dn, int64_t *rows, int64_t *cols, int64_t *offset);
/* Host-only test hooks (no device): the block table of a fermionic basis and `mode_mask`, as ls_amd_test_expand_layout, with the
 * refusals that need no device (spin bases, a mask outside the modes, a particle number beyond the binomial table, more than 40
 * modes without a fixed number); and sigma(state) = +-1 for the bipartition A = mode_mask_a of a word of `modes` modes, by the host
 * run of the device code (0 on bad arguments: modes outside [1, 64], bits of the mask or the state outside the modes) */
int ls_amd_test_fermi_expand_layout(ls_hs_basis const *basis, uint64_t mode_mask, int capacity, int *n_up, int *n_dn, int64_t *rows,
                                    int64_t *cols, int64_t *offsets, int64_t *total);
int ls_amd_test_fermi_split_parity(uint64_t mode_mask_a, int modes, uint64_t state);

/* ---- projection of full-basis vectors into a sector (csrc/k_project.hip, k_project_fermi.hip) ------------
 * The adjoint of the expansion above.  Let B be the matrix of the columns <s|r~> = conj(chi(g)) sign(g, r) n(r), s = g r (sign = 1
 * on spin bases), so that the full-basis vector of a sector state is B psi (A = every site: unproject).  For a vector Phi over the
 * ascending states of the same basis WITHOUT symmetries,
 *     psi[r] = <r~|Phi> = (B+ Phi)[r] = (|G| n(r))^-1 sum_{g in G} chi(g) sign(g, r) Phi[index(g r)]      (n(r) > 0; otherwise 0)
 * G includes the global spin inversion where the basis has one: every permutation element contributes its image t with chi(g) and
 * t ^ mask with chi(g) inv, and |G| counts both.  index = the position in the layout of the expansion with A = every site / mode:
 * the word itself without a fixed weight, the combinadic rank at fixed weight or particle number, rank_dn C(L, N_up) + rank_up on the
 * spinful (N, N_up) product basis.  B+ B = 1, so projecting an expanded state returns it; B B+ is the projector on the sector.
 * Pull form (k_project_pull; k_project_pull_fermi with the orbit sign): one representative per lane, the elements in a loop, the
 * image ranked once per (row, element) for up to 8 columns, ONE plain store per (row, column) -- no atomics on the output, no
 * floating-point atomics, and two calls return the same bytes.
 *
 * Scope: ONE partition (the whole sector and the whole full-basis vector on this device).  ONE create entry for both particle
 * families (it dispatches on the basis): spin-1/2 bases and every fermionic basis the expansion takes, projected or not, the
 * up <-> down flip included.  Refused by name: a NULL basis, more than 40 sites / modes without a fixed number, a weight beyond the
 * binomial table (33), LS_AMD_F64 with characters other than +-1, K outside [1, 64]. */
typedef struct ls_amd_project ls_amd_project;
/* d_reps: the n ascending representatives of `basis` in HBM (borrowed until ls_amd_project_destroy).  Builds the norms n(r) -- by the
 * routine of the expansion and the cross-sector plans; synchronises `stream`. */
int ls_amd_project_create(ls_amd_project **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream);
int64_t ls_amd_project_full_size(ls_amd_project const *plan); /* F: the states of the basis without symmetries */
/* d_phi: K columns over the F full-basis states, element (j, c) at d_phi[j * phi_s0 + c * phi_s1]; d_out: K columns over the n
 * representatives, element (i, c) at d_out[i * out_s0 + c * out_s1], every one ASSIGNED (rows of zero norm read 0) and nothing else
 * written.  Strides in elements of `dtype`, not negative; (K, 1) -- the columns interleaved -- is the fast layout of d_phi (one gather
 * fetches K neighbours).  1 <= K <= 64.  LS_AMD_F64 needs +-1 characters; anything else must be LS_AMD_C128.  Asynchronous on `stream`. */
int ls_amd_project_apply(ls_amd_project *plan, ls_amd_dtype dtype, int K, void const *d_phi, int64_t phi_s0, int64_t phi_s1,
                         void *d_out, int64_t out_s0, int64_t out_s1, void *stream);
/* synchronises `stream` and reports the device error flag: -1 when a representative or one of its images is not in the basis
 * (another Hamming weight or particle number, bits above the sites) -- such images are never ranked or loaded */
int ls_amd_project_check(ls_amd_project *plan, void *stream);
char const *ls_amd_project_kernel_name(ls_amd_project const *plan); /* "k_project_pull"; "k_project_pull_fermi" on a fermionic basis */
void ls_amd_project_destroy(ls_amd_project *plan);
/* Host-only test hook (no device): F of `basis`, or -1 with the message of the refusals above that need no device */
int64_t ls_amd_test_project_full_size(ls_hs_basis const *basis);
/* Host-only (no device): index(state), the position of `state` among the ascending states of the basis without symmetries, or -1 with
 * a message that names why the word is no state of the basis (bits above the sites / modes, another weight or particle numbers) */
int64_t ls_amd_test_project_state_index(ls_hs_basis const *basis, uint64_t state);

/* ---- amplitudes of sector states on product states, and orbit images (csrc/k_amplitude.hip, k_amplitude_fermi.hip) ----
 * The value of a sector state on a BATCH of product states, without the full-basis vector of the expansion: with state_info(s) =
 * (rep, character, norm) of a word s of the basis without symmetries,
 *     <s|psi> = conj(character(s)) norm(rep) psi[index(rep)]
 * (the character carries the orbit sign on a projected fermionic basis; psi[index(s)] on an unprojected basis).  The B words may come
 * in any order, with duplicates.  A word that is no state of the basis without symmetries -- a bit above the sites, another Hamming
 * weight or particle number, another (N_up, N_down) split -- and a word on an orbit of zero norm read 0 in every column: no error (the
 * rule of ls_amd_expect for images that leave the conserved numbers).  A representative inside the conserved numbers that is missing
 * from d_reps raises the plan's flag, which ls_amd_amp_check reports ("... not in the basis ...").  k_amplitude_pull (k_amplitude_pull_fermi
 * on projected fermionic bases): one state per lane; projection and look-up once per state whatever K; plain stores, so two calls
 * return the same bytes.  One partition.  The inverse direction, for Born sampling: Sum_{s in orbit(r)} |<s|psi>|^2 = |psi_r|^2 and a
 * uniform element of the effective group maps r uniformly onto its orbit, so drawing a row with probability |psi_r|^2 and an element
 * uniformly samples |<s|psi>|^2 exactly; ls_amd_amp_orbit_states applies the elements (k_orbit_image). */
typedef struct ls_amd_amp ls_amd_amp;
/* d_reps: the n ascending representatives of `basis` in HBM (borrowed until ls_amd_amp_destroy).  Builds the look-up of the array: the
 * static index table of a projected basis (shared with the matvec plans over the same array), a closed form or a searched index
 * otherwise.  Refuses by name: NULL arguments, a negative count, >= 2^32 - 1 rows, projected fermionic bases above 60 modes. */
int ls_amd_amp_create(ls_amd_amp **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream);
int ls_amd_amp_num_elements(ls_amd_amp const *plan); /* effective group order, inversion / flip included */
/* out[j, c] = <s_j|psi_c> for the B words d_states and the K columns of psi (n rows): psi[i, c] = psi[i * psi_row + c * psi_col],
 * out[j, c] = out[j * out_row + c * out_col] in ELEMENTS of the dtype, 1 <= K <= 64.  LS_AMD_F64 needs +-1 characters.  Refuses strides
 * that make two elements of out share storage, and an out that overlaps psi.  B = 0 is a no-op. */
int ls_amd_amp_amplitudes(ls_amd_amp *plan, ls_amd_dtype dtype, int K, int64_t B, uint64_t const *d_states, void const *d_psi,
                          int64_t psi_row, int64_t psi_col, void *d_out, int64_t out_row, int64_t out_col, void *stream);
/* the device-pointer form of ls_hs_state_info + ls_hs_state_index: representative, row (-1 for a word outside the basis, on a zero-norm
 * orbit, or whose representative is missing), character (re, im: 2 B doubles; with the orbit sign on projected fermionic bases, as in
 * ls_hs.h) and norm of every word.  A word outside the basis reports itself, character 0 and norm 0.  Any output may be NULL. */
int ls_amd_amp_state_info(ls_amd_amp *plan, int64_t B, uint64_t const *d_states, uint64_t *d_reps_out, int64_t *d_index,
                          double *d_characters /* 2B */, double *d_norms, void *stream);
/* out[j] = g_e reps[rows[j]], e = elements[j] in [0, ls_amd_amp_num_elements): on a spin basis with the global inversion element 2 p is
 * permutation p and 2 p + 1 is permutation p followed by the flip of every site; every other basis uses its own element list (the up <->
 * down flip of a spinful basis is among its elements).  A row or element out of range raises the flag (and stores 0). */
int ls_amd_amp_orbit_states(ls_amd_amp *plan, int64_t B, int64_t const *d_rows, int32_t const *d_elements, uint64_t *d_out, void *stream);
/* synchronises the stream; -1 with a message if a kernel since the last check raised the flag (then cleared) */
int ls_amd_amp_check(ls_amd_amp *plan, void *stream);
char const *ls_amd_amp_kernel_name(ls_amd_amp const *plan); /* "k_amplitude_pull" / "k_amplitude_pull_fermi" */
void ls_amd_amp_destroy(ls_amd_amp *plan);
/* host only, no device: the image of `state` under element `element` in the numbering of ls_amd_amp_orbit_states; *ok = 0 with a message
 * for an element out of range or a word with bits above the sites */
uint64_t ls_amd_test_orbit_state(ls_hs_basis const *basis, uint64_t state, int element, int *ok);

/* ---- two-point correlation matrices of a sector state (csrc/k_corr.hip, k_corr_fermi.hip) ---------------
 * For a NORMALISED state psi on the n representatives of `basis` (projected or not), over the M bits of a state word (the sites
 * of a spin or spinless basis; the 2 L modes of a spinful one, mode (i, up) = bit i, mode (i, down) = bit i + L):
 *   densities   d[i] = <b_i>,  D[i][j] = <b_i b_j>,  b_i = bit i of the product state (bit 1 = spin down / an occupied mode), so
 *               <sigma^z_i sigma^z_j> = 1 - 2 d_i - 2 d_j + 4 D_ij and <n_i n_j> = D_ij                          (k_corr_diag)
 *   hoppings    G[i][j] = <B+_i B_j>, B_j clears bit j and B+_i sets bit i: sigma^-_i sigma^+_j on a spin basis (sigma^+ clears a
 *               bit), c+_i c_j on a fermionic one -- there the kernel multiplies the Jordan-Wigner sign
 *               (-1)^popcount(state & between(i, j)) in, the mode order of the state word.  G[i][i] = d[i].   (k_corr_hop)
 * The operators are not invariant under the sector's group, the state is: the device sums over the representatives alone,
 *   R[i][j] = sum_r conj(psi_r) / n(r) (O_ij psi^)(r),   psi^(s) = conj(chi(s)) [sign] n(rep s) psi[index(rep s)]
 * (the conventions of ls_amd_cross / ls_amd_expand), and the host averages, C[i][j] = |G|^-1 sum_g R[g(i)][g(j)] -- |G| M^2
 * operations; an element with the global spin inversion acts as D -> 1 - d_i - d_j + D_ij, (i, j) -> (j, i) on the hoppings.
 * symmetrize = 0 returns R itself.  Neither kernel uses floating-point atomics: one partial sum per (block, pair), added in block
 * order, so two calls on the same input return the same bytes.  On the spinful (N, N_up) product basis only the pairs inside one
 * species are evaluated, the others are exactly zero.
 * Scope: ONE partition, one state.  ls_amd_corr_create refuses by name a NULL basis, a basis this library does not know
 * (ls_amd_adopt_basis), n <= 0 or NULL representatives, and projected fermionic bases above 60 modes (the limit of
 * ls_amd_cross_create).  It builds the norms by the routine the matvec, cross-sector and expansion plans use and shares the static
 * index table with the plans over the same array.  LS_AMD_F64 needs +-1 characters (the rule of ls_amd_cross_create). */
typedef struct ls_amd_corr ls_amd_corr;
int ls_amd_corr_create(ls_amd_corr **out, ls_hs_basis const *basis, uint64_t const *d_reps, int64_t n, void *stream);
int ls_amd_corr_modes(ls_amd_corr const *plan); /* M */
/* d_psi: n elements of `dtype` in HBM.  h_d: M doubles, h_dd: M * M doubles (row i, column j), HOST memory, either may be NULL.
 * Synchronises `stream`. */
int ls_amd_corr_densities(ls_amd_corr *plan, ls_amd_dtype dtype, void const *d_psi, double *h_d, double *h_dd, int symmetrize, void *stream);
/* h_g: M * M (re, im) pairs in HOST memory, row i column j = <B+_i B_j>, diagonal = the densities.  Synchronises `stream`; -1 with
 * a message when the image of a row has non-zero norm and is not among the representatives (the array is not the whole sector of
 * this basis) -- the error flag of ls_amd_cross_check; nothing is returned then. */
int ls_amd_corr_hoppings(ls_amd_corr *plan, ls_amd_dtype dtype, void const *d_psi, double *h_g, int symmetrize, void *stream);
/* which = 0: "k_corr_diag"; 1: "k_corr_hop", or "k_corr_hop_fermi" on a projected fermionic basis (signed characters) */
char const *ls_amd_corr_kernel_name(ls_amd_corr const *plan, int which);
void ls_amd_corr_destroy(ls_amd_corr *plan);
/* Host-only test hook (no device): the group average alone.  kind 0: raw / out = the one-point row d[M] followed by D[M][M];
 * kind 1: G[M][M] as (re, im) pairs. */
int ls_amd_test_corr_symmetrize(ls_hs_basis const *basis, int kind, double const *raw, double *out);

/* ------------------------------------------------------------------------------------------
 * Expectation values of arbitrary operators on a sector state (csrc/k_expect.hip, k_expect_fermi.hip): the
 * operators need not be invariant under the group of the sector and may act on any number of sites -- dimer-dimer correlations,
 * scalar chirality, pair correlations, four-point functions.  With R[A] = sum_r conj(psi_r) / n(r) (A psi^)(r) over the
 * representatives alone (psi^ as for ls_amd_corr; R is linear in A),
 *     <psi|O|psi> = |G|^-1 sum_{g in G} R[U_g O U_g^-1]
 * for every O and every sector.  The HOST conjugates every term (v, m, r, x, s) of every operator by every group element -- inside
 * the term format: a permutation relabels the masks, on projected fermionic bases with the permutation signs U_g|a> = sign(g, a)|g.a>
 * (the rule of ls_amd_operator_maps_sector_signed); an element with the global spin inversion sends a term to
 * ((-1)^popcount(s) v, m, r ^ m, x, s) -- brings the results to one canonical row-wise form (the orientation of
 * ls_amd_operator_adjoint; r inside m, the sign bits inside m folded into the coefficient) and keeps the UNIQUE terms of the whole
 * batch with a sparse combination value[k] = sum_u w[k][u] R[u].  The DEVICE computes R[u] of every unique term in one pass over the
 * representatives: the image r ^ x of a row is projected and looked up once per flip mask x and shared by all terms with that mask.
 * No floating-point atomics; two calls on the same input return the same bytes.  psi is taken as it is (no normalisation is assumed).
 * An image that leaves the conserved numbers of the basis (sigma^x on a fixed-weight basis, a lone c+) contributes exactly zero.
 * Scope: ONE partition; one state per call of ls_amd_expect_values, a block of up to 64 states per call of
 * ls_amd_expect_values_block (below).  ls_amd_expect_create refuses by name what ls_amd_corr_create refuses, n_ops <= 0, a NULL or
 * unknown operator, an operator of another basis and, on projected fermionic bases, a term that flips modes outside its projector
 * mask.  Only the term tables of the operators are read: they may be destroyed afterwards.  LS_AMD_F64 needs +-1 characters. */
typedef struct ls_amd_expect ls_amd_expect;
int ls_amd_expect_create(ls_amd_expect **out, ls_hs_basis const *basis, ls_hs_operator const *const *ops, int n_ops,
                         uint64_t const *d_reps, int64_t n, void *stream);
/* d_psi: n elements of `dtype` in HBM.  h_out: n_ops (re, im) pairs in HOST memory.  Synchronises `stream`; -1 with a message when
 * an image inside the conserved numbers has non-zero norm and is not among the representatives (not the whole sector). */
int ls_amd_expect_values(ls_amd_expect *plan, ls_amd_dtype dtype, void const *d_psi, double *h_out, void *stream);
int ls_amd_expect_num_terms(ls_amd_expect const *plan);  /* unique device terms of the batch */
int ls_amd_expect_num_groups(ls_amd_expect const *plan); /* flip-mask groups the device walks */
char const *ls_amd_expect_kernel_name(ls_amd_expect const *plan); /* "k_expect", or "k_expect_fermi" on a projected fermionic basis */
void ls_amd_expect_destroy(ls_amd_expect *plan);
/* Blocks of states (csrc/k_expect_blk.hip, k_expect_blk_fermi.hip): <psi_c|O_k|psi_c> of every operator of the
 * plan for the K columns of a block in ONE pass -- the packets of a flip mask, their projection and their look-up are shared by a
 * chunk of 8 columns; a resolved image gathers the chunk (interleaved columns: 64 / 128 consecutive bytes).  The same guarantees as
 * ls_amd_expect_values: no floating-point atomics, equal bytes from equal inputs, the same error.
 * d_psi: an (n, K) block of `dtype` in HBM with element strides (row, col), 1 <= K <= 64.  h_out: n_ops x K (re, im) pairs in HOST
 * memory, operator-major (h_out[2 (k K + c)]).  Synchronises `stream`.  Refused by name: K outside [1, 64], a NULL plan, block or
 * output, an unknown dtype, LS_AMD_F64 with complex characters, strides <= 0 and strides that make two elements share storage.
 * The first block call allocates the plan's block buffers (16 bytes per (block of rows, term, column) of a launch, at most
 * 8 * 4096 (term, column) pairs per launch: a batch with more splits its launches by terms and by columns).
 * LS_AMD_EXPECT_BLOCK=auto|kernel|columns, read at every call: `columns` loops ls_amd_expect_values over the columns (through a
 * contiguous scratch column of the plan where row != 1); `auto` is `kernel`. */
int ls_amd_expect_values_block(ls_amd_expect *plan, ls_amd_dtype dtype, int K, void const *d_psi, int64_t row_stride, int64_t col_stride,
                               double *h_out, void *stream);
char const *ls_amd_expect_block_kernel_name(ls_amd_expect const *plan, int K); /* "k_expect_blk", "k_expect_blk_fermi", or "columns" */
/* Matrix elements between two blocks of states of the sector (csrc/k_expect_mat.hip, k_expect_mat_fermi.hip):
 * <phi_a|O_k|psi_b> of every operator of the plan for every column a of a bra block and every column b of a ket block in ONE pass.
 * Two states of one sector transform with the same character, so the group average of O maps the sector into itself and
 *     <phi|O|psi> = |G|^-1 sum_{g in G} R[U_g O U_g^-1](phi, psi),    R[A](phi, psi) = sum_r conj(phi_r) / n(r) (A psi^)(r)
 * over the representatives alone: the sesquilinear form of R above, ANTILINEAR in the bra (its columns are conjugated) and linear in
 * the ket (the block the operator acts on).  The plan, its term tables and its combination are those of ls_amd_expect_create; the
 * packets of a flip mask, their projection and their look-up are shared by a chunk of 8 bra x 8 ket columns.  The same guarantees as
 * ls_amd_expect_values: no floating-point atomics, equal bytes from equal inputs, the same error.  The columns are taken as they are.
 * d_bra: an (n, Ka) block, d_ket: an (n, Kb) block, both of `dtype` in HBM, each with its own element strides (row, col),
 * 1 <= Ka, Kb <= 64; both are only read and may be the same memory or overlap.  h_out: n_ops x Ka x Kb (re, im) pairs in HOST memory,
 * operator-major, then bra, then ket (h_out[2 ((k Ka + a) Kb + b)] = Re <phi_a|O_k|psi_b>).  Synchronises `stream`.  Refused by name:
 * a NULL plan, block or output, Ka or Kb outside [1, 64], an unknown dtype, LS_AMD_F64 with complex characters, strides <= 0 and
 * strides that make two elements of one block share storage.
 * The first call allocates the plan's matrix buffers (16 bytes per (block of rows, term, bra, ket) of a launch, at most 8 * 4096
 * (term, bra, ket) triples per launch: a larger batch splits its launches by terms, then by ket columns, then by bra columns). */
int ls_amd_expect_matrix_elements(ls_amd_expect *plan, ls_amd_dtype dtype, int Ka, void const *d_bra, int64_t bra_row, int64_t bra_col,
                                  int Kb, void const *d_ket, int64_t ket_row, int64_t ket_col, double *h_out, void *stream);
char const *ls_amd_expect_matrix_kernel_name(ls_amd_expect const *plan, int Ka, int Kb); /* "k_expect_mat" or "k_expect_mat_fermi" */
/* Host-only test hook (no device): the merged terms of |G|^-1 sum_g U_g O U_g^-1 in the operator's OWN orientation
 * (A|a> = v [a & m == r] (-1)^popcount(a & s) |a ^ x>), r inside m and s outside m.  Returns their number, or -1; at most `cap` are
 * written to v (re, im pairs), m, r, x, s. */
int64_t ls_amd_test_expect_average(ls_hs_basis const *basis, ls_hs_operator const *op, int64_t cap, double *v, uint64_t *m, uint64_t *r,
                                   uint64_t *x, uint64_t *s);

/* test hooks: evaluate compiled host-side tables on the CPU (no device work) ------------------ */
int ls_amd_basis_group_order(ls_hs_basis const *basis);
/* 1 when the basis is a projected fermionic basis (spinless, or spinful with fixed number_up), i.e.
 * its group elements carry permutation signs (include/ls_hs.h) */
int ls_amd_basis_fermion_signs(ls_hs_basis const *basis);
/* test hook, no device: sign(g, state) = +-1 of group element `element` of such a basis, by the closed forms of rotations and
 * reflections or (table != 0) by the sign table for every element; 0 on bad arguments */
int ls_amd_test_fermion_sign(ls_hs_basis const *basis, int element, uint64_t state, int table);
/* the up <-> down flip character of a spinful-fermion basis (ls_hs_create_spinful_fermion_basis): 0 none, +1, -1 */
int ls_amd_basis_spin_flip(ls_hs_basis const *basis);
/* test hook: the compiled kind of a group element -- 0 network, 1 rotation, 2 reflection, 4 | 1 (reflection) | 2 (half swap) for the
 * ring elements of a spinful basis lifted to both species, -1 out of range */
int ls_amd_test_group_element_kind(ls_hs_basis const *basis, int element);
uint64_t ls_amd_basis_apply_group_element(ls_hs_basis const *basis, int element, uint64_t state);
int ls_amd_basis_group_character(ls_hs_basis const *basis, int element, double *re, double *im);

/* Host-only test hook (no device needed): the tile map of the row kernels (distributed-matvec_amd/csrc/lsk.h: lsk_tilemap)
 * for n rows in tiles of tile_rows, dealt to the 8 XCD lists contiguously (chunk == 0) or in round-robin chunks.
 * Returns the number of entries per list; *entries (malloc'ed, release with ls_amd_test_free) holds the 8 lists
 * (first row | rows << 48; 0 = empty slot); < 0 on error. */
int64_t ls_amd_test_tilemap(int64_t n, int tile_rows, int64_t chunk, uint64_t **entries);
/* Rows of y that the plan's paired launch computes (k_chain_pair_t: tiles of two 512-row segments that the top bond of a chain maps
 * onto each other); 0 for every plan that runs on k_chain_t alone (LS_AMD_CHAIN_PAIRED=0 forces that) or not on it at all. */
int64_t ls_amd_plan_chain_paired_rows(ls_amd_plan const *pl);
/* Host-only test hook: the two tile maps of the paired chain plan (k_chain_pair_t) of the weight-`weight` words of L sites -- `pairs`:
 * first row of every tile of two 512-row segments d rows apart, `rest`: the tiles of all other rows (bit 63 of an entry: that tile
 * runs on its records).  Returns 1 (out[0..5] = rows, first and one-past-last paired row of the first segments, d, slots per XCD of
 * rest and of pairs), 0 when the basis has no whole paired segment, < 0 on error; free both with ls_amd_test_free. */
int ls_amd_test_tilemap_paired(int L, int weight, int tile_rows, int64_t chunk, uint64_t **rest, uint64_t **pairs, int64_t *out);
/* Pairing levels.  The top site bits read as disjoint pairs (L-1, L-2), (L-3, L-4), ... are levels 1, 2, ...; a row is paired across
 * the bond L - 2 level of the first level, from the top, whose two bits differ (LS_AMD_CHAIN_PAIR_LEVELS=n stops at level n; 1 = the
 * top bond alone).  ls_amd_plan_chain_paired_rows_at: the rows paired at `level` (level 1: ls_amd_plan_chain_paired_rows);
 * ls_amd_plan_chain_pair_levels: the deepest level at which the plan pairs rows, 0 for an unpaired plan. */
int64_t ls_amd_plan_chain_paired_rows_at(ls_amd_plan const *pl, int level);
int ls_amd_plan_chain_pair_levels(ls_amd_plan const *pl);
/* Host-only test hook: the two tile maps of ls_amd_test_tilemap_paired for up to `levels` levels of a ring (every bond in a run), the
 * paired map dealt in chunks of pair_chunk, and the table of ranges.  Returns the number of ranges (0: no whole paired segment,
 * nothing is filled; < 0 on error).  out[0..3] = rows, slots per XCD of rest and of pairs, deepest level in use.  *ranges = six int64
 * per range in table order -- level, bond, first and one-past-last row of its first segments, d, first header of its second
 * segments -- and a tile of `pairs` holds its range's place in that table in bits 32..47.  Free all three with ls_amd_test_free. */
int ls_amd_test_tilemap_pair_levels(int L, int weight, int tile_rows, int64_t chunk, int64_t pair_chunk, int levels, uint64_t **rest,
                                    uint64_t **pairs, int64_t **ranges, int64_t *out);
void ls_amd_test_free(void *p);
/* Host-only test hook: the near-window search of the staged pull kernel for projected bases (k_tile_pull): position of
 * `key` among the ascending reps[0, n) (n <= 1280, stored as saturating 32-bit offsets from reps[0] exactly as a tile
 * stores them in LDS), -1 if it is not there or not representable (then the kernel takes the hash table), -2 on bad n */
int ls_amd_test_window_find(uint64_t const *reps, int n, uint64_t key);
/* ... and the near window of the INDEXED kernels (k_pull_t), a two-way hash set in LDS over the same offsets (n <= 1024): the
 * position of `key`, or -1 when the window does not answer -- the key is absent, or its set was already full when it was
 * staged (the kernel then takes the static index table, which holds every representative); never a wrong position */
int ls_amd_test_nw_find(uint64_t const *reps, int n, uint64_t key);
/* Host-only test hook: the near-pair table of the staged row kernel (distributed-matvec_amd/csrc/k_rows.hip: chain_lds_image) for
 * vectors of `elem` bytes per entry and `ldsp` pairs served from the LDS window: 480 entries of four int16 into `out`. */
int ls_amd_test_chain_near_table(int elem, int ldsp, int16_t *out);
/* Host-only test hook: the LDS windows of one tile of the staged row kernel, placed by the function the kernels call (k_rows.hip:
 * ChainWindow).  kind 0 = f64 tile, 1 = c128 tile, 2 = paired f64 tile; first = the tile's first row in x, first_b = that of a paired
 * tile's second segment.  out[0..1] = first row of the windows (may be < 0), out[2] = rows of one window, out[3] = windows, out[4] =
 * the tile's rows in one window, out[5] = halo, out[6] = pairs served from the window.  Returns 1 when the tile is interior -- the
 * prologue loads every window whole, without a bounds check --, 0 when it keeps the checked loads, -1 on an unknown kind. */
int ls_amd_test_chain_tile_windows(int kind, int64_t first, int64_t first_b, int64_t n_x, int64_t *out);
/* Host-only test hook: the word tables behind the wave headers of the staged row kernel (host.c: chain_wave_tables).  U[4096]: the
 * 12-bit words grouped by weight, ascending inside each weight, class k starting at class_off[k] (14 entries, the last 4096);
 * Rg[4096]: Rg[w] = rank of w ^ (1 << low_site) inside its own weight class (low_site < 12; < 0: all zero). */
int ls_amd_test_chain_wave_tables(int low_site, uint16_t *U, uint16_t *Rg, int *class_off);
/* Host-only test hook: the orbit minimum of `a` under the translations of a ring of L sites (and its reflections / the global
 * spin flip when asked), computed by the candidate-pruning routine the projected-basis kernels use (K4, trivial sector). */
uint64_t ls_amd_test_rep_trivial_dihedral(uint64_t a, int L, int inv, int reflect);
/* Profiling entry: K4 alone over the packets of a ring (every state of d_reps with each adjacent pair flipped), see scripts/k4_rate.py */
int ls_amd_bench_k4(int L, int inv, int reflect, int variant, int64_t n, uint64_t const *d_reps, uint64_t *d_out, void *stream);
/* Host-only test hooks of the lattice-group form of K4 (trivial sectors of groups that contain every translation of a
 * tw x (L / tw) torus: the translations are walked with bit operations, only one element per coset -- the point group -- goes
 * through a compiled network): the width found (-1: the group has no such subgroup) and the number of cosets; the orbit
 * minimum of `state` computed that way (with the global spin flip folded in when the basis has one; ~0 when not applicable) */
int ls_amd_test_translation_cosets(ls_hs_basis const *basis, int *n_cosets);
uint64_t ls_amd_test_rep_by_cosets(ls_hs_basis const *basis, uint64_t state);
/* ... and of its factorised form (K4 mode 5): when the cosets are the point group of the torus itself -- D2 = {1, r, o, r o}
 * (rows reversed, row order reversed, both) or on a square torus D4 = D2 x {1, transpose}, or a subgroup -- the mask of the
 * images that belong to the group (bits 0-3 of the word, 4-7 of its transpose; 0: the cosets are not of that form).  Then only
 * the transpose is a compiled network and ls_amd_test_rep_by_cosets mirrors THAT routine (LS_AMD_K4=cosets: mode 4). */
int ls_amd_test_d4_mask(ls_hs_basis const *basis);
/* Host-only test hooks of the static index table {representative -> 32-bit payload} of the indexed pull mode
 * (distributed-matvec_amd/csrc/lsk.h: lsk_gtab): bucket bits for n keys of L bits (-1: no admissible shape), a sequential
 * build with the device kernel's placement rule into a malloc'ed array of 2 << bbits entries (release with
 * ls_amd_test_free; payload NULL: the key's position), and the lookup (payload, or -1 when absent) */
int ls_amd_test_gtab_bits(int L, int64_t n);
int ls_amd_test_gtab_build(int L, int bbits, int64_t n, uint64_t const *reps, uint32_t const *payload, uint64_t **entries);
int64_t ls_amd_test_gtab_find(int L, int bbits, uint64_t const *entries, uint64_t key);
/* byte offsets of commInfo / globalSumReal_type inside primme_params as the PRIMME callbacks read them (ls_chpl.h) */
int ls_amd_test_primme_comminfo_offset(void);
int ls_amd_test_primme_sumtype_offset(void);
int ls_amd_test_primme_nlocal_offset(void);
int ls_amd_test_primme_matrix_offset(void);

#ifdef __cplusplus
}
#endif
#endif /* LS_AMD_H */
