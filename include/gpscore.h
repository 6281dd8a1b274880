/*
 * gpscore.h — C-ABI of libgpscore.so, the MI355X (gfx950) GP-regression hot path.
 *
 * Reference being replaced (polarlightman/Scoring-rules-for-Gaussian-process-
 * regression..., aliases as in SURVEY.md §0: KF = kin40k-FULL-compare.py,
 * K20 = KIN40K-COMPARE-ALL-FITC-20.py, SD = "SIMPLE-DATA FULL-comapre.py").
 * The reference has no FFI; its call surface is module-level torch-CPU helpers.
 * Each entry point below names the reference code it replaces.  The ctypes
 * binding that a maintainer would add is gpscore/_lib.py.
 *
 * Conventions
 *  - All arrays are caller-owned, C-contiguous, row-major float64 HOST arrays
 *    unless the name ends in _dev; the library copies H2D/D2H itself.
 *  - Device buffers are owned by the opaque context and reused across calls.
 *  - Return value: 0 ok; >0 LAPACK-style info (the leading minor of that order
 *    is not positive definite, as torch.potrf raises); <0 argument / HIP / RCCL
 *    error, message via gps_last_error().  NaN/Inf propagate, nothing clamps.
 *  - A context is bound to one device and one HIP stream; it is not thread-safe.
 *  - theta layout everywhere: [log_sf2, log_ell_0 .. log_ell_{n_ell-1}, log_sn2]
 *    (n_ell = 1 or d), the reference's log-parameterisation para_k, para_l,
 *    para_noise (KF:7-12, KF:239).  kind: GPS_ARD (b = log ℓ) or GPS_RBF
 *    (b = log ℓ², SD:8-21).
 */
#ifndef GPSCORE_H
#define GPSCORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gps_ctx gps_ctx;

enum { GPS_ARD = 0, GPS_RBF = 1 };
enum { GPS_FULL = 0, GPS_LOWER = 1 };

/* objective vector written by the fit calls */
enum {
  GPS_OBJ_NLML = 0,      /* ½n·log2π + ½log|A| + ½yᵀA⁻¹y            KF:334 / K20:339-340 */
  GPS_OBJ_LOO_CRPS = 1,  /* mean LOO CRPS                             KF:241-245 / K20:222-234 */
  GPS_OBJ_LOO_LOGS = 2,  /* mean LOO log score                        KF:416-424 / K20:434-447 */
  GPS_OBJ_LOGDET = 3,    /* log|A|                                    KF:332 (×2) */
  GPS_OBJ_QUAD = 4,      /* yᵀA⁻¹y                                    KF:334 */
  GPS_N_OBJ = 5
};
/* score vector written by gps_*_predict_score / gps_scores (KF:276-292) */
enum {
  GPS_SC_CRPS = 0, GPS_SC_LOGS = 1, GPS_SC_MSLL = 2, GPS_SC_SMSE = 3,
  GPS_SC_MSE = 4, GPS_SC_COVER = 5, GPS_N_SC = 6
};

/* ---- context ------------------------------------------------------------ */
/* ABI version of this header; gps_version() returns the library's.  Bumped whenever an entry
 * point changes its arguments or an array it writes changes size (500: gps_ctx_stats takes a
 * capacity, gps_comm_info and gps_build_id added; 600: gps_phase_enable / gps_phase_collect /
 * gps_rccl_info added; 700: the joint test predictive, gps_*_predict_cov / _predict_joint /
 * _predict_draws added; 800: the GEMM launch diagnostics gps_gemm_diag / gps_gemm_diag_check /
 * gps_gemm_schedule added; 900: the batched small GPs, gps_full_grad_batch / gps_full_train_batch
 * added).  gps_fitc_grad_batch / gps_fitc_train_batch joined at 900 without a bump:
 * they are purely additive, no existing entry point or array changed; so did gps_potrf_diag
 * (DESIGN §21), gps_fitc_grad_tall / gps_fitc_train_tall, the gradient-layer
 * diagnostics gps_grad_terms_diag / gps_grad_contract_diag / gps_fitc_contract_diag
 * and gps_full_grad_tall / gps_full_train_tall, their block-LOO siblings
 * gps_full_blockloo_grad_tall / gps_full_blockloo_train_tall and
 * gps_fitc_blockloo_grad_tall / gps_fitc_blockloo_train_tall, and the vector-layer
 * diagnostic gps_vec_diag, and the validated fits gps_full_train_tall_va /
 * gps_full_blockloo_train_tall_va and gps_fitc_train_tall_va /
 * gps_fitc_blockloo_train_tall_va, and the block / energy-score / joint kernels'
 * diagnostic gps_block_diag.
 * The binding refuses a mismatch at load. */
#define GPS_ABI_VERSION 900
int gps_version(void);
/* The SHA-256 (hex) of the sources the library was built from (csrc/, this header; computed by
 * gpscore/buildid.py at build time).  Writes at most cap-1 characters and a NUL; returns the
 * id's length. */
int gps_build_id(char* out, int cap);
int gps_ctx_create(int device, gps_ctx** out);
int gps_ctx_destroy(gps_ctx* ctx);
const char* gps_last_error(gps_ctx* ctx);
/* Use an external hipStream_t (e.g. torch's current stream) instead of the ctx's own. */
int gps_ctx_set_stream(gps_ctx* ctx, void* hip_stream);
void* gps_ctx_stream(gps_ctx* ctx);
int gps_ctx_synchronize(gps_ctx* ctx);

/* ---- options ----------------------------------------------------------------
 * Round 6 removed the switches whose other settings had measured slower (4 / 14 fork bounds of
 * the side-stream product, 16 side-stream priority, 22 unfused chain tasks, 24 GEMM wave-priority
 * levels); their keys are refused like any unknown key.  Only options the defaults use.  Round-1 experiments measured neutral or slower on C3
 * (lookahead split, CU-reserved streams, in-launch split-K combine, CU-masked main stream,
 * split-K fill of the trailing update) were removed from the library. */
enum {
  GPS_OPT_OVERLAP = 0,  /* 1 (default): the factorisation's off-critical-path products (and the
                           energy score's folds) run on extra HIP streams; 0: everything on one
                           stream (clean per-kernel timing) */
  GPS_OPT_GEMM_MAP = 3, /* GEMM tile-order override: 0 automatic (default), 1-5 fixed orders, 6 the
                           row norms in paired column tiles (other launches automatic)
                           (A/B measurements; same values bitwise) */
  GPS_OPT_TINY_GEMM = 7, /* 1 (default): the bottom-of-recursion GEMMs (up to the 1280 level)
                            use the small kernel (16/32-blocks per wave, K split over the waves
                            of a workgroup, no LDS staging, no reduce launch); 0: the 64-tile
                            split-K + reduce path for them.  Process-wide. */
  GPS_OPT_GRAM_REG = 9,  /* 2 (default): as 1, with the d = 8, 16 builds on the matrix cores
                            in the reference's expansion 2·x·x'ᵀ − ‖x‖² − ‖x'‖² (KF:15-22;
                            equal to 1 within its rounding); 1: Gram builds with d in {1, 8, 16}
                            keep the column features in registers (128×128 tiles); 0: the
                            LDS-column kernel (bitwise equal to 1).  Process-wide. */
  GPS_OPT_GRAPH = 10,    /* 1 (default): the recursive factorisation's launch sequence is
                            captured once per (buffers, size, streams, options) into a hipGraph
                            and replayed; 0: eager launches.  Same kernels, same results. */
  GPS_OPT_PRED_PRE = 11, /* 1 (default): gps_fitc_fit forms the row-norm columns
                            q_i = ‖Lm⁻¹k_i‖² that need only the top-level Lm11⁻¹ (a quarter of
                            the pass) on a second stream while the rest of Lm's factorisation
                            runs; 0: the whole pass after it.  Same tiles, same results. */
  GPS_OPT_DAG = 12,      /* 1 (default): diagonal blocks of at most GPS_OPT_DAG_TILES 128-tiles
                            at the bottom of the recursive factorisation are factored and
                            inverted by ONE persistent launch (a device task queue of tile
                            products, per-tile arrival counters); 0: the recursion down to
                            the 128-block leaf.  Same algorithm, other summation order. */
  GPS_OPT_AR_CHUNKS = 15, /* sharded FITC: B's all-reduce in this many row blocks (default 4),
                             each on a comm stream while the next block's SYRK runs; 1: one
                             all-reduce after the SYRK.  Same bits either way. */
  GPS_OPT_DAG_TILES = 13, /* largest block (in 128-tiles, 2..64, default 20) the persistent
                            factorisation takes */
  GPS_OPT_STREAM_K = 18,  /* the stream-K tail of a 128-tile GEMM launch with uniform K ranges (the
                             trailing-update SYRKs) whose last round of workgroup slots would be at
                             most 3/4 full: that round's tiles split into equal K runs over every
                             slot (in-launch fixed-order combine).  2 (default): for a trailing update
                             that runs alone (overlap off, or below the fork level) — beside the side
                             stream's T product the round is filled already; 1: every eligible
                             launch; 0: never.  Process-wide. */
  GPS_OPT_DAG_WGS = 19,   /* workgroups of a persistent factorisation launch; 0 (default):
                             automatic — one per CU for the full GP, half the CUs for the FITC
                             m×m factorisations (the test pre-pass runs beside them) */
  GPS_OPT_DAG_GROUP = 17, /* persistent factorisation: 16-deep operand chunks a strip task has in
                             flight per load group (2, 3 (default) or 4).  Same values bitwise. */
  GPS_OPT_SLAB_XCD = 26,  /* 1: split-K GEMM launches (the FITC SYRK, small trailing updates) deal
                             their (tile, K slice) pairs slice-major, each XCD a contiguous run,
                             so one XCD's resident workgroups share a slice's operand rows in its
                             L2 (default; C4's SYRK 7x -> 2.9x its operand in L2-fabric bytes,
                             time neutral); 0: tile-major.  Same values bitwise.  Process-wide. */
  GPS_OPT_DAG_ORDER = 25, /* queue order of the persistent factorisation's tasks: 1 (default)
                             largest upward rank with the round-4 measured task durations, 2 the
                             same with round 3's, 0 earliest estimated start.  Same values bitwise
                             (the order changes only which workgroup runs a task, and when). */
  GPS_OPT_FITC_DEP = 27,  /* 1 (default): when K̃mm's factorisation is one persistent launch (m_pad ≤
                             20 tiles), the q_i = ‖Lm⁻¹k_i‖² row norms start on a second stream while
                             it runs, each column tile as soon as its row of Lm⁻¹ is final
                             (device-side row signals), and a completion launch after it takes
                             the tiles left; with m_pad > 20 tiles (a recursive factorisation)
                             the same for the q pre-pass over the top-level L11⁻¹ columns when
                             that block is one persistent launch and the pre-pass ≤ 8192 tiles,
                             and for the r pre-pass behind Lb's L11 block at ≤ 4096 tiles;
                             0: the row norms after the factorisation.  Same tiles, same values
                             bitwise. */
  GPS_OPT_DAG_TILES_FULL = 28, /* largest block (in 128-tiles, 2..64; default 40) the persistent
                             factorisation takes in the full GP's fit; 0: GPS_OPT_DAG_TILES.
                             Every other factorisation (FITC m×m, gps_potrf_diag, the block-LOO
                             folds) keeps GPS_OPT_DAG_TILES. */
  GPS_OPT_DAG_KBATCH = 29,  /* persistent factorisation: B | g << 4 [| 256] — the UPD / UPDX terms
                             of one tile run as single products over up to B adjacent K tiles (B
                             in 2..8), the last g (0..3) terms of every tile staying single
                             tasks; with 256 only in blocks of more than GPS_OPT_DAG_TILES tiles
                             (those GPS_OPT_DAG_TILES_FULL admits: smaller blocks are bound by
                             their leaf chain and gain nothing).  B = 0 or 1: every term a task
                             of its own, the queue of before.  Default 8 | 256.  Same algorithm,
                             other summation order within a batch; for a given value the bits do
                             not depend on the queue order, the workgroup count or the load
                             group. */
  GPS_OPT_DAG_TILE_FORM = 30, /* persistent factorisation: minlen | d << 4 — a K batch (option 29)
                             of an off-diagonal tile with at least minlen (1..8) terms, whose last
                             term ends at least d (0..15) tile columns short of the column where
                             the tile is consumed, runs as ONE task on one workgroup, each wave a
                             64×64 block, instead of four 32-row strips.  0: strips only, the
                             queue of before word for word.  Acts only in blocks that have
                             batches.  Default 2 | 2 << 4.  For a given option 29 the bits are those of
                             the strips (same K range and per-element product chain; DESIGN
                             §29). */
  GPS_OPT_GEMM_LIVE = 31,   /* 1 (default): the 64/128-tile GEMM skips the MFMA blocks of an edge
                             tile that lie wholly in the padding, where the caller knows the
                             products to be exact zeros (rows >= n of the full GP's factorisation
                             products and of the predictive product) or never read (its columns
                             >= n*); 0: every block multiplied.  Same values bitwise for finite
                             operands. */
  GPS_OPT_GEMM_PIPE = 32,   /* 1 (default): full 128-tiles of the store and column-reduction GEMM
                             kernels run the pipelined steady-state loop (the LDS stores of the
                             prefetched slice issued between the MFMAs of the last two k steps,
                             fragment reads a fixed distance ahead, issue order pinned); 0: the
                             loop of before.  Edge tiles, k-scaled launches, the row-norm
                             epilogues, the 64-tile and small kernels and the stream-K tail's
                             tiles run the loop of before either way.  Same values bitwise
                             (DESIGN §38). */
};
int gps_ctx_set_option(gps_ctx* ctx, int key, int value);

/* Context statistics: out[GPS_STAT_GRAPHS] factorisation graphs cached (one per distinct
 * (buffers, size, streams, options); each holds its instantiated launch sequence, ~1-3 MB of
 * host memory and a few KB of device memory), out[GPS_STAT_GRAPH_CAP] the cache's capacity
 * (least recently used exec destroyed beyond it), out[GPS_STAT_GRAPH_OVERFLOW] 0 (kept for the
 * layout: no factorisation runs eagerly for want of a slot), out[GPS_STAT_DEVICE_BYTES] device
 * memory held by the context's buffers, out[GPS_STAT_GRAPH_DROPPED] execs destroyed because a
 * buffer they use was freed or grown (a graph never outlives its buffers),
 * out[GPS_STAT_GRAPH_EVICTED] execs destroyed by the capacity limit. */
enum { GPS_STAT_GRAPHS = 0, GPS_STAT_GRAPH_CAP = 1, GPS_STAT_GRAPH_OVERFLOW = 2,
       GPS_STAT_DEVICE_BYTES = 3, GPS_STAT_GRAPH_DROPPED = 4, GPS_STAT_GRAPH_EVICTED = 5,
       GPS_N_STATS = 6 };
/* Writes min(cap, GPS_N_STATS) entries; returns GPS_N_STATS (the count this library knows). */
int gps_ctx_stats(gps_ctx* ctx, int64_t* out, int cap);

/* Diagnostics: the persistent factorisation's task queue for a block of T tiles (2..64), one
 * word per strip task (type | part << 3 | fine << 7 | i << 8 | j << 16 | k << 24; types 0 LEAF,
 * 1 TRSM, 2 UPD, 3 UPDX, 4 FIN; flags bit 0: the chain tasks' fine parts (the library's queue),
 * bits 2-3: the order (GPS_OPT_DAG_ORDER: 0 or 1 the default 1, 2 order 2, 3 order 0), other
 * bits rejected — kernels_potrf.hip).  Returns the queue length (writes at most cap words);
 * needs no device. */
int gps_dag_task_list(int T, int flags, uint32_t* out, int cap);
/* The same with K batches (GPS_OPT_DAG_KBATCH): kb in 1..8 terms per UPD / UPDX task, the last
 * kg in 0..3 terms of every tile single.  i, j, k take 6 bits each; the batch length − 1 sits in
 * bits 14-15 (low two) and 22 (high), k (UPD) resp. j (UPDX) naming the batch's first term.
 * kb = 1 gives gps_dag_task_list's words exactly. */
int gps_dag_task_list_ex(int T, int flags, int kb, int kg, uint32_t* out, int cap);
/* The same with the tile form (GPS_OPT_DAG_TILE_FORM's value tf: 0, or minlen | d << 4): a batch
 * in tile form is one word with bit 23 set and part 0, standing for the four strips of its tile.
 * tf = 0 gives gps_dag_task_list_ex's words exactly. */
int gps_dag_task_list_tf(int T, int flags, int kb, int kg, int tf, uint32_t* out, int cap);
/* What each of n task words means to the kernel, by the functions the kernel and the generator
 * use (csrc/dag_task.h): per word GPS_DAG_PROTO_ROW ints in out —
 *   [0..7]   type, part, fine, i, j, k, len (terms of the K batch), tile (the tile form);
 *   [8..19]  three polled counts (array, i, j, threshold): the task runs once array[i][j] >=
 *            threshold for each; array 0 = the A side (acnt), 1 = the X side (xcnt), −1 = unused
 *            (then i, j, threshold are 0);
 *   [20..27] two arrivals (array, i, j, increment) added when the task is done, unused as above.
 * T in 2..64 (the counters' row length); a word of unknown type or with i, j, k (or its batch's
 * last term) outside the block is refused.  Returns n; needs no device. */
enum { GPS_DAG_PROTO_ROW = 28 };
int gps_dag_task_protocol(int T, const uint32_t* words, int n, int32_t* out);

/* Diagnostics: ONE internal FP64 GEMM launch (csrc/kernels_gemm.hip's launch_gemm, through the
 * same gemm() every production caller uses, on the context's main stream with that stream's
 * split-K workspace and stream-K tickets) on host arrays copied to the device unpadded — the
 * tests drive each kernel variant alone with it (tests/test_gpu_gemm_modes.py).  Not
 * API: the description mirrors the internal GemmParams and changes with it.
 *   lay_a / lay_b  0: A stored [i][k] / B stored [k][j]; 1: A stored [k][i] / B stored [j][k]
 *   epi            0 store, 1 row squares, 2 column reduction, 3 row squares + row dot
 *   tri            0 none, 1 k <= i, 2 k <= j, 3 k >= j, 4 k >= i (128-tile granular, shifted by
 *                  tri_off), 5 per 16-column group [kr[2g], kr[2g+1])
 *   tile           0 automatic (gemm_plan), 16 / 32 the small kernel (ksplit = waves per block:
 *                  1, 2, 4), 64 / 128 the LDS kernel (ksplit = K slices)
 *   use_ws         a split (ksplit > 1) goes through the workspace slabs and the reduction
 *                  kernel; 0: slice s writes C + s·c_kslice_stride (beta 0, 128-tiles)
 *   dep_mode       must be 0 (the dependent row-norm launch waits on a running factorisation)
 * Array extents (doubles): A rows×lda with rows = M (lay_a 0) or K; B rows×ldb with rows = K
 * (lay_b 0) or N; C M×ldc, or ksplit·c_kslice_stride for the unslabbed split (epi 0 only, else
 * may be NULL); kscale K or NULL; w M (epi 2) or K (epi 3); kr 2·N/16 ints (tri 5); out0
 * (N/128)×ld_out (epi 1, 3) or (M/128)×ld_out (epi 2); out1 as out0 (epi 2) or M (epi 3).  C,
 * out0 and out1 go to the device as given and come back whole, so what a launch leaves unwritten
 * keeps the caller's values. */
typedef struct gps_gemm_desc {
  int32_t lay_a, lay_b, epi;
  int32_t M, N, K;               /* M, N multiples of 128, K of 16 */
  int64_t lda, ldb, ldc;         /* even, at least the stored row length */
  double alpha, beta;
  int32_t tri, tri_off;          /* tri_off >= 0, a multiple of 16 */
  int32_t lower_out, mirror;
  int32_t kend;                  /* 0 or a multiple of 16: A's columns from kend on are zero */
  int32_t tile, ksplit, map_mode;
  int32_t use_ws, sk_alone, dep_mode;
  int32_t reserved;
  int64_t ld_out, c_kslice_stride;
} gps_gemm_desc;
/* the launch as launch_gemm chose it */
enum { GPS_GEMM_PLAN_TILE = 0, GPS_GEMM_PLAN_KSPLIT = 1, GPS_GEMM_PLAN_MAP = 2,
       GPS_GEMM_PLAN_SK_DP = 3, GPS_GEMM_PLAN_SK_WGS = 4, GPS_GEMM_PLAN_SLAB_XCD = 5,
       GPS_GEMM_PLAN_GRID_X = 6, GPS_GEMM_PLAN_GRID_Y = 7, GPS_N_GEMM_PLAN = 8 };
/* 0 if gps_gemm_diag would run the description, else -1 with the reason in
 * gps_last_error(NULL): every description that could make a kernel read or write outside the
 * arrays above, and every combination launch_gemm rejects, is refused here.  have_* say which
 * optional arrays the caller has (kr itself is read: entries in [0, K], multiples of 16).
 * Needs no device. */
int gps_gemm_diag_check(const gps_gemm_desc* d, int have_c, int have_kscale, int have_w,
                        const int32_t* kr, int have_out0, int have_out1);
/* Runs the launch (after gps_gemm_diag_check, before anything touches the device: -1 on a
 * refused description) and writes plan[GPS_N_GEMM_PLAN]. */
int gps_gemm_diag(gps_ctx* ctx, const gps_gemm_desc* d, const double* A, const double* B,
                  double* C, const double* kscale, const double* w, const int32_t* kr,
                  double* out0, double* out1, int32_t* plan);
/* Diagnostics, beside gps_dag_task_list: the work items the workgroups of that launch would run,
 * enumerated on the host by the very functions the kernels call (csrc/gemm_schedule.h) — 8 ints
 * per item: workgroup (x + y·grid_x), tile row ti, tile column tj (in units of the plan's tile),
 * k begin, k end, K slice (small kernel: the wave's part), stream-K workspace slot (−1: none) and
 * the ticket count the tile's last arriver waits for (0: no combine).  slots: the chip's workgroup
 * slots for the stream-K tail (2 per CU; 0: no tail).  The option switches (GPS_OPT_STREAM_K, ...)
 * apply as they are set.  Writes plan[GPS_N_GEMM_PLAN] and at most cap items; returns the item
 * count, -1 on a refused description.  Needs no device. */
int64_t gps_gemm_schedule(const gps_gemm_desc* d, const int32_t* kr, int have_kscale, int slots,
                          int32_t* plan, int32_t* items, int64_t cap);
/* Diagnostics, beside gps_gemm_schedule: whether that launch's kernel would be told to run the
 * pipelined loop of its full 128-tiles when GPS_OPT_GEMM_PIPE is `pipe` — 1, or 0 where launch_gemm
 * clears the request (the option off, 64-tiles, the small kernel, the row-norm epilogues, a
 * k-scaled launch); -1 on a refused description.  Needs no device. */
int gps_gemm_pipe_resolved(const gps_gemm_desc* d, const int32_t* kr, int have_kscale, int pipe);

/* Diagnostics: the factorisation with its fused inverse as gps_potrf runs it (the same upload,
 * buffers, options, graph capture and replay), everything it wrote copied back whole
 * (tests/test_gpu_factor.py).  With n_pad = n rounded up to 128: L and Linv take the
 * padded n_pad × n_pad squares (row stride n_pad) — the upper parts the kernels never write and
 * the identity padding included — and logdiag the n_pad values log L_ii.  *info is 0 or the first
 * non-positive-definite leading minor; the call RETURNS 0 in both cases (the launches complete
 * on a bad pivot, the factors hold NaNs from there on), -1 on a bad argument (NULL, n <= 0,
 * lda < n; nothing is launched), other negatives as everywhere.  plan[GPS_N_POTRF_PLAN]: what
 * ran — n_pad, stand-alone 128-leaf launches, persistent launches with their smallest and largest
 * block (in tiles; 0 without one), the recursion's GEMM launches, and 1 if the sequence was
 * replayed from a cached graph (the counts then are those of its capture). */
enum { GPS_POTRF_PLAN_NPAD = 0, GPS_POTRF_PLAN_LEAVES = 1, GPS_POTRF_PLAN_DAGS = 2,
       GPS_POTRF_PLAN_DAG_TMIN = 3, GPS_POTRF_PLAN_DAG_TMAX = 4, GPS_POTRF_PLAN_GEMMS = 5,
       GPS_POTRF_PLAN_REPLAYED = 6, GPS_N_POTRF_PLAN = 8 };
int gps_potrf_diag(gps_ctx* ctx, int64_t n, const double* A, int64_t lda, double* L, double* Linv,
                   double* logdiag, int32_t* info, int32_t* plan);

/* Diagnostics: the gradient layer's kernels one launch at a time on host arrays
 * (tests/test_gpu_grad_terms.py).  Each call judges its arguments before anything
 * touches the device (-1 with the reason in gps_last_error), uploads, calls the production
 * launcher, and copies the outputs back; what a kernel must write, and what it must not read, is
 * NaN on the device beforehand.
 *
 * gps_grad_terms_diag, the per-point terms.  in / out are arrays of pointers (in: 8, out: 6
 * slots; unused slots are not read), every vector n long on input and n_pad long on output:
 *   which 0  loo_grad_terms   in {y, alpha, dinv}; obj LOO_CRPS / LOO_LOGS; out {u, ct}
 *   which 1  fitc_grad_terms  in {y, lam, r, g}; obj NLML / LOO_*; scal = n_total;
 *                             out {alpha, dinv, v, ulam, h, hl2}
 *   which 2  fold_terms       in {y, r, c}; n = b = n_pad; out {gm or NULL, gc, value[1]}
 *                             (gc may be NULL with gm)
 *   which 3  fitc_grad_mdiag  in {KN or NULL, K, lam, r, dinv, alpha, v, h or NULL}, KN and K
 *                             [n][m_pad] (m_pad even; K may be NULL with KN); scal = a;
 *                             out {mdiag, s1, s2, s3}
 * m_pad is read by which 3 only. */
int gps_grad_terms_diag(gps_ctx* ctx, int which, int obj, int64_t n, int64_t n_pad, int64_t m_pad,
                        double scal, const double* const* in, double* const* out);
/* launch_grad_contract on X [n][d], Ainv / Mx [n][ld] (either NULL with its coefficient a[0] /
 * a[3] zero; v NULL with a[2] zero — the kernel then gets a buffer of NaN, not a null pointer),
 * a[4] = {a0, a1, a2, a3}.  out: ceil(d/16) × 18 doubles as the launcher writes them —
 * per pass [Σ w·m·K, Σ_{i=j} m, Σ w·m·K·Δ_k² for the pass's 16 dimensions]. */
int gps_grad_contract_diag(gps_ctx* ctx, int64_t n, int d, const double* X, const double* inv_ell,
                           double sf2, const double* Ainv, const double* Mx, int64_t ld,
                           const double* alpha, const double* v, const double* a, double* out);
/* launch_fitc_grad_contract on xr [nr][d], xc [nc][d], nt <= 4 matrix terms R[t] [nr][ldr[t]] with
 * coef[t] and row scales rs[t] (rs, or any rs[t], may be NULL), two rank-one terms pc[q]·pv[q]·
 * qv[q]ᵀ (pc[q] = 0: off, the vectors are not read).  out: ceil(d/16) × 17 doubles
 * [Σ G·K, Σ G·K·Δ_k²], zout [nc][d] = Σ_i G·K·Δ_k.  On the device every array has a NaN tail past
 * its real rows and columns. */
int gps_fitc_contract_diag(gps_ctx* ctx, int64_t nr, int64_t nc, int64_t nc_pad, int d,
                           const double* xr, const double* xc, const double* inv_ell, double sf2,
                           int nt, const double* const* R, const int64_t* ldr, const double* coef,
                           const double* const* rs, const double* pc, const double* const* pv,
                           const double* const* qv, double* out, double* zout);

/* Diagnostics: the vector layer's kernels (csrc/kernels_vec.hip) one production launch_* call at
 * a time on host arrays (tests/test_gpu_vec.py).  The call judges its arguments before
 * anything touches the device (-1 with the reason in gps_last_error; the launchers' own refusals
 * — odd cols, odd ld, crows < 1, n outside 1..64 for the local sum, the transposed trmv — are
 * among them), uploads, and copies the outputs back.  On the device everything the kernel must
 * write and everything it must not read is NaN beforehand: the strict-upper 128-tiles of the
 * lower forms, the row gaps where ld exceeds the row length, one slab past the nslab real ones,
 * the vectors past their real length, and the outputs.  An optional operand that is NULL here
 * is NULL in the launch.  dims: 8 integers, scal: 2 doubles, in / out: 8 pointer slots each
 * (unused entries are not read).  Matrices are dense row-major on the host ([rows][cols]); the
 * device copy has the row stride given in dims.  With n_pad = n rounded up to 128:
 *   which  launcher                 dims                              in -> out
 *   0  launch_gemv_full / _lower /  {mode 0 full 1 lower 2 trmv,      {M, x} -> {y [rows]}
 *      launch_trmv_lower             rows, cols, ldm, trans}
 *   1  launch_colred                {rows, cols, ldm, lower, crows}   {M, w|NULL, rowscale|NULL}
 *                                                                      -> {s1|NULL, s2|NULL}
 *   2  launch_colred_partials       {rows, cols, ldm, lower}          {M, w} -> {slab [2][nchunk]
 *                                                                      [cols], count [1]}
 *   3  launch_slab_sum              {nslab, len, ld}                  {slab [nslab][len],
 *                                                                      init|NULL} -> {out [len]}
 *   4  launch_sym_slab_sum          {nslab, M, stride}                {slab [nslab][M*M],
 *                                                                      base|NULL} -> {dst [M*M]}
 *   5  launch_sym_pack (rows [r0,   {nslab, M, stride, m, r0, r1,     same -> {packed [m(m+1)/2]
 *      r1)), then launch_sym_unpack  unpack, full}                     (uploaded first: what the
 *      if unpack                                                       pack leaves alone stays),
 *                                                                      dst [M*M] if unpack}
 *   6  launch_full_loo              {n, nslab, ld}                    {y [n], slab1, slab2
 *                                                                      [nslab][n_pad], beta,
 *      logdiag [n_pad]} -> {alpha, dinv, mu_loo, var_loo [n_pad], obj [5], sums [4]}
 *   7  launch_fitc_lambda           {n, n_pad, nslab, ld}; scal       {slab [nslab][n_pad], y [n]}
 *                                    {sf2, sn2}                        -> {q, lam, inv_lam, ys
 *                                                                      [n_pad], sums [2]}
 *   8  launch_fitc_loo              {n, n_pad, nslab, ld}             {y, lam [n], slab [nslab]
 *      [n_pad], g [n]} -> {r, mu_loo, var_loo [n_pad], sums [2]}
 *   9  launch_pred_finalize /       {nt, fitc}; scal {base_var}       {s1|qm, s2|qb [nt]} ->
 *      launch_fitc_pred_finalize                                       {mu (fitc 0), var [nt]}
 *   10 launch_surface_point_sums    {n, add_noise}; scal {s2}         {y, alpha, dinv} -> {sums [2]}
 *   11 launch_dot                   {n}                               {a, b|NULL} -> {out [1]}
 *   12 launch_pad_copy              {rows, cols, lds, rows_pad,       {src [rows][cols]} ->
 *                                    cols_pad, ldd, pad_identity}      {dst [rows_pad][ldd]}
 *   13 launch_local_sum             {n, count}                        {src [n][count]} ->
 *                                                                      {out [count]}
 * Entries of mu_loo / var_loo past n are never written and come back NaN. */
int gps_vec_diag(gps_ctx* ctx, int which, const int64_t* dims, const double* scal,
                 const double* const* in, double* const* out);

/* Diagnostics: the block-LOO, energy-score and joint-predictive kernels (csrc/kernels_block.hip,
 * csrc/kernels_joint.hip, and fitc_grad_v / fitc_grad_y of csrc/kernels_fitc_grad.hip) one
 * production launch_* call at a time on host arrays (tests/test_gpu_block.py).  As
 * gps_vec_diag: the arguments are judged before anything touches the device (-1 with the reason in
 * gps_last_error; the launchers' own refusals — odd cols / ld / m_pad, bp % 64 for es_dist, S < 2
 * or Sp < S + 1 for es_reduce, joint_cov's bp % 128, d outside 1..GPS_MAX_D and ks < 1 — are among
 * them), and on the device everything is NaN beforehand, with a 16-double NaN gap after every
 * array.  dims: 8 integers, scal: 8 doubles, in: 12 pointer slots, out: 4.  An input is dense on
 * the host ([rows][cols]) and has the row stride given in dims on the device.  An output is its
 * device image: [rows][ld] doubles and the 16 of the gap after it, so what the kernel left alone
 * (row gaps, the gap, entries it must not write) comes back NaN.  "in/out": the kernel reads the
 * array too; its first contents are taken from the host image (the row gaps stay NaN whatever the
 * host holds there).  An optional operand that is NULL here is NULL in the launch.
 *   which  launcher            dims                          in -> out
 *   0  launch_fold_grad        {b, ldp, ldh, ldg}; scal      {PI [b][b], H|NULL, r [b], w|NULL}
 *                               {c0, c1, c2, c3, gr, gw}      -> {G [b][ldg], g [b]}
 *   1  launch_row_dots         {rows, cols, lda, ldb, same}  {A, B|NULL, t|NULL [cols]} ->
 *                               same 1: B is A's own array    {at|NULL, ab|NULL [rows]}
 *   2  launch_lr_fold_vec      {mode, b, bp}                 {lam, x, at, ab, r, c, w, gc, q [b]}
 *                                                             (those the mode reads) -> {o1, o2 [bp]}
 *                                                             (o2 may be NULL in mode 1)
 *   3  launch_lr_combine       {rows, rows_pad, cols, ldx,   {X, Y, lam, rs|NULL, u1|NULL, v1|NULL,
 *                               ldy, ldo}; scal {c0, c1, c2}  u2|NULL, v2|NULL} -> {out [rows_pad][ldo]}
 *   4  launch_fold_sum         {nslab, skip, len, stride,    {slab [nslab][len], base|NULL,
 *                               inplace}; scal {sgn}          base2|NULL} -> {dst [len]}; inplace 1:
 *                                                             dst is base (in/out); one NaN slab follows
 *   5  launch_fold_logdet      {m, b}                        {ldf, ldb [m], lam [b]} -> {out [1]}
 *   6  launch_row_scale        {rows, cols, ld}              {scale [rows]} -> {M in/out}
 *   7  launch_vec_mul          {n}                           {a, b} -> {out [n]}
 *   8  launch_blk_mdiag        {n, n_pad, m_pad, ldf, ldus,  {F, US, U [n][m_pad], gd, lam, v, alpha
 *                               ldu, ldy, alias}              [n]} -> {md, sc [n_pad], Y [n_pad][ldy]};
 *                                                             alias 1: Y is US (in/out, in[1] NULL)
 *   9  launch_ns_init          {b, bp, ldc}; scal {scale,    {C [b][b]|NULL} -> {Y [bp][bp]}
 *                               pad}
 *   10 launch_diag_add_const   {n, ld}; scal {c}             {} -> {M [n][ld] in/out}
 *   11 launch_sym_avg          {n, ld}                       {} -> {M [n][ld] in/out}
 *   12 launch_scaled_row       {b, bp}; scal {scale}         {src [b]} -> {dst [bp]}
 *   13 launch_row_axpy         {rows, cols, ldc, ldz}        {Z, sv [rows]} -> {C [rows][ldc] in/out}
 *   14 launch_ns_resid         {n, ld}                       {T [n][n]} -> {out [1]}
 *   15 launch_es_dist          {S, bp, ldd}                  {Z [S][bp], Zh [S+1][bp]} -> {D [ldd][ldd]}
 *   16 launch_es_reduce        {S, Sp, ldd, grad}; scal      {} -> {D [Sp][ldd] in/out, rs|NULL,
 *                               {beta}                        cs|NULL [Sp], out [1]}; D's rows >= S and
 *                                                             columns > S are NaN going in
 *   17 launch_joint_cov        {b, bp, d, ks, stride}; scal  {x [b][d], inv_ell [d], slab [ks][bp*bp]}
 *                               {sf2, sn2}                    -> {out [bp][bp]}; the slabs are NaN in the
 *                                                             strict-upper 32-tiles, rows and columns >= b
 *   18 launch_joint_resid      {b, bp}                       {y, mu [b]} -> {r [bp]}
 *   19 launch_joint_dss        {b}                           {logdiag, t [b]} -> {out [1]}
 *   20 launch_sign_fill        {npos, n}                     {} -> {dst [n]}
 *   21 launch_row_add          {rows, cols, ld}              {mu [cols]} -> {M [rows][ld] in/out}
 *   22 launch_fitc_grad_v      {n}                           {ulam, z, lam|NULL} -> {v [n]}
 *   23 launch_fitc_grad_y      {rows, cols, ld, alias}       {U, UP|NULL [rows][cols], s1, s2|NULL}
 *                                                             -> {Y [rows][ld]}; alias 1: Y is UP (in/out) */
int gps_block_diag(gps_ctx* ctx, int which, const int64_t* dims, const double* scal,
                   const double* const* in, double* const* out);

/* on: 0 off, 1 per-kernel-class tags, 2 GEMM tags also carry layout/shape/tri/split-K/lda */
int gps_prof_enable(gps_ctx* ctx, int on);
/* Synchronises, then writes a JSON object {tag: {count, ms, flop, bytes}} and clears. */
int gps_prof_collect(gps_ctx* ctx, char* json_out, int64_t cap);
/* Phase timing of the FITC forward on its production schedule (the launches, streams and their
 * overlap are unchanged; gps_prof_enable instead serialises them): with on, every FITC forward
 * (gps_fitc_fit, the gradients' and block-LOO's forward) records a timing event on its main
 * stream at each phase boundary, and two around every all-reduce on the stream that issues it.
 * Phases, each the main-stream time since the previous mark (K20:222-234 restated):
 *   "kmm_lm"   K̃mm and Lm's factorisation (replicated on every rank; Knm's Gram beside it),
 *   "knm"      the wait for Knm (sharded),  "q" the q row norms and λ (sharded),
 *   "syrk"     B's split-K SYRK with its packing (sharded; the row-block all-reduces beside it),
 *   "exchange" the main stream's wait for B's last all-reduce (exposed exchange),
 *   "lb"       B's unpack and Lb's factorisation, "c" c = B⁻¹b (replicated),
 *   "r"        the r row norms, g and the LOO terms (sharded), "scal" the scalar all-reduce.
 * gps_phase_collect synchronises and writes {"phases": {name: {"count", "ms"}}, "allreduce":
 * [[bytes, ms], ...]} (one pair per all-reduce, on its own stream) and clears. */
int gps_phase_enable(gps_ctx* ctx, int on);
int gps_phase_collect(gps_ctx* ctx, char* json_out, int64_t cap);
/* The RCCL this process runs: ncclGetVersion and the file holding ncclAllReduce as the dynamic
 * linker resolved it (the library links librccl.so.1 from /opt/rocm/lib; a process that loaded a
 * librccl.so.1 first — torch's bundled copy, when torch is imported before the library — runs
 * that one).  Writes at most cap-1 characters and a NUL to path; needs no device. */
int gps_rccl_info(int* version, char* path, int cap);

/* ---- L1 building blocks ---------------------------------------------------- */
/* ARD(x, xp, a, b) KF:7-23 / rbf SD:8-21: out[n][m] = sf2·exp(−½‖(x−x')/ℓ‖²)
 * (+ diag_add where i == j); uplo GPS_LOWER writes only j <= i. */
int gps_gram(gps_ctx* ctx, int kind, const double* X, int64_t n, const double* Xp,
             int64_t m, int d, double log_sf2, const double* log_ell, int n_ell,
             double diag_add, int uplo, double* out);
/* torch.potrf(A).diag().log().sum() (KF:332): lower Cholesky L written into A
 * (lower triangle, upper zeroed); *logdet = log|A|.  Returns info > 0 if not PD. */
int gps_potrf(gps_ctx* ctx, int64_t n, double* A, int64_t lda, double* logdet);
/* chol_solve(B, A) KF:25-29: X = A⁻¹·B for SPD A (n×n) and B (n×nrhs). */
int gps_potrs(gps_ctx* ctx, int64_t n, int64_t nrhs, const double* A, int64_t lda,
              const double* B, int64_t ldb, double* X, int64_t ldx);
/* diag(chol_solve(I, A)) KF:242: dinv[i] = (A⁻¹)_ii. */
int gps_diag_inv(gps_ctx* ctx, int64_t n, const double* A, int64_t lda, double* dinv);
/* torch.mm in the reference helpers (Q KF:38, cal_mean_and_cov KF:123-125,
 * spgp_cal_mean_and_cov K20:81-82): C = alpha·op(A)·op(B) + beta·C on the FP64
 * MFMA path; op(X) = Xᵀ when trans != 0. */
int gps_gemm(gps_ctx* ctx, int transA, int transB, int64_t M, int64_t N, int64_t K, double alpha,
             const double* A, int64_t lda, const double* B, int64_t ldb, double beta, double* C,
             int64_t ldc);
/* crps/logs/trivial_loss/SMSE/MSE/coverage of a Gaussian predictive (KF:52-68,
 * 110-134, 276-292); var is the VARIANCE.  ytr_mean / ytr_var_unbiased are
 * the train-target statistics trivial_loss and SMSE use. */
int gps_scores(gps_ctx* ctx, const double* mu, const double* var, const double* y,
               int64_t nt, double ytr_mean, double ytr_var_unbiased, double out[GPS_N_SC]);

/* ---- full GP (fused hot path) --------------------------------------------- */
/* Upload training data (kept resident until replaced). */
int gps_full_set_data(gps_ctx* ctx, const double* X, const double* y, int64_t n, int d);
int gps_full_set_test(gps_ctx* ctx, const double* Xt, const double* yt, int64_t nt);
/* One forward evaluation of the per-iteration bodies KF:239-245, 329-334,
 * 416-424 at theta: Gram + potrf + L⁻¹ + α + diag(A⁻¹) → objectives.
 * mu_loo / var_loo (length n) may be NULL (kept on device). */
int gps_full_fit(gps_ctx* ctx, int kind, const double* theta, int n_ell,
                 double obj[GPS_N_OBJ], double* mu_loo, double* var_loo);
/* Forward + analytic gradient of one objective (GPS_OBJ_NLML / _LOO_CRPS / _LOO_LOGS) at
 * theta: what one GD iteration of the reference computes with autograd `.backward()`
 * (KF:252 LOO-CRPS, KF:339 NLML, KF:428 LOO-LogS) before its SGD update (KF:254-260).
 * grad (length 2 + n_ell) = [d/d log sf2, d/d b (n_ell), d/d log sigma2] in the
 * reference's parameterisation (para_k, para_l, para_noise).  Also leaves the factor
 * for gps_full_predict, like gps_full_fit. */
int gps_full_grad(gps_ctx* ctx, int kind, const double* theta, int n_ell, int objective,
                  double obj[GPS_N_OBJ], double* grad);
/* Predictive mean/variance at the test points with the last fit's factor
 * (cal_mean_and_cov KF:121-126, diag of the covariance), plus the score bundle
 * against yt (KF:276-292).  mu / var may be NULL; sc may be NULL. */
int gps_full_predict(gps_ctx* ctx, double* mu, double* var, double sc[GPS_N_SC]);

/* ---- FITC sparse GP (Woodbury restatement of K20:32-39, 76-83, 222-340) ----- */
int gps_fitc_set_data(gps_ctx* ctx, const double* X, const double* y, int64_t n, int d,
                      double ytr_mean, double ytr_var_unbiased, int64_t n_total);
int gps_fitc_set_test(gps_ctx* ctx, const double* Xt, const double* yt, int64_t nt,
                      int64_t nt_total);
int gps_fitc_set_inducing(gps_ctx* ctx, const double* Z, int64_t m);
/* FITC objectives over this rank's rows.  With a communicator (gps_comm_init)
 * the m×m accumulator and scalar partials are all-reduced over RCCL; objectives
 * are then global and mu_loo / var_loo hold this rank's rows.  With a test set resident
 * (gps_fitc_set_test) and GPS_OPT_OVERLAP on, the fit also forms the test-side row norms
 * ‖Lm⁻¹k*‖² and ‖Lb⁻¹k*‖² on a second stream where its own chain leaves the chip idle, so
 * gps_fitc_predict is left with μ* and the finalise; a new test set voids them. */
int gps_fitc_fit(gps_ctx* ctx, const double* theta, int n_ell, double obj[GPS_N_OBJ],
                 double* mu_loo, double* var_loo);
/* Forward + analytic gradient of one FITC objective w.r.t. theta AND the inducing
 * inputs: the reference's `.backward()` through its dense FITC bodies at K20:236
 * (LOO-CRPS), K20:344 (NLML), K20:452 (LOO-LogS) before the SGD step that also moves
 * inducing_x (K20:238-247).  grad (2 + n_ell) as gps_full_grad; grad_z (m×d, row-major,
 * may be NULL) = d obj / d Z.  O(n·m²); with a communicator every rank gets the global
 * gradient. */
int gps_fitc_grad(gps_ctx* ctx, const double* theta, int n_ell, int objective,
                  double obj[GPS_N_OBJ], double* grad, double* grad_z);
int gps_fitc_predict(gps_ctx* ctx, double* mu, double* var, double sc[GPS_N_SC]);
/* Diagnostics: the last FITC forward's device intermediates, unpadded and row-major — Knm (n×m,
 * this shard's rows), λ (n), Lm⁻¹ and Lb⁻¹ (m×m, lower; the factorisations' inverses of K̃mm =
 * K(Z, Z) + 1e-3·I and B = K̃mm + KmnΛ⁻¹Knm) and K̃mm (m×m, lower).  Any pointer may be NULL.
 * (DESIGN §9 feeds them one at a time into the oracle's gradient to find which one carries the
 * GPU's extra rounding.) */
int gps_fitc_intermediates(gps_ctx* ctx, double* Knm, double* lam, double* Lm_inv, double* Lb_inv,
                           double* Kmm);

/* ---- block-LOO objectives -----------------------------
 * nfold-fold (the scripts use 4) block leave-out predictive from the diagonal blocks of
 * A⁻¹: fold f = rows [int(f·n/k), int((f+1)·n/k)) (KF:496-499), m_f = y_f − P_f⁻¹α_f,
 * C_f = P_f⁻¹, P_f = (A⁻¹)_ff.  GPS_BLOCK_DSS: Σ_f dss(m_f, C_f, y_f) (KF:487-543,
 * K20:523-587, dss KF:103-108); GPS_BLOCK_KC: Σ_f crps(m_f, diag C_f, y_f) (K20:655-720);
 * GPS_BLOCK_ES: Σ_f ES(m_f, C_f, y_f) (KF:607-663, ES KF:70-101; gps_full_blockloo_es).
 * value = the sum over folds, fold_values (nfold, may be NULL) the per-fold terms. */
enum { GPS_BLOCK_DSS = 0, GPS_BLOCK_KC = 1, GPS_BLOCK_ES = 2 };
/* Full GP, DSS or KC; grad (2 + n_ell, may be NULL) = the `.backward()` at KF:543 in the
 * reference's parameterisation.  Leaves the factor for gps_full_predict. */
int gps_full_blockloo(gps_ctx* ctx, int kind, const double* theta, int n_ell, int nfold,
                      int objective, double* value, double* grad, double* fold_values);
/* Full GP, energy score with num_sim draws per fold (300 at KF:652-655) and exponent beta
 * (1 at KF:70).  draws (2·num_sim·n doubles) hold, fold after fold, ξ_f then ξ'_f
 * (num_sim × b_f, row-major): the two torch.randn(num_sim, shape1) calls of ES (KF:79-80) in
 * the scripts' order.  C_f^½ (an SVD at KF:74-77) is the coupled Newton–Schulz iteration on
 * the MFMA GEMM.  grad as gps_full_blockloo (the `.backward()` at KF:663). */
int gps_full_blockloo_es(gps_ctx* ctx, int kind, const double* theta, int n_ell, int nfold,
                         int num_sim, double beta, const double* draws, double* value,
                         double* grad, double* fold_values);
/* FITC, DSS or KC; grad (2 + n_ell) and grad_z (m×d, row-major) may be NULL: the
 * `.backward()` at K20:587 / K20:720 w.r.t. theta and the inducing inputs, which the scripts
 * move too (K20:593, 726).  With a communicator the rows may be sharded: the nfold folds are
 * those of the GLOBAL rows ([⌊fN/k⌋, ⌊(f+1)N/k⌋), KF:496-499) and each must lie inside one
 * rank's rows (gpscore.dist.fold_shard_rows), else every rank returns -1; every rank gets the
 * global value, gradients and all nfold fold_values. */
int gps_fitc_blockloo(gps_ctx* ctx, const double* theta, int n_ell, int nfold, int objective,
                      double* value, double* grad, double* grad_z, double* fold_values);
/* ES(m, c, shape1, data_y, num_sim, beta) (KF:70-101) of one Gaussian N(m, C) (b×b,
 * row-major) at y with the draws given (ξ then ξ', num_sim × b each): the compat helper. */
int gps_energy_score(gps_ctx* ctx, const double* m, const double* C, int64_t b, const double* y,
                     int num_sim, double beta, const double* draws, double* out);

/* ---- joint test predictive -------------------------------------
 * The FULL predictive covariance of the resident test rows, which gps_*_predict reduces to its
 * diagonal: cal_mean_and_cov (KF:121-126) / spgp_cal_mean_and_cov (K20:76-83) as they return it,
 * observation noise included:
 *   full GP  Sigma = sigma²I + K** − K*f A⁻¹ Kf*          = sigma²I + K** − VᵀV,  V = L⁻¹Kf*
 *   FITC     Sigma = sigma²I + K** − V₁ᵀV₁ + V₂ᵀV₂,  V₁ = Lm⁻¹Km*, V₂ = Lb⁻¹Km*
 * and on it the paper's multivariate scores of held-out data — dss(mean_term, cov_term, num_va,
 * va_y) (KF:556-563, dss KF:103-108) and ES(mean_term, cov_term, num_va, va_y) (KF:677-684, ES
 * KF:70-101), which the scripts carry commented out — and joint draws mu + xi·L_Sigmaᵀ (as SD:174
 * draws its data).  All need a fit and a test set resident, as gps_*_predict; a block is rows
 * [r0, r1) with 0 <= r0 < r1 <= nt and at most 16384 rows (its V buffer at most 8 GiB).  They leave
 * the fit, the test-side buffers of gps_*_predict and the FITC test pre-pass untouched: a
 * gps_*_predict after them returns what it returned before, bitwise.  A context with a
 * communicator is refused (-1): sharded joint scores are not implemented.  Sigma not positive
 * definite: info > 0. */
/* mu (b = r1 − r0, may be NULL) and cov (b×b, row-major, ldc >= b, BOTH triangles, bitwise
 * symmetric) of rows [r0, r1) */
int gps_full_predict_cov(gps_ctx* ctx, int64_t r0, int64_t r1, double* mu, double* cov,
                         int64_t ldc);
int gps_fitc_predict_cov(gps_ctx* ctx, int64_t r0, int64_t r1, double* mu, double* cov,
                         int64_t ldc);
enum { GPS_JOINT_DSS = 0, GPS_JOINT_ES = 1 };
/* nblock contiguous blocks [⌊f·nt/k⌋, ⌊(f+1)·nt/k⌋) of the test rows (the KF:496-499 rule);
 * value = Σ_f score(N(mu_f, Sigma_f), yt_f), block_values (nblock, may be NULL) the terms.
 * GPS_JOINT_DSS: ½b·log2π + ½log|Sigma_f| + ½(yt_f − mu_f)ᵀSigma_f⁻¹(yt_f − mu_f) (KF:103-108).
 * GPS_JOINT_ES: num_sim, beta and draws (2·num_sim·nt doubles) as gps_full_blockloo_es — block f
 * holds ξ_f then ξ'_f, num_sim × b_f each; ignored for DSS (draws may be NULL).  nblock = 1 is the
 * scripts' commented validation score.  Needs the test targets (set_test with yt). */
int gps_full_predict_joint(gps_ctx* ctx, int nblock, int objective, int num_sim, double beta,
                           const double* draws, double* value, double* block_values);
int gps_fitc_predict_joint(gps_ctx* ctx, int nblock, int objective, int num_sim, double beta,
                           const double* draws, double* value, double* block_values);
/* out (nsamp × b, row-major) = mu + xi·L_Sigmaᵀ with xi (nsamp × b) the caller's N(0,1) draws and
 * L_Sigma the lower Cholesky factor of the rows' covariance */
int gps_full_predict_draws(gps_ctx* ctx, int64_t r0, int64_t r1, int nsamp, const double* xi,
                           double* out);
int gps_fitc_predict_draws(gps_ctx* ctx, int64_t r0, int64_t r1, int nsamp, const double* xi,
                           double* out);

/* ---- objective surfaces (contour-plot.R) ---------------
 * The objectives of CP.R:43-85 on a length-scale × noise grid, one small full GP per grid
 * point (CP.R uses n = 20 points and a 50 × 50 grid, CP.R:88-141): kernel
 * sf²·exp(−½‖x − x'‖²/ℓ²) with ℓ = ell[j] (CP.R:15-23, not a log) and noise s.d. s = noise_sd[i]
 * entering as s² (CP.R:45).  out (4 · n_noise · n_ell, row-major [objective][i][j], R's
 * matrix(…, nrow = 50) orientation): GPS_SURF_LOO_CRPS (cal_m_crps CP.R:43-53),
 * GPS_SURF_INSAMPLE_CRPS (wrong_cal_m_crps CP.R:55-64), GPS_SURF_NLML (cal_NLML CP.R:68-73),
 * GPS_SURF_LOO_LOGS (cal_m_logs CP.R:75-85).  flags GPS_SURF_LOGS_ADD_NOISE: the LOO-LogS
 * variance is 1/d + s² as CP.R:81 writes it; without it 1/d (the KF:416-424 form).  A grid
 * point whose matrix is not positive definite gets NaN objectives.  n > 128: each grid point
 * is one resident fit (the gps_full_fit path) and X, y become the context's full-GP data, as
 * after gps_full_set_data (no fit is left in place). */
enum { GPS_SURF_LOO_CRPS = 0, GPS_SURF_INSAMPLE_CRPS = 1, GPS_SURF_NLML = 2, GPS_SURF_LOO_LOGS = 3,
       GPS_N_SURF = 4 };
enum { GPS_SURF_LOGS_ADD_NOISE = 1 };
int gps_full_surface(gps_ctx* ctx, const double* X, const double* y, int64_t n, int d,
                     double log_sf2, const double* ell, int64_t n_ell, const double* noise_sd,
                     int64_t n_noise, int flags, double* out);

/* ---- batches of small full GPs ----------------------------------
 * nprob independent full GPs of one shape (n <= 128 training points, d <= 16 inputs, n_ell = 1 or
 * d, one kind and objective), each with its own data and θ, one workgroup per problem in one
 * launch — the replicate loops of "SIMPLE-DATA FULL-comapre.py" (TT = 100 data sets of n = 120,
 * three SGD fits each, SD:192-231 / 277-301 / 372-396) and contour-plot.R's n = 20.  Arrays are
 * problem-major: X nprob·n·d, y nprob·n, theta nprob·(2 + n_ell).  Both return 0 when the batch
 * ran, even if some problems failed: info[q] > 0 is the order of the leading minor of problem q
 * that is not positive definite (a non-finite θ ends there too) and that problem's outputs are
 * NaN; every other problem is untouched by it.  Results are bitwise independent of nprob and of a
 * problem's position in the batch.  The resident full-GP / FITC data, any fit and the test
 * buffers are left as they are (a gps_full_predict afterwards returns what it returned before),
 * and a communicator does not matter: nothing is sharded. */
/* Value and gradient (as gps_full_grad) of every problem at its own θ: obj (nprob·GPS_N_OBJ, may
 * be NULL), grad (nprob·(2 + n_ell)), info (nprob). */
int gps_full_grad_batch(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* theta, int n_ell,
                        double* obj, double* grad, int* info);
/* itr plain SGD steps θ ← θ − lr·grad (KF:254-260) from theta0 on the device, then one forward at
 * the final kernel parameters: values[q][i] (nprob·itr, may be NULL) is the objective before
 * step i, thetas[q][i] (nprob·itr·(2 + n_ell), may be NULL) θ after it — the series GP.train
 * returns — theta_out the final θ, obj (nprob·GPS_N_OBJ, may be NULL) the final objectives.  Xt
 * (nprob·nt·d; NULL or nt = 0: no predictive) gives mu / var (nprob·nt each, may be NULL) =
 * k*·α and σ² + sf² − ‖L⁻¹k*‖², and with yt (nprob·nt; NULL: no scores) sc (nprob·GPS_N_SC, may be
 * NULL) against the problem's own train-target mean and unbiased variance (KF:276-292).  flags
 * GPS_BATCH_STALE_NOISE: the final pass uses the σ² of the last step's forward (θ0's with itr =
 * 0) instead of the final one — the scripts' module-global sigma_noise_sq.  A
 * problem whose factorisation fails stops there: steps_done[q] says how many steps it completed,
 * its remaining series entries and final outputs are NaN, theta_out[q] is the θ it stopped at. */
enum { GPS_BATCH_STALE_NOISE = 1 };
int gps_full_train_batch(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                         const double* y, int64_t n, int d, const double* theta0, int n_ell,
                         int64_t itr, double lr, const double* Xt, const double* yt, int64_t nt,
                         int flags, double* theta_out, double* values, double* thetas, double* obj,
                         double* mu, double* var, double* sc, int* info, int* steps_done);

/* ---- batches of small FITC GPs -----------------------------------
 * The FITC sibling of the calls above: nprob independent FITC GPs of one shape (n <= 128 training
 * points, m <= 32 inducing inputs — m > n is legal —, d <= 16 inputs, n_ell = 1 or d, the ARD
 * kernel, jitter 1e-3 inside K(Z,Z) as K20:32-39), each with its own data, θ and inducing inputs,
 * one workgroup per problem — the replicate loops of "SIMPLE-FITC--comapre.py" (TT = 100 data sets
 * of n = 120 with m = 5, three SGD fits each that move the inducing inputs too, SF:189-237 /
 * 301-343 / 420-463).  Arrays are problem-major: X nprob·n·d, y nprob·n, Z and grad_z nprob·m·d,
 * theta nprob·(2 + n_ell).  Both return 0 when the batch ran, even if some problems failed:
 * info[q] is 0, k in 1..m (the leading minor of order k of K(Z,Z) + 1e-3·I is not positive, a NaN
 * included) or m + k (the same for B = K(Z,Z) + 1e-3·I + KᵀΛ⁻¹K); a failed problem's outputs are
 * NaN and every other problem is untouched by it.  Results are bitwise independent of nprob, of a
 * problem's position in the batch and of how the steps are split over launches.  The resident
 * data, any fit and the test buffers are left as they are; a communicator does not matter. */
/* Value and gradient (as gps_fitc_grad) of every problem at its own (θ, Z): obj
 * (nprob·GPS_N_OBJ, may be NULL), grad (nprob·(2 + n_ell)), grad_z (nprob·m·d), info (nprob). */
int gps_fitc_grad_batch(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* Z, int m,
                        const double* theta, int n_ell, double* obj, double* grad, double* grad_z,
                        int* info);
/* itr SGD steps θ ← θ − lr·grad, Z ← Z − lr_z·grad_z (SF:229-233) from (theta0, Z0) on the device,
 * then one forward at the final θ and Z: values / thetas / theta_out / obj / flags as
 * gps_full_train_batch, z_out (nprob·m·d) the final inducing inputs.  Xt gives mu = k*·c and var
 * = σ² + sf² − ‖Lm⁻¹k*‖² + ‖Lb⁻¹k*‖², yt the six scores.  A problem whose factorisation fails
 * stops there: steps_done[q] says how many steps it completed, its remaining series entries and
 * final outputs are NaN, theta_out[q] / z_out[q] are where it stopped. */
int gps_fitc_train_batch(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                         const double* y, int64_t n, int d, const double* Z0, int m,
                         const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                         const double* Xt, const double* yt, int64_t nt, int flags,
                         double* theta_out, double* z_out, double* values, double* thetas,
                         double* obj, double* mu, double* var, double* sc, int* info,
                         int* steps_done);

/* ---- batches of tall FITC GPs -------------------------------------
 * gps_fitc_grad_batch / gps_fitc_train_batch for 1 <= n <= 2048 training points: the same argument
 * lists, model (m <= 32, d <= 16, n_ell = 1 or d, ARD, jitter 1e-3), outputs, info codes, failure
 * semantics and bitwise independence of nprob, position and launch split — the replicate loops of
 * "KIN40K-COMPARE-ALL-FITC-20" (n = 500, d = 8, m = 20; LOO-CRPS 2000, NLML 3000, LOO-LogS 3000
 * steps).  One workgroup per problem as there, with V, U and the n-vectors in a per-problem
 * device workspace of the call's own instead of LDS; a launch runs max(1, 64 / ceil(n / 128))
 * steps.  They agree with the small-batch calls within rounding, never bitwise; for n <= 128 the
 * small-batch calls are the faster route.  A batch whose inputs, outputs or workspace
 * (nprob·(2n(m|1) + 9n) doubles) exceed 8 GiB is refused. */
int gps_fitc_grad_tall(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                       const double* y, int64_t n, int d, const double* Z, int m,
                       const double* theta, int n_ell, double* obj, double* grad, double* grad_z,
                       int* info);
int gps_fitc_train_tall(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* Z0, int m,
                        const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                        const double* Xt, const double* yt, int64_t nt, int flags,
                        double* theta_out, double* z_out, double* values, double* thetas,
                        double* obj, double* mu, double* var, double* sc, int* info,
                        int* steps_done);

/* ---- batches of full GPs of up to 512 rows ---------------------------
 * gps_full_grad_batch / gps_full_train_batch for 1 <= n <= 512 training
 * points: the same argument lists, model (d <= 16, n_ell = 1 or d, GPS_ARD or GPS_RBF; NLML,
 * LOO-CRPS, LOO-LogS), outputs (which may be NULL included), GPS_BATCH_STALE_NOISE, info codes,
 * failure semantics and bitwise independence of nprob, position and launch split — the replicate
 * loop of "kin40k-FULL-compare.py" (n = 500, d = 8; LOO-CRPS 400, NLML 400, LOO-LogS 500 steps).
 * One workgroup per problem as there; the n×n arrays sit in a per-problem device workspace of the
 * call's own (two np×np arrays, np = 64·ceil(n/64)) instead of LDS, and the O(n³) work runs tile by
 * tile on the FP64 matrix instruction; a launch runs min(64, max(1, 1024 / ceil(n/64)³)) steps.
 * They agree with the small-batch calls and the resident path within rounding, never bitwise; for
 * n <= 128 the small-batch calls are the faster route.  A batch whose inputs, outputs or workspace
 * (nprob·2np² doubles) exceed 8 GiB is refused. */
int gps_full_grad_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                       const double* y, int64_t n, int d, const double* theta, int n_ell,
                       double* obj, double* grad, int* info);
int gps_full_train_tall(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                        const double* y, int64_t n, int d, const double* theta0, int n_ell,
                        int64_t itr, double lr, const double* Xt, const double* yt, int64_t nt,
                        int flags, double* theta_out, double* values, double* thetas, double* obj,
                        double* mu, double* var, double* sc, int* info, int* steps_done);

/* ---- batches of full GPs of up to 512 rows on the block-LOO objectives ----------
 * gps_full_grad_tall / gps_full_train_tall with the objective GPS_BLOCK_DSS or GPS_BLOCK_KC over
 * nfold folds [int(f·n/nfold), int((f+1)·n/nfold)) (gps_full_blockloo's objectives and folds: the
 * 4-fold DSS fit of "kin40k-FULL-compare.py", KF:487-601, 150 steps at lr 1e-3, and its CRPS
 * sibling K20:655-720) for a whole batch: the same model, limits (1 <= n <= 512, d <= 16, n_ell =
 * 1 or d, GPS_ARD or GPS_RBF), SGD loop, final pass, outputs (which may be NULL included),
 * GPS_BATCH_STALE_NOISE, failure semantics and bitwise independence of nprob, position and launch
 * split.  2 <= nfold <= 32 and nfold <= n; GPS_BLOCK_ES is refused (it needs draws and a matrix
 * square root: gps_full_blockloo_es).  The value + gradient call returns value[q], the objective
 * of problem q, fold_values[q·nfold + f], fold f's term of it (may be NULL), obj, the five
 * GPS_OBJ_* entries at θ (may be NULL), and grad as gps_full_grad_tall; the training call's
 * values[q·itr + i] is the block objective before step i.  info[q] is 0, k in 1..n (the leading
 * minor of order k of A = K + σ²I is not positive definite, as everywhere) or n + k: the pivot of
 * global row k (1-based) of its fold's block P_f = (A⁻¹)_ff is not > 0 — an internal error, since a
 * positive definite A has positive definite P_f; the problem's outputs are NaN either way.  One
 * workgroup per problem; the per-problem workspace is np² + max(np², 2·bp²) + np² doubles (np =
 * 64·ceil(n/64), bp = 64·ceil(ceil(n/nfold)/64)), and a batch whose inputs, outputs or workspace
 * exceed 8 GiB is refused; a launch runs min(64, max(1, 1024 / ceil(n/64)³)) steps.  They agree
 * with gps_full_blockloo within rounding, never bitwise. */
int gps_full_blockloo_grad_tall(gps_ctx* ctx, int kind, int objective, int nfold, int64_t nprob,
                                const double* X, const double* y, int64_t n, int d,
                                const double* theta, int n_ell, double* value,
                                double* fold_values, double* obj, double* grad, int* info);
int gps_full_blockloo_train_tall(gps_ctx* ctx, int kind, int objective, int nfold, int64_t nprob,
                                 const double* X, const double* y, int64_t n, int d,
                                 const double* theta0, int n_ell, int64_t itr, double lr,
                                 const double* Xt, const double* yt, int64_t nt, int flags,
                                 double* theta_out, double* values, double* thetas, double* obj,
                                 double* mu, double* var, double* sc, int* info, int* steps_done);

/* ---- the same fits with a validation set scored step by step -----------------------
 * gps_full_train_tall and gps_full_blockloo_train_tall with every problem's own validation rows Xv
 * (nprob·nv·d) and targets yv (nprob·nv) scored INSIDE the fit: the per-iteration validation
 * series the scripts carry commented out (KF:441-449, 557-563, 678-684; K20:258-264, 469-476),
 * from the factorisation the step has in hand.  Everything up to steps_done means what it means
 * there, and the fit itself — theta_out, values, thetas, obj, mu, var, sc, info, steps_done — is
 * bitwise what those calls return.  Checkpoints: training step i (0-based) with i % va_every == 0
 * writes the six GPS_SC_* scores of the predictive at Xv against yv (and the problem's own
 * train-target mean and unbiased variance) to va_sc[(q·nva + i / va_every)·GPS_N_SC + ·], at the
 * parameters of that step's forward: θ before step i with its own σ², the model values[q·itr + i]
 * describes.  The final pass adds the last row, nva − 1 with nva = ceil(itr / va_every) + 1, at
 * the final pass's parameters, so it honours GPS_BATCH_STALE_NOISE: with that flag and itr = k it
 * is the scripts' va_series[k − 1] — the kernel parameters after update k − 1 with the σ² of
 * forward k − 1 (KF:239 against KF:441-449); without it, the score at the final θ.  Each row is
 * bitwise the sc of an itr = 0 call of the plain entry point at that θ with Xt = Xv, yt = yv, and
 * is independent of nprob, position and launch split.  A failed problem keeps the rows it reached
 * and gets NaN in every later row, the final row included.  Xv, yv and va_sc (nprob·nva·GPS_N_SC)
 * are required; 1 <= nv <= 2^24, 1 <= va_every <= 2^20; the 8 GiB guard counts Xv, yv and va_sc.
 * The LDS and the workspace are those of the plain calls; a checkpoint costs about n²·nv flops. */
int gps_full_train_tall_va(gps_ctx* ctx, int kind, int objective, int64_t nprob, const double* X,
                           const double* y, int64_t n, int d, const double* theta0, int n_ell,
                           int64_t itr, double lr, const double* Xv, const double* yv, int64_t nv,
                           int64_t va_every, const double* Xt, const double* yt, int64_t nt,
                           int flags, double* theta_out, double* values, double* thetas,
                           double* obj, double* mu, double* var, double* sc, double* va_sc,
                           int* info, int* steps_done);
int gps_full_blockloo_train_tall_va(gps_ctx* ctx, int kind, int objective, int nfold,
                                    int64_t nprob, const double* X, const double* y, int64_t n,
                                    int d, const double* theta0, int n_ell, int64_t itr, double lr,
                                    const double* Xv, const double* yv, int64_t nv,
                                    int64_t va_every, const double* Xt, const double* yt,
                                    int64_t nt, int flags, double* theta_out, double* values,
                                    double* thetas, double* obj, double* mu, double* var,
                                    double* sc, double* va_sc, int* info, int* steps_done);

/* ---- batches of full GPs of up to 512 rows on the block-LOO energy score --------
 * gps_full_blockloo_es (KF:607-663) and the SGD fit around it (KF:665-732: 25 steps at lr 0.1,
 * 300 draws a fold, redrawn every step) for a whole batch: the model, limits (1 <= n <= 512, d <=
 * 16, n_ell = 1 or d, GPS_ARD or GPS_RBF, 2 <= nfold <= min(n, 32)), SGD loop, final pass,
 * outputs (which may be NULL included), GPS_BATCH_STALE_NOISE and failure semantics of
 * gps_full_blockloo_*_tall, and further ceil(n / nfold) <= 128 (a fold is at most two tiles on a
 * side: its O(b³) square-root work has to fit one launch), 2 <= num_sim <= 512, 0 < beta <= 2.
 * draws holds nprob × draw_sets × 2·num_sim·n doubles, every set in gps_full_blockloo_es's layout
 * (per fold [a, a + b): ξ then ξ', num_sim × b each, at 2·num_sim·a); the value + gradient call
 * reads one set a problem, training step i reads set i mod draw_sets, 1 <= draw_sets <= max(itr,
 * 1): draw_sets = itr is the scripts' fresh draws every step, draw_sets = 1 common random numbers.
 * A step is three launches — per problem, per (problem, fold), per problem — and one step runs per
 * launch sequence; results are bitwise independent of nprob, the problem's position and how itr
 * is split over calls chained through θ.  info[q] is 0, k in 1..n, n + k (as
 * gps_full_blockloo_*_tall) or 2n + 1 + f: fold f's Newton–Schulz schedule would need more than
 * 40 steps (σ² below ~1e-24 of ‖Π_f‖∞).  The per-problem workspace is 3·np² + 2·np + 72 +
 * nfold·(11·bp² + 6·Sp·bp + Sp²) doubles (np, bp as above, Sp = 64·ceil((num_sim + 1)/64)); a
 * batch whose inputs (the draws included), outputs or workspace exceed 8 GiB is refused: fewer
 * draw_sets or a smaller batch are the ways out.  They agree with gps_full_blockloo_es within
 * rounding, never bitwise. */
int gps_full_es_grad_tall(gps_ctx* ctx, int kind, int nfold, int num_sim, double beta,
                          int64_t nprob, const double* X, const double* y, int64_t n, int d,
                          const double* theta, int n_ell, const double* draws, double* value,
                          double* fold_values, double* obj, double* grad, int* info);
int gps_full_es_train_tall(gps_ctx* ctx, int kind, int nfold, int num_sim, double beta,
                           int64_t nprob, const double* X, const double* y, int64_t n, int d,
                           const double* theta0, int n_ell, int64_t itr, double lr,
                           const double* Xt, const double* yt, int64_t nt, int flags,
                           const double* draws, int64_t draw_sets, double* theta_out,
                           double* values, double* thetas, double* obj, double* mu, double* var,
                           double* sc, int* info, int* steps_done);

/* ---- batches of tall FITC GPs on the block-LOO objectives ----------------------
 * gps_fitc_grad_tall / gps_fitc_train_tall with the objective GPS_BLOCK_DSS or GPS_BLOCK_KC over
 * nfold folds [int(f·n/nfold), int((f+1)·n/nfold)) (gps_fitc_blockloo's objectives and folds: the
 * 4-fold DSS and KC fits of "KIN40K-COMPARE-ALL-FITC-20", K20:523-593 and K20:655-726, 3000 steps
 * each) for a whole batch: the same model, limits (1 <= n <= 2048, m <= 32, d <= 16, n_ell = 1 or
 * d, ARD, jitter 1e-3), SGD loop on θ and Z, final pass, outputs, GPS_BATCH_STALE_NOISE, failure
 * semantics and bitwise independence of nprob, position and launch split.  2 <= nfold <= 32 and
 * nfold <= n; GPS_BLOCK_ES is refused (it needs draws and a matrix square root, and FITC has no
 * energy-score path).  The value + gradient call returns value[q], the objective of problem q,
 * fold_values[q·nfold + f], fold f's term of it (may be NULL), obj, the five GPS_OBJ_* entries at
 * (θ, Z) (may be NULL), and grad / grad_z as gps_fitc_grad_tall; the training call's
 * values[q·itr + i] is the block objective before step i.  info[q] is 0, k in 1..m or m + k as
 * gps_fitc_grad_tall, or (2 + f)·m + k: the leading minor of order k of fold f's B₋f = K(Z,Z) +
 * 1e-3·I + Σ_{g≠f} K_gᵀΛ_g⁻¹K_g is not > 0 — an internal error, since B₋f is K̃mm plus positive
 * semidefinite terms; the problem's outputs are NaN either way.  One workgroup per problem; the
 * per-problem workspace is 4n(m|1) + (nfold + 1)·m(m|1) + 11n doubles, and a batch whose inputs,
 * outputs or workspace exceed 8 GiB is refused; a launch runs max(1, 32 / ceil(n / 128)) steps.
 * They agree with gps_fitc_blockloo within rounding, never bitwise. */
int gps_fitc_blockloo_grad_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                const double* X, const double* y, int64_t n, int d,
                                const double* Z, int m, const double* theta, int n_ell,
                                double* value, double* fold_values, double* obj, double* grad,
                                double* grad_z, int* info);
int gps_fitc_blockloo_train_tall(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                 const double* X, const double* y, int64_t n, int d,
                                 const double* Z0, int m, const double* theta0, int n_ell,
                                 int64_t itr, double lr, double lr_z, const double* Xt,
                                 const double* yt, int64_t nt, int flags, double* theta_out,
                                 double* z_out, double* values, double* thetas, double* obj,
                                 double* mu, double* var, double* sc, int* info, int* steps_done);

/* ---- the tall FITC fits with a validation set scored step by step -----------------
 * gps_fitc_train_tall and gps_fitc_blockloo_train_tall with every problem's own validation rows Xv
 * (nprob·nv·d) and targets yv (nprob·nv) scored INSIDE the fit: K20's commented-out validation
 * series (K20:258-264, 469-476, 737-743), from Lm⁻¹, Lb⁻¹ and c as the step's forward left them.
 * The argument lists are the plain calls' with Xv, yv, nv, va_every in front of Xt and va_sc, va_z
 * in front of info; everything else means what it means there, and the fit itself — theta_out,
 * z_out, values, thetas, obj, mu, var, sc, info, steps_done — is bitwise what those calls return.
 * Checkpoints, the final row (nva − 1, nva = ceil(itr / va_every) + 1, honouring
 * GPS_BATCH_STALE_NOISE), the failure rule (a failed problem keeps the rows it reached, NaN in
 * every later row, the final row included; on the block path a fit that fails in its fold work
 * after a good forward keeps that step's row) and the refusals (1 <= nv <= 2^24, 1 <= va_every <=
 * 2^20, Xv, yv and va_sc required) are those of gps_full_train_tall_va above; a row's parameters
 * are θ AND Z before step i with that step's own σ².  va_sc holds nprob·nva·GPS_N_SC doubles.
 * va_z (nprob·nva·m·d, may be NULL: no Z is kept) receives the Z of every row — the SGD steps move
 * Z, and the series of θ alone does not name a row's model; its last row is z_out.  Each row of
 * va_sc is bitwise the sc of an itr = 0 call of the plain entry point at that row's θ and Z with
 * Xt = Xv, yt = yv, and is independent of nprob, position and launch split.  The 8 GiB guard counts
 * Xv, yv, va_sc and va_z.  LDS and workspace are the plain calls'; a launch runs at most the plain
 * rule's steps and at most max(1, floor(4096 / nv)·va_every): its checkpoints stream at most 4096
 * validation rows (or one checkpoint's), about nv·m² FMAs a checkpoint. */
int gps_fitc_train_tall_va(gps_ctx* ctx, int objective, int64_t nprob, const double* X,
                           const double* y, int64_t n, int d, const double* Z0, int m,
                           const double* theta0, int n_ell, int64_t itr, double lr, double lr_z,
                           const double* Xv, const double* yv, int64_t nv, int64_t va_every,
                           const double* Xt, const double* yt, int64_t nt, int flags,
                           double* theta_out, double* z_out, double* values, double* thetas,
                           double* obj, double* mu, double* var, double* sc, double* va_sc,
                           double* va_z, int* info, int* steps_done);
int gps_fitc_blockloo_train_tall_va(gps_ctx* ctx, int objective, int nfold, int64_t nprob,
                                    const double* X, const double* y, int64_t n, int d,
                                    const double* Z0, int m, const double* theta0, int n_ell,
                                    int64_t itr, double lr, double lr_z, const double* Xv,
                                    const double* yv, int64_t nv, int64_t va_every,
                                    const double* Xt, const double* yt, int64_t nt, int flags,
                                    double* theta_out, double* z_out, double* values,
                                    double* thetas, double* obj, double* mu, double* var,
                                    double* sc, double* va_sc, double* va_z, int* info,
                                    int* steps_done);

/* ---- multi-GPU (RCCL over xGMI) ------------------------------------------- */
int gps_comm_unique_id(char uid[128]);
int gps_comm_init(gps_ctx* ctx, int nranks, int rank, const char uid[128]);
/* In-process stand-in for the communicator: nranks contexts of ONE process (each driven by its
 * own host thread, e.g. several shards on one GPU) that pass the same `group` key meet at every
 * all-reduce of the FITC path, where their partials are summed on the host in rank order.
 * Same call sites and element counts as the RCCL path; used to test the row-sharded FITC
 * bookkeeping without a multi-GPU node.  A rank that waits > 60 s, or a member that leaves,
 * aborts the group: every member's current and later all-reduces then fail (call
 * gps_comm_init_local again, which joins a fresh group under the same key).  Two live
 * contexts may not hold the same rank of one group. */
int gps_comm_init_local(gps_ctx* ctx, int nranks, int rank, long long group);
/* What the context's communicator holds: *nranks and *rank as RCCL reports them
 * (ncclCommCount / ncclCommUserRank) for GPS_COMM_RCCL, the group's size and this context's rank
 * for GPS_COMM_LOCAL, 1 and 0 with GPS_COMM_NONE. */
enum { GPS_COMM_NONE = 0, GPS_COMM_RCCL = 1, GPS_COMM_LOCAL = 2 };
int gps_comm_info(gps_ctx* ctx, int* nranks, int* rank, int* kind);
/* Leaves either communicator. */
int gps_comm_destroy(gps_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* GPSCORE_H */
