/*
 * ldpc_amd.h -- C ABI of the MI355X-native batched LDPC decoder.
 *
 * Drop-in boundary for the `ldpc.exe` step of the DNA-storage pipeline of
 * sjpark0905/DNA-LDPC-codes.  The reference crosses a process boundary once
 * per codeword (ex_decoder/decoder.py:553-562 -> def_func.py:47-51 ->
 * `ldpc 0 0 0 7 200 1 <codeword> <soft> <pchk> 0 0 0 0`), re-parses the .pchk
 * each time and decodes one frame on one CPU thread.  This ABI replaces that
 * with: load the .pchk once, decode a whole batch of LLR vectors per call on
 * one or more GPUs.
 *
 * Plain C types only: pointers + sizes, caller-owned buffers.  The library
 * owns device memory and the graph; a graph is immutable after load and may
 * be shared by threads; every call is reentrant per handle (no globals beyond
 * the thread-local error string).  Errors are negative return codes plus
 * ldpc_last_error() -- never exit(), unlike the reference (rcode.cpp:61-79,
 * mod2sparse.cpp:513-514).
 *
 * Arithmetic contract: IEEE fp64, reference operation order, bit-exact hard
 * decisions / iteration counts with LDPC_dec/ldpc/dec.cpp.
 */
#ifndef LDPC_AMD_H
#define LDPC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_AMD_ABI_VERSION 3

/* error codes */
enum {
    LDPC_OK = 0,
    LDPC_ERR_ARG = -1,      /* bad argument */
    LDPC_ERR_IO = -2,       /* cannot open / read a file */
    LDPC_ERR_FORMAT = -3,   /* not a parity-check file / malformed */
    LDPC_ERR_DEVICE = -4,   /* HIP runtime error, no device, out of memory */
    LDPC_ERR_UNSUPPORTED = -5 /* graph shape outside the compiled kernels */
};

/* decoder algorithms (reference decoder_type, DNA_main.cpp:49, 1565-1594) */
enum {
    LDPC_ALGO_BP = 0,  /* sum-product, LR domain: Run_Belief_Propagation_Decoder dec.cpp:583 */
    LDPC_ALGO_MSA = 1, /* float min-sum: Run_MSA_Decoder_INF dec.cpp:1216 (ldpc argv decoder_type 20) */
    /* integer-message decoders of dec.cpp (not used by the DNA flow; LLR input):
     * QMSA -- quantized min-sum Run_MSA_Decoder dec.cpp:1174 with q-bit messages,
     *         quantizer step and offset beta (decoder_type 20/21 with g_precision > 0);
     *         zero-posterior ties use a seeded counter hash instead of MKL rand_int(2)
     * GALLAGER_* -- Run_Gallager_Decoder dec.cpp:699 type 0/1/2 (decoder_type 1/2/3)
     *         on the hard decision of the input (LLR < 0 -> -1, else +1) */
    LDPC_ALGO_QMSA = 2,
    LDPC_ALGO_GALLAGER_A = 3,
    LDPC_ALGO_GALLAGER_B1 = 4,
    LDPC_ALGO_GALLAGER_B2 = 5
};

/* posterior output kinds (ldpc_opts.post_kind) */
enum {
    LDPC_POST_LLR = 0,   /* BP: log(P), P = LR*prod(lr) with NaN->1; MSA: L (already an LLR) */
    LDPC_POST_RATIO = 1  /* BP only: the raw fp64 posterior likelihood ratio P (bit-exact checks) */
};

/* input kinds for device-resident decode */
enum {
    LDPC_IN_LLR = 0, /* ln(P0/P1); BP converts with exp() (on device: ocml exp) */
    LDPC_IN_LR = 1   /* P0/P1 (BP only) -- what the reference feeds its BP (DNA_main.cpp:1344) */
};

typedef struct ldpc_graph ldpc_graph;

/* Decode schedule.  The schedule changes only which
 * codewords share a launch and where messages live between the phases, never
 * a codeword's arithmetic: every schedule is bit-exact.  A zeroed struct (or
 * a NULL pointer) selects the defaults, which were chosen by same-process A/B
 * measurements on MI355X.  The library reads no environment variable to pick
 * a schedule. */
enum {
    LDPC_SCHED_NONTEMPORAL = 1 << 0,    /* grouped schedule (and compressed min-sum): nontemporal
                                           variable->check stream (default on) */
    LDPC_SCHED_CONTINUOUS = 1 << 3,     /* continuous batching: a finished codeword's lane is refilled with
                                           the next one (fp64 decoders on graphs whose column degrees are all
                                           <= 32, or (8,72)-regular; default on; needs hard / iters / valid
                                           outputs) */
    LDPC_SCHED_MSA_COMPRESSED = 1 << 4, /* min-sum check->variable messages as per-row records (min1, min2,
                                           NaN planes) + one 16-bit meta word per row and codeword
                                           ((8,72)-regular graphs with E < 2^18; default on) */
    LDPC_SCHED_RESIDENT = 1 << 5,       /* continuous BP / fp64 min-sum on (8,72)-regular graphs with N % 32 == 0
                                           or graphs with rows <= 96 and columns <= 32: a pool of pool_tiles tiles
                                           iterated
                                           in place, its state sized to the 256 MB Infinity Cache, the
                                           syndrome fused into the check kernel (default on when the lane
                                           pool is chosen by the engine or is at most 4 tiles) */
    LDPC_SCHED_SPLIT_SYNDROME = 1 << 6, /* (ldpc_engine_info only) continuous grouped schedule: syndrome
                                           spread over syn_blocks blocks per tile */
    LDPC_SCHED_HANDOVER = 1 << 7,       /* resident pool on (8,72)-regular graphs, BP / fp64 min-sum: a lane
                                           whose codeword enters its max_iter-th update claims its next
                                           codeword in that step; the variable kernel writes the finished
                                           outputs and initialises the new codeword in one launch, and the
                                           last syndrome (the valid flag) follows in the next check: max_iter
                                           instead of max_iter + 1 steps per codeword that does not converge
                                           (default on; off elsewhere) */
    LDPC_SCHED_FUSE_ROW_BLOCK = 1 << 8, /* resident pool on (8,72)-regular graphs, BP, var_cpw at its default:
                                           when one of the 8 row blocks of M / 8 rows holds every column
                                           exactly once, the variable kernel runs one workgroup per row of that
                                           block, keeps the block's variable->check messages in LDS and
                                           finishes the rows' check update itself; the check kernel skips
                                           those rows' messages (default on; off elsewhere) */
    LDPC_SCHED_FIRST_FROM_PRIOR = 1 << 12, /* single-fill BP decodes: the first check derives its messages
                                              from the prior instead of E stored copies (default on) */
    LDPC_SCHED_LR_TABLE = 1 << 13,      /* ldpc_decode, BP (host exp) and min-sum: LLR batches on a k * unit
                                           lattice cross PCIe as one byte each and are decoded as codes with the
                                           table k * unit (BP: its host exp), as ldpc_engine_decode_codes
                                           (default on; off = fp64 input: host exp / copy of every value) */
    LDPC_SCHED_DEBUG_NO_DRAIN = 1 << 14, /* tests only: the host ignores a drained pool, so a decode runs
                                           into its step bound and returns LDPC_ERR_DEVICE (default off) */
    LDPC_SCHED_DEBUG_BAD_LANE = 1 << 15 /* tests only (continuous schedules): the lane that claims codeword 0
                                           records an out-of-range index instead; the kernels' bounds checks
                                           skip its output stores and input reads and the decode returns
                                           LDPC_ERR_DEVICE (default off) */
};

typedef struct ldpc_schedule {
    int32_t flags_set;   /* LDPC_SCHED_* bits whose value is taken from `flags`; the others keep the default */
    int32_t flags;
    int32_t group_tiles; /* grouped schedule: 64-codeword tiles per check/variable launch
                            (0 = default: 3, 8 for compressed min-sum; < 0 = the whole pass) */
    int32_t var_cpw;     /* columns per variable-phase wavefront: 1, 2, 4 or 8 (3: compressed min-sum only;
                            0 = default: 2 for coded input in the resident pool or the compressed
                            min-sum, else 4) */
    int32_t pool_tiles;  /* resident pool tiles when the engine chooses the pool (0 = default: 3 for the
                            (8,72)-regular kernels, else as many as fit ~226 MB of messages + priors) */
    int32_t poll_every;  /* resident pool: steps between occupancy polls (0 = default 8) */
    int32_t syn_blocks;  /* continuous grouped schedule: syndrome blocks per tile (0 = default 32) */
    int32_t reserved;    /* 0 */
} ldpc_schedule;

typedef struct ldpc_opts {
    int32_t n_devices;      /* <= 0: use device 0 only; at most 64 (else LDPC_ERR_ARG) */
    const int32_t *devices; /* device ordinals >= 0 (NULL: 0..n_devices-1) */
    int64_t chunk;          /* lane pool: codewords resident per device at once (0: auto --
                               all of a shard of <= 1024, else the engine's own pool);
                               codewords cross PCIe in double-buffered chunks of
                               max(4096, chunk) that overlap the decode */
    int32_t exp_on_host;    /* BP: compute LR = exp(LLR) with the host libm, exactly as
                               DNA_main.cpp:1344 does (default 1 when opts == NULL) */
    int32_t post_kind;      /* LDPC_POST_* */
    int32_t host_threads;   /* threads for host exp/packing (0: auto; clamped to 256) */
    int32_t msa_precision;  /* LDPC_ALGO_QMSA: message bits q, 2..16 (Set_MSA dec.cpp:1683) */
    int32_t msa_offset;     /* LDPC_ALGO_QMSA: offset beta (1 = offset min-sum, decoder_type 21) */
    int32_t reserved0;
    double msa_step;        /* LDPC_ALGO_QMSA: quantizer step (g_step_length), > 0 */
    uint64_t tie_seed;      /* LDPC_ALGO_QMSA: seed of the zero-posterior tie hash */
    const ldpc_schedule *schedule; /* NULL: the default schedule (ABI version 2) */
} ldpc_opts;

/* ------------------------------------------------------------------------ */
/* Graph                                                                     */
/* ------------------------------------------------------------------------ */

/* Largest M or N a graph may have (every constructor below returns
 * LDPC_ERR_UNSUPPORTED above it).  The reference allocates whatever a file's
 * header asks for (mod2sparse_allocate via mod2sparse_read,
 * mod2sparse.cpp:381-400); a 12-byte .pchk could otherwise make the host
 * allocate and clear 16 GB of row/column pointers. */
#define LDPC_MAX_DIM (1 << 26)

/* Load a Radford-Neal .pchk file.  Replaces read_pchk (rcode.cpp:54-85) +
 * mod2sparse_read (mod2sparse.cpp:381-427): same magic ('P'<<8)+0x80, same
 * record stream, same row/column ordering and duplicate rule
 * (mod2sparse_insert, mod2sparse.cpp:502-604).  *err gets LDPC_OK or a code. */
ldpc_graph *ldpc_graph_load(const char *pchk_path, int *err);

/* Build a graph from (row, col) pairs (0-based).  Same ordering/dedup rules. */
ldpc_graph *ldpc_graph_from_edges(int32_t M, int32_t N, const int32_t *rows, const int32_t *cols,
                                  int64_t n_edges, int *err);

/* Load an alist file with the rules of the reference's alist-to-pchk
 * (alist-to-pchk.cpp:36-160); transpose != 0 is its -t option. */
ldpc_graph *ldpc_graph_load_alist(const char *alist_path, int32_t transpose, int *err);

/* Write the graph as a .pchk (intio_write magic + mod2sparse_write,
 * mod2sparse.cpp:338-376) or as an alist file. */
int ldpc_graph_save_pchk(const ldpc_graph *g, const char *pchk_path);
int ldpc_graph_save_alist(const ldpc_graph *g, const char *alist_path);

/* Build the RS-based LDPC code of RS_LDPC.c (RS LDPC encode/RS_LDPC/
 * RS_LDPC.c:221-431): q = 2^s (2 <= s <= 10), M = gamma*q, N = rho*q,
 * 3 <= rho <= q, 1 <= gamma <= q.  Optional outputs: gen_poly[rho-1]
 * (generator polynomial exponents, -1 = zero) and coset[q*q] (coset number
 * of every RS codeword, -1 = none) -- the tables its H_pri = 0 mode prints.
 * The DNA code's decode_n18432_m2048_final.pchk is (8, 72, 8) with its
 * columns permuted (tests/golden/rs_8_72_8_colperm.npz). */
ldpc_graph *ldpc_graph_rs_ldpc(int32_t s, int32_t rho, int32_t gamma, int32_t *gen_poly,
                               int32_t *coset, int *err);

void ldpc_graph_free(ldpc_graph *g);

/* Dimensions and degrees (CheckRegular, dec.cpp:138-189). */
int ldpc_graph_info(const ldpc_graph *g, int32_t *M, int32_t *N, int64_t *E, int32_t *dv_max,
                    int32_t *regular_dv, int32_t *dc_max, int32_t *regular_dc);

/* Block structure of array codes (RS-LDPC, quasi-cyclic): H is row_blocks x
 * col_blocks permutation matrices of size Q, rows in contiguous blocks.  Q = 0
 * when H has no such structure (regular degrees, M = dv * Q, N = dc * Q).
 * col_block[N] (may be NULL) receives each column's block.  The column blocks
 * are found as contiguous runs of Q columns or, for RS-LDPC codes with
 * permuted columns (the DNA code), by matching the column row sets against
 * ldpc_graph_rs_ldpc(log2 Q, col_blocks, row_blocks).  Code-structure tooling;
 * the decoders do not depend on it. */
int ldpc_graph_blocks(const ldpc_graph *g, int32_t *Q, int32_t *row_blocks, int32_t *col_blocks,
                      int32_t *col_block);

/* Copy out the CSR/CSC edge arrays (row_ptr[M+1], col_idx[E], col_ptr[N+1],
 * col_edge[E]); any pointer may be NULL. */
int ldpc_graph_edges(const ldpc_graph *g, int32_t *row_ptr, int32_t *col_idx, int32_t *col_ptr,
                     int32_t *col_edge);

/* Syndrome on the host: returns the number of unsatisfied checks for hard
 * bits dblk[N] (check.cpp:28-45); pchk[M] (may be NULL) receives parities. */
int ldpc_graph_syndrome(const ldpc_graph *g, const uint8_t *dblk, uint8_t *pchk);

/* ------------------------------------------------------------------------ */
/* Batched decode, host buffers (the in-process replacement of ldpc.exe)     */
/* ------------------------------------------------------------------------ */

/* Decode B codewords.  llr: [B][N] row-major fp64 channel LLRs ln(P0/P1) --
 * what soft*.txt holds (decoder.py:314, 528-535).  Outputs (caller-owned,
 * any of post/iters/valid may be NULL):
 *   hard_out [B][N] u8  -- the reference's dblk / dec_*.txt bits
 *   post_out [B][N] f64 -- per opts->post_kind
 *   iters_out[B]    i32 -- return value of Run_*_Decoder (dec.cpp:604, 1249)
 *   valid_out[B]    u8  -- *bIsCodeword (syndrome zero at exit)
 * Replaces LDPC_Decode (DNA_main.cpp:1565-1594) for decoder_type 0 / 20. */
int ldpc_decode(const ldpc_graph *g, const double *llr, int64_t B, int32_t max_iter, int32_t algo,
                uint8_t *hard_out, double *post_out, int32_t *iters_out, uint8_t *valid_out,
                const ldpc_opts *opts);

/* The same decode for a channel output held as small integers -- the DNA
 * pipeline's per-bit read-count differences k = count_0 - count_1, whose LLR
 * is k * ln((1-eps)/eps) (decoder.py:314) -- so no [B][N] fp64 matrix is
 * built, scanned or sent: codes [B][N] int8 (host), table[256] the channel
 * value of code k at table[k + 128], of kind table_kind (LDPC_IN_LLR; for BP
 * also LDPC_IN_LR).  BP's LR is the host libm exp of an LLR table entry, as
 * DNA_main.cpp:1344 computes it per bit.  Identical results to ldpc_decode on
 * llr[b][j] = table[codes[b][j] + 128] (LDPC_IN_LLR); one byte per bit
 * crosses PCIe.  Outputs and opts as ldpc_decode. */
int ldpc_decode_codes(const ldpc_graph *g, const int8_t *codes, const double *table, int32_t table_kind,
                      int64_t B, int32_t max_iter, int32_t algo, uint8_t *hard_out, double *post_out,
                      int32_t *iters_out, uint8_t *valid_out, const ldpc_opts *opts);

/* ------------------------------------------------------------------------ */
/* Device-resident engine (benchmarks, pipelines that keep data in HBM)      */
/* ------------------------------------------------------------------------ */
typedef struct ldpc_engine ldpc_engine;

/* One engine = one device + one HIP stream + chunk-sized message buffers,
 * with the default schedule.  An engine serves one thread at a time (its
 * calls enqueue on its one stream); engines on one graph may run in
 * different threads at once. */
ldpc_engine *ldpc_engine_create(const ldpc_graph *g, int32_t device, int32_t algo, int64_t chunk, int *err);

/* Same with an explicit schedule (NULL = defaults). */
ldpc_engine *ldpc_engine_create_ex(const ldpc_graph *g, int32_t device, int32_t algo, int64_t chunk,
                                   const ldpc_schedule *schedule, int *err);
void ldpc_engine_free(ldpc_engine *e);

/* Decode B codewords whose input already lives in device memory (d_in:
 * [B][N] fp64, kind LDPC_IN_*).  Device outputs (NULL to skip): d_hard
 * [B][N] u8, d_post [B][N] f64 (post_kind), d_iters [B] i32, d_valid [B] u8.
 * Asynchronous on the engine's stream; ldpc_engine_sync() waits. */
int ldpc_engine_decode(ldpc_engine *e, const double *d_in, int32_t in_kind, int64_t B, int32_t max_iter,
                       uint8_t *d_hard, double *d_post, int32_t post_kind, int32_t *d_iters, uint8_t *d_valid);

/* The same decode for channel outputs given as small integers -- the DNA
 * pipeline's per-bit count differences k, whose LLR is k * ln((1-eps)/eps)
 * (decoder.py:314), or a BSC's +-1: d_codes [B][N] int8 on the device and
 * table[256] (host) the channel value of code k at table[k + 128], of kind
 * table_kind (LDPC_IN_LLR; LDPC_IN_LR for BP only).  BP takes LR = the host
 * libm exp of an LLR table entry, as DNA_main.cpp:1344 does per bit.  The
 * result equals ldpc_engine_decode on the fp64 input table[code + 128]
 * bit for bit; the continuous schedules keep each codeword's prior as its
 * one-byte code instead of an fp64 value. */
int ldpc_engine_decode_codes(ldpc_engine *e, const int8_t *d_codes, const double *table, int32_t table_kind,
                             int64_t B, int32_t max_iter, uint8_t *d_hard, double *d_post, int32_t post_kind,
                             int32_t *d_iters, uint8_t *d_valid);

int ldpc_engine_sync(ldpc_engine *e);

/* The engine's HIP stream (hipStream_t as void*). */
void *ldpc_engine_stream(ldpc_engine *e);

/* Synthetic BSC channel on device: for codeword
 * index b in [b0, b0+B) and bit j, the transmitted bit is
 * codewords[(b mod n_cw)][j] (d_codewords: [n_cw][N] u8 on device), flipped
 * when hash(seed, b, j) < p; output value = +-llr_mag (LDPC_IN_LLR) or
 * +-exp(+-llr_mag) with host-computed exp (LDPC_IN_LR), written to d_out
 * [B][N] fp64. */
int ldpc_engine_gen_bsc(ldpc_engine *e, double *d_out, int32_t out_kind, int64_t b0, int64_t B,
                        const uint8_t *d_codewords, int32_t n_cw, uint64_t seed, double p, double llr_mag);

/* The same channel as codes for ldpc_engine_decode_codes: d_out [B][N] int8,
 * +1 where the received bit is 0 and -1 where it is 1 (table[129] = llr_mag,
 * table[127] = -llr_mag gives ldpc_engine_gen_bsc's LLRs). */
int ldpc_engine_gen_bsc_codes(ldpc_engine *e, int8_t *d_out, int64_t b0, int64_t B, const uint8_t *d_codewords,
                              int32_t n_cw, uint64_t seed, double p);

/* Kernel timing: HIP events on the engine stream around every stride-th
 * launch of each kernel class (stride 1 = every launch, 0 = off).  Enabling
 * resets the counters; read them after ldpc_engine_sync(). */
typedef struct ldpc_kernel_stats {
    int64_t launches[6];    /* [0]=check [1]=variable [2]=syndrome [3]=init [4]=finalize [5]=other */
    int64_t sampled[6];     /* launches that carried events */
    double ms[6];           /* summed device time of the sampled launches */
} ldpc_kernel_stats;

int ldpc_engine_profile(ldpc_engine *e, int32_t stride);

/* Parameters of LDPC_ALGO_QMSA (ignored by the other algorithms); the
 * engine starts with q = 6, step = 0.5, beta = 0, seed = 0. */
int ldpc_engine_set_params(ldpc_engine *e, int32_t msa_precision, double msa_step, int32_t msa_offset,
                           uint64_t tie_seed);
/* The schedule an engine runs with: resident codewords per pass (the lane
 * pool in continuous mode), tiles per launch, and the LDPC_SCHED_* bits that
 * are in effect. */
int ldpc_engine_info(ldpc_engine *e, int64_t *cap, int64_t *group_tiles, int32_t *flags);
int ldpc_engine_stats(ldpc_engine *e, ldpc_kernel_stats *out);

/* Pinned (page-locked) host memory.  Host-buffer inputs that live in it cross
 * PCIe straight from the caller's array (ldpc_decode_codes: no staging
 * copy); any other host memory is staged through the library's own pinned
 * buffers. */
void *ldpc_host_alloc(size_t bytes);
int ldpc_host_free(void *p);

/* Device buffers for callers without their own HIP allocator (bench, tests). */
enum { LDPC_H2D = 0, LDPC_D2H = 1, LDPC_D2D = 2 };
void *ldpc_dev_malloc(int32_t device, size_t bytes);
int ldpc_dev_free(int32_t device, void *p);
int ldpc_dev_memcpy(int32_t device, void *dst, const void *src, size_t bytes, int32_t kind);

/* ------------------------------------------------------------------------ */
/* Systematic encoding (the write half of the codec)                         */
/* ------------------------------------------------------------------------ */
/* For a graph H (M x N) with r = rank over GF(2) and K = N - r:
 *   parity positions: scanning columns j = N-1, N-2, ..., 0, column j is a
 *     parity position iff it is linearly independent of the parity columns
 *     already chosen (the greedy basis in that order; r positions);
 *   information positions: the other K columns (zero columns and duplicates
 *     of later columns among them), message bit k at info_pos[k], ascending;
 *   codeword: the unique c with c[info_pos[k]] = m[k] and H c = 0 (redundant
 *     rows of H -- the DNA code has 188 -- are handled by construction).
 * The reference ships only the pieces of an encoder (LDPC_dec/ldpc
 * make_gen.cpp, enc.cpp: N - M message bits, dense / mixed branches commented
 * out); the DNA code's K = 16572 = N - rank is what its file names (m1860)
 * record.  Messages and codewords are row-major u8, one byte per bit:
 * msg [B][K], cw [B][N] (the layout of hard_out and of d_codewords below).
 * An encoder is immutable after create and may be shared by threads; it keeps
 * what it needs of the graph, which may be freed. */
typedef struct ldpc_encoder ldpc_encoder;

/* Host only (GF(2) elimination), no device call.  LDPC_ERR_UNSUPPORTED when
 * K = 0 or when the encoder's dense matrix (r x M bits) exceeds 2^31 bits. */
ldpc_encoder *ldpc_encoder_create(const ldpc_graph *g, int *err);
void ldpc_encoder_free(ldpc_encoder *e);

/* Dimensions and positions: info_pos[K], par_pos[rank], ascending (any
 * pointer may be NULL). */
int ldpc_encoder_info(const ldpc_encoder *e, int32_t *N, int32_t *K, int32_t *rank, int32_t *info_pos,
                      int32_t *par_pos);

/* Encode B messages on the CPU.  A message byte other than 0 or 1 is
 * LDPC_ERR_ARG. */
int ldpc_encode_host(const ldpc_encoder *e, const uint8_t *msg, int64_t B, uint8_t *cw_out);

/* The same on `device`, from and to host buffers (any B: the batch crosses
 * device memory in passes).  Message bytes are checked as in
 * ldpc_encode_host before any device call; B = 0 touches no device; without
 * a GPU the call returns LDPC_ERR_DEVICE (ldpc_encode_host still works). */
int ldpc_encode(const ldpc_encoder *e, const uint8_t *msg, int64_t B, uint8_t *cw_out, int32_t device);

/* The same for device buffers d_msg [B][K] -> d_cw [B][N] (bit 0 of each
 * message byte is used).  stream: a hipStream_t of `device` -- the call only
 * enqueues and the caller's stream orders it -- or NULL: the library's own
 * stream, and the call returns when the codewords are written.  The encoder
 * is uploaded once per device. */
int ldpc_encoder_encode_device(const ldpc_encoder *e, int32_t device, void *stream, const uint8_t *d_msg, int64_t B,
                               uint8_t *d_cw);

/* ------------------------------------------------------------------------ */
/* DNA soft-input construction (the step before the decoder)                 */
/* ------------------------------------------------------------------------ */
/* Per-strand LLRs from read candidates -- the arithmetic of decoder.py's
 * strand loop (ex_decoder/decoder.py:142-519; count rule :266-320,
 * :442-497).  The caller (ldpc_dna_plan below, or dna_llr.py) classifies
 * strand s into kind[s]:
 *   0 no LLRs, 1 count over its rows, 2 one short candidate, 3 alignment
 *   failed (count of the failed rows' last bases)
 * and lays the candidate rows of strand s at rows[row_ptr[s]..row_ptr[s+1])
 * (payload_nt bytes each, ASCII bases; for kinds 2 and 3 byte 0 of a row is
 * the candidate's last base) with per-row quality row_q.  Output, on the
 * host: llr[2*payload_nt][n_strands] (row i = soft file i+1, i.e. the
 * decoder's [codeword][bit] layout) and optionally int_mask of the same
 * shape (1 where the reference leaves an int 0, which str() prints as "0").
 * Runs on `device`. */
int ldpc_dna_llr(int32_t n_strands, const int32_t *kind, const int64_t *row_ptr, const uint8_t *rows,
                 const int32_t *row_q, int32_t payload_nt, double llr_unit, double *llr, uint8_t *int_mask,
                 int32_t device);

/* ldpc_dna_llr, plus each entry's count difference as an int8 code:
 * llr = codes * llr_unit exactly (decoder.py:297-314), codes
 * [2*payload_nt][n_strands].  *codes_exact = 1 when every |code| <= 127,
 * else 0 (the codes are then saturated and only llr is usable).  The codes
 * and the table k * llr_unit feed ldpc_decode_codes / the engine's coded
 * input without a host lattice pass over the fp64 matrix. */
int ldpc_dna_llr_codes(int32_t n_strands, const int32_t *kind, const int64_t *row_ptr, const uint8_t *rows,
                       const int32_t *row_q, int32_t payload_nt, double llr_unit, double *llr, uint8_t *int_mask,
                       int8_t *codes, int32_t *codes_exact, int32_t device);

/* Levenshtein distances of sequence pairs on `device`
 * (def_func.edit_dist, def_func.py:10-26).  Sequence i is
 * seqs[offsets[i] .. offsets[i]+lengths[i]); lengths <= 800. */
int ldpc_dna_edit_distance(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int64_t n_seqs,
                           const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int32_t *dist,
                           int32_t device);

/* The strand index code: every strand starts with a
 * 16-nt prefix, the 16-bit strand index and 16 parity bits as one word of the
 * systematic RS(8,4) code over GF(16) (primitive polynomial 19, generator
 * roots alpha^1..alpha^4, index symbols first; two bases per symbol,
 * A/C/G/T = 0..3, high pair first -- the format of original
 * files/final_DNA.txt).
 *
 * ldpc_dna_index_encode: prefix[n][16] ASCII for n index values, on the host;
 * an index outside 0..65535 is LDPC_ERR_ARG. */
int ldpc_dna_index_encode(const int32_t *index, int64_t n, uint8_t *prefix);

/* Decode the prefix of n raw reads (the reference's rs_dec.exe step,
 * decoder.py:59-92).  Read i is seqs[offsets[i] .. offsets[i]+lengths[i]), as
 * in ldpc_dna_edit_distance; only its first 16 bytes are used.  If a codeword
 * lies within two symbol errors of the prefix, cnumerr[i] is that number (0,
 * 1 or 2) and index[i] the corrected index; otherwise, and for a read shorter
 * than 16 or with a character other than A, C, G, T in the prefix, both are
 * -1.  The _host form runs on the CPU; the other passes the host buffers
 * through `device` (n = 0 does nothing and needs no device). */
int ldpc_dna_index_decode_host(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int64_t n,
                               int32_t *index, int32_t *cnumerr);
int ldpc_dna_index_decode(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int64_t n,
                          int32_t *index, int32_t *cnumerr, int32_t device);

/* The strands to synthesise: codewords [n_cw][N] u8 (n_cw even, >= 2; bit 0
 * of each byte is used) and index[N] (0..65535) -> out [N][16 + n_cw/2] ASCII
 * without separators: strand j = the prefix of index[j], then base k from
 * bits (2k, 2k+1) of column j (A/C/G/T = 00/01/10/11).  Host form and, with
 * host buffers, on `device`. */
int ldpc_dna_strands_host(const uint8_t *codewords, int32_t n_cw, int64_t N, const int32_t *index, uint8_t *out);
int ldpc_dna_strands(const uint8_t *codewords, int32_t n_cw, int64_t N, const int32_t *index, uint8_t *out,
                     int32_t device);

/* The aligner of ragged strands (the reference calls
 * MUSCLE, decoder.py:201-207): a deterministic centre-star multiple alignment
 * of every group of reads.  Sequence i is seqs[offsets[i] ..
 * offsets[i]+lengths[i]) (any bytes, any length); group g is sequences
 * group_ptr[g] .. group_ptr[g+1] (group_ptr[0] = 0, group_ptr[n_groups] =
 * n_seqs, at most 32768 reads per group).  Per group: the centre is the read
 * with the smallest sum of Levenshtein distances to the others (ties: lowest
 * index); every other read is aligned to it by the Levenshtein traceback that
 * prefers diagonal, then up (an insertion before the centre position), then
 * left (a '-' on the centre position); insertions of all rows share
 * left-justified, '-'-padded columns.
 *
 * Outputs: center[g] (index inside the group, -1 for an empty group),
 * width[g], out_ptr[n_groups+1] and the rows: row r of group g is the
 * width[g] bytes at out + out_ptr[g] + r * width[g], rows in input order.
 * *out_needed (may be NULL) gets out_ptr[n_groups], the bytes all rows take;
 * if out_capacity is smaller the call returns LDPC_ERR_ARG with center, width,
 * out_ptr, *out_needed and dist filled and no row written (out may be NULL
 * with out_capacity 0: the size query).  dist (may be NULL) gets, per
 * sequence, its Levenshtein distance to its group's centre.
 *
 * The _host form runs on one CPU thread.  ldpc_dna_star_align computes the
 * in-group distances and the pairwise tables and tracebacks on `device` and
 * merges on the host; the results are byte-identical.  workspace_bytes bounds
 * the device memory that holds the traceback moves of one kernel pass (0: 256
 * MiB); the pairs run in as many passes as that takes.  A group with a read
 * longer than 800 bytes, or with a pair whose moves (64 * m * ceil(n / 16) * 4
 * bytes for a read of m and a centre of n bytes) exceed workspace_bytes, is
 * aligned by the host code inside the call.  stats (may be NULL) gets
 * {groups of two or more reads aligned on the host, kernel passes, pairs
 * aligned on the device}.  Null pointers, negative counts, a group_ptr that is
 * not monotone from 0 to n_seqs, negative or overflowing offsets / lengths and
 * output sizes that overflow are LDPC_ERR_ARG, checked before any device call. */
int ldpc_dna_star_align_host(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int64_t n_seqs,
                             const int64_t *group_ptr, int64_t n_groups, int32_t *center, int32_t *width,
                             int64_t *out_ptr, uint8_t *out, int64_t out_capacity, int64_t *out_needed,
                             int32_t *dist);
int ldpc_dna_star_align(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int64_t n_seqs,
                        const int64_t *group_ptr, int64_t n_groups, int32_t *center, int32_t *width,
                        int64_t *out_ptr, uint8_t *out, int64_t out_capacity, int64_t *out_needed, int32_t *dist,
                        int32_t device, int64_t workspace_bytes, int64_t *stats);

/* The read planner (decoder.py:103-497, what
 * dna_llr.plan_llr does in Python): reads -> the kind / row_ptr / rows / row_q
 * plan that ldpc_dna_llr consumes.
 *
 * Inputs.  Read i is seqs[offsets[i] .. offsets[i]+lengths[i]) with quality
 * quals[i].  With index_vals[n_reads] a read is its payload and index_vals[i]
 * its decoded index.  With index_vals = NULL the reads are raw: the first 16
 * bytes go through the RS(8,4) decoder of ldpc_dna_index_decode, reads with
 * cnumerr -1 are dropped and the payload is the bytes from 16 on.
 * strands[n_strands] are the valid index values, strictly ascending; a read
 * whose index is not among them is dropped, the others are grouped per strand
 * in input order.  align: 1 = the centre-star aligner of ldpc_dna_star_align,
 * 0 = no aligner (a ragged strand with candidates is then LDPC_ERR_ARG).
 *
 * Per strand: no reads -> kind 0; one read -> kind 2 if shorter than
 * payload_nt, else 1; several reads all exactly payload_nt long -> kind 1;
 * otherwise the strand is ragged: the Levenshtein distance of every pair
 * i < k of its reads is taken, the candidates are the reads with a partner at
 * distance < 15 (the reference's constant), in input order; none -> kind 0;
 * otherwise the candidates are aligned as one group: aligned width ==
 * payload_nt -> kind 1 with the aligned rows, any other width -> kind 3, each
 * row holding the last byte of its aligned row in byte 0.
 *
 * Outputs.  kind[n_strands], row_ptr[n_strands + 1], and R = row_ptr[n_strands]
 * rows of payload_nt bytes prefilled with '-': a plain kind-1 strand has each
 * read's first payload_nt bytes, kind 2 the read's last byte in byte 0 ('-'
 * for an empty read; an empty read with quality > 63 is LDPC_ERR_ARG naming
 * the strand); row_q[r] is the quality of row r's read.  R <= n_reads, so the
 * caller allocates rows[max(n_reads, 1)][payload_nt] and row_q[max(n_reads,
 * 1)]; rows from R on are not touched.  stats (may be NULL), int64[9]:
 *   [0] reads valid after both filters     [1] distance pairs
 *   [2] ragged strands sent to the aligner [3] read-to-centre alignments
 *   [4] R                                  [5..8] reads with cnumerr -1, 0, 1, 2
 *                                                 (all 0 with index_vals)
 * Null pointers, negative counts, payload_nt < 1, strands not strictly
 * ascending and negative or overflowing offsets / lengths are LDPC_ERR_ARG,
 * checked before any device call; n_reads = 0 gives all kinds 0.
 *
 * ldpc_dna_plan_host runs on one CPU thread and has no limit on read length.
 * ldpc_dna_plan runs the grouping, classification, pair enumeration, distances,
 * candidate selection and row layout as kernels on `device` and gives the same
 * bytes; the aligner is ldpc_dna_star_align's (workspace_bytes as there, 0 =
 * its default), whose merge is host code.  It inherits the distance kernel's
 * limit: a ragged strand holding a read longer than 800 bytes is LDPC_ERR_ARG
 * naming the read. */
int ldpc_dna_plan_host(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, const int32_t *quals,
                       int64_t n_reads, const int32_t *index_vals, const int32_t *strands, int32_t n_strands,
                       int32_t payload_nt, int32_t align, int32_t *kind, int64_t *row_ptr, uint8_t *rows,
                       int32_t *row_q, int64_t *stats);
int ldpc_dna_plan(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, const int32_t *quals,
                  int64_t n_reads, const int32_t *index_vals, const int32_t *strands, int32_t n_strands,
                  int32_t payload_nt, int32_t align, int32_t device, int64_t workspace_bytes, int32_t *kind,
                  int64_t *row_ptr, uint8_t *rows, int32_t *row_q, int64_t *stats);

/* Raw reads in, decoder input out: ldpc_dna_plan followed by
 * ldpc_dna_llr_codes in one call, the plan never leaving the device.  Inputs
 * as ldpc_dna_plan; outputs as ldpc_dna_llr_codes: llr[2*payload_nt][n_strands],
 * int_mask (may be NULL), codes with *codes_exact (codes may be NULL), plus
 * kind[n_strands] (may be NULL) and stats (may be NULL).  The results equal
 * those of the two calls. */
int ldpc_dna_reads_llr(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, const int32_t *quals,
                       int64_t n_reads, const int32_t *index_vals, const int32_t *strands, int32_t n_strands,
                       int32_t payload_nt, int32_t align, int32_t device, int64_t workspace_bytes, double llr_unit,
                       double *llr, uint8_t *int_mask, int8_t *codes, int32_t *codes_exact, int32_t *kind,
                       int64_t *stats);

/* ------------------------------------------------------------------------ */
/* A whole DNA trial (decoder.py:541-664, what            */
/* dna_pipeline.decode_trial does in Python)                                  */
/* ------------------------------------------------------------------------ */
/* The decoder input of a trial is one int8 matrix codes [n_cw][N] of count
 * differences (ldpc_dna_llr_codes); row i's LLRs are table[codes + 128].
 *
 *   first decode   every row with table[k + 128] = k * unit, unit =
 *                  log((1 - eps) / eps); errors[i] = number of hard != truth;
 *                  fail_first = the rows with errors, 1-based, ascending;
 *                  re_decode[j] = rows with hard[i][j] != (codes[i][j] < 0);
 *                  erasure_index = the columns with re_decode > 140, computed
 *                  once, after the first decode
 *   second decode  eps2 = eps - 0.0005; while failures remain and eps2 > 0.001:
 *                  the failed rows are decoded from the same codes with
 *                  table[k + 128] = (k == 0) ? 0 : ((k * unit) * num) / den,
 *                  num = log((1 - eps2 + 0.0005) / (eps2 - 0.0005)), den = unit
 *                  (the reference's rescale of the LLRs, in its operation
 *                  order), then eps2 -= 0.0005; a row decoded without errors
 *                  replaces its row of hard.  faithful != 0 keeps the
 *                  reference's reset of the failure list per codeword
 *                  (decoder.py:659-661: only the last re-decoded row's outcome
 *                  survives an iteration), faithful = 0 tracks every failure
 *   genie-less     without the true codewords (codewords = NULL) a row fails
 *                  iff its valid flag (syndrome at exit) is 0; its error count
 *                  reads -1, and 0 for a row that did not fail
 *
 * ldpc_trial_result: counts, and caller-owned arrays any of which may be NULL.
 * fail_first / fail_second / first_errors / second_errors / iters / valid hold
 * n_cw entries (the lists' lengths are n_fail_first / n_fail_second;
 * second_errors is -2 for a row that was never re-decoded), erasure_index N
 * (n_erasure used), hard [n_cw][N] (the first decode's bits with the second
 * decode's replacements), iters / valid of the first decode, kind [n_strands]
 * and stats[9] as ldpc_dna_plan (ldpc_trial_run_reads only), codes_exact as
 * ldpc_dna_llr_codes.  t_llr_s / t_first_s / t_second_s: seconds the library
 * spent in the planner + code kernel, the first decode with its statistics,
 * and the second-decode loop. */
typedef struct ldpc_trial_result {
    int32_t n, first_success, second_success, second_iterations;
    int32_t n_fail_first, n_fail_second, n_erasure, codes_exact;
    int32_t *fail_first, *fail_second;
    int32_t *first_errors, *second_errors;
    int32_t *erasure_index;
    uint8_t *hard;
    int32_t *iters;
    uint8_t *valid;
    int32_t *kind;
    int64_t *stats;
    double t_llr_s, t_first_s, t_second_s;
} ldpc_trial_result;

/* The decoder of ldpc_dna_trial_host: decode B rows codes [B][N] as the LLRs
 * table[codes + 128] with max_iter iterations into hard [B][N] and valid [B]
 * (1 = zero syndrome at exit).  Nonzero return: the trial ends with it. */
typedef int (*ldpc_trial_decode_fn)(void *user, const int8_t *codes, const double *table, int64_t B,
                                    int32_t max_iter, uint8_t *hard, uint8_t *valid);

/* The trial's control flow on host buffers with the caller's decoder (the
 * library has no CPU decoder): codes [n_cw][N], codewords [n_cw][N] or NULL.
 * iters of *out is not written.  Null codes / decode / out, n_cw or N < 1,
 * eps outside (0.0015, 0.5) and max_iter < 0 are LDPC_ERR_ARG. */
int ldpc_dna_trial_host(const int8_t *codes, int32_t n_cw, int32_t N, const uint8_t *codewords,
                        ldpc_trial_decode_fn decode, void *user, double eps, int32_t max_iter, int32_t faithful,
                        ldpc_trial_result *out);

/* Speculated second decodes.  The engine maps one wave
 * to one (row, tile of 64 lanes), so a second decode of F rows costs what
 * 64 * ceil(F / 64) rows cost, and the decode of (row, eps2 step) depends on
 * nothing else.  With speculation on, one decoder call holds the failed rows
 * under several consecutive eps2 steps and the control flow is replayed over
 * its results; every field of ldpc_trial_result is what it is without.
 *
 *   steps   0 or 1: off, the decoder calls are exactly those above; n >= 2: at
 *           most n eps2 steps per call; -1: as many as fit; below -1 LDPC_ERR_ARG
 *   K       the largest |code| over the rows of fail_first (-128 counts 128);
 *           W = 2K + 1, P = 256 / W: P steps' tables fit side by side in the one
 *           256-entry table
 *   a call  for a list of F rows with rem steps left holds
 *           k = max(1, min(rem, P, 64 * ceil(F / 64) / F, steps if >= 2)) steps:
 *           only the tiles the batch occupies anyway are filled.  k = 1 is the
 *           plain decode.  For k >= 2 batch row j * F + f is list row f with
 *           K + j * W - 128 added to every code, and table[j * W + (c + K)] is
 *           step j's table entry of code c (0.0 in unused entries): the same
 *           doubles reach the decoder.
 *   replay  steps j = 0 .. k - 1 in order, each over the rows still failing,
 *           as the loop above; results past a row's last step are dropped
 *
 * ldpc_trial_counters: of the last run.  With speculation off second_decodes
 * == second_iterations, second_rows == second_rows_used, and K is not
 * computed: code_absmax and steps_per_decode read 0. */
typedef struct ldpc_trial_counters {
    int32_t second_decodes;   /* decoder calls of the eps2 loop */
    int32_t code_absmax;      /* K; 0 when the first decode left no failure */
    int32_t steps_per_decode; /* P */
    int32_t reserved;
    int64_t second_rows;      /* rows handed to those calls */
    int64_t second_rows_used; /* rows whose result the replay consumed */
} ldpc_trial_counters;

/* ldpc_dna_trial_host with `steps` as above; the callback sees k * F rows and
 * the packed table.  counters may be NULL. */
int ldpc_dna_trial_host_spec(const int8_t *codes, int32_t n_cw, int32_t N, const uint8_t *codewords,
                             ldpc_trial_decode_fn decode, void *user, double eps, int32_t max_iter,
                             int32_t faithful, ldpc_trial_result *out, int32_t steps, ldpc_trial_counters *counters);

/* The trial handle: one engine (algo LDPC_ALGO_BP or LDPC_ALGO_MSA, its lane
 * pool sized as ldpc_decode_codes sizes it for n_cw codewords), the true
 * codewords [n_cw][N] on `device` (NULL: genie-less), the device code matrix
 * and the buffers of both decodes, created once and reused by every run.  The
 * decoder input never leaves the device: per stage the host reads errors,
 * valid and re_decode, at the end the caller's optional hard / iters.  The
 * graph must outlive the handle; a handle serves one thread at a time.
 * Without a GPU, good arguments give LDPC_ERR_DEVICE; argument errors are
 * reported before any device call. */
typedef struct ldpc_trial ldpc_trial;
ldpc_trial *ldpc_trial_create(const ldpc_graph *g, int32_t device, int32_t algo, int32_t n_cw,
                              const uint8_t *codewords, const ldpc_schedule *schedule, int *err);
void ldpc_trial_free(ldpc_trial *t);

/* Raw reads to trial result: ldpc_dna_plan's planner (arguments as there),
 * the code kernel straight into the handle's code matrix, then the trial.
 * Needs 2 * payload_nt == n_cw and n_strands == N (else LDPC_ERR_ARG).  When
 * some count difference is outside int8 the codes cannot carry the input: the
 * call writes codes_exact = 0 (kind and stats are filled) and returns
 * LDPC_ERR_UNSUPPORTED; ldpc_dna_reads_llr and the fp64 decode remain. */
int ldpc_trial_run_reads(ldpc_trial *t, const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths,
                         const int32_t *quals, int64_t n_reads, const int32_t *index_vals, const int32_t *strands,
                         int32_t n_strands, int32_t payload_nt, int32_t align, int64_t workspace_bytes, double eps,
                         int32_t max_iter, int32_t faithful, ldpc_trial_result *out);

/* The trial of host codes [B][N], 1 <= B <= n_cw, against the first B true
 * codewords: one upload, then as above. */
int ldpc_trial_run_codes(ldpc_trial *t, const int8_t *codes, int64_t B, double eps, int32_t max_iter,
                         int32_t faithful, ldpc_trial_result *out);

/* The handle's code matrix after a run, rows [0, B) to host codes [B][N]
 * (tests: the code kernel against ldpc_dna_reads_llr's codes). */
int ldpc_trial_read_codes(ldpc_trial *t, int8_t *codes, int64_t B);

/* Speculated second decodes for every later run of the handle (`steps` as
 * for ldpc_dna_trial_host_spec; a new handle has 0).  A speculated batch holds
 * up to 64 * ceil(n_cw / 64) rows: the first call with steps on grows the
 * handle's batch buffers to that many.  The copies are made on the device
 * (one kernel reads a failed row once and writes its k shifted copies). */
int ldpc_trial_set_speculation(ldpc_trial *t, int32_t steps);

/* The counters of the handle's last run (zeros before the first). */
int ldpc_trial_get_counters(const ldpc_trial *t, ldpc_trial_counters *out);

/* --- the sequencing channel: strands to raw reads -----
 *
 * Strands [n_strands][strand_nt] over ACGT, 1 <= strand_nt <= 399, to the raw
 * reads [r0, r0 + n_reads) of seed `seed`, r0 + n_reads <= 2^40.  Every draw
 * is a counter hash, integers only:
 *   h(r, c, p) = splitmix64(((r << 24) | (c << 16) | p) ^ splitmix64(seed)),
 *   hi(x) = x >> 32, u(x) = x >> 11;
 *   strand of read r   (hi(h(r,0,0)) * n_strands) >> 32
 *   quality            q_val[i], i the largest index with q_lo[i] <= hi(h(r,1,0))
 *   slot p = 0..L      inserts iff u(h(r,2,p)) < t_ins, the base "ACGT"[(hi(h(r,3,p)) * 4) >> 32]
 *   base p = 0..L-1    e = u(h(r,4,p)): deleted iff e < t_del; substituted iff
 *                      t_del <= e < t_del + t_sub by "ACGT"[(b + 1 + ((hi(h(r,5,p)) * 3) >> 32)) & 3]
 *                      (b: the source base's position in ACGT); else copied
 *   read               for p = 0..L-1 slot p's insertion, then base p unless
 *                      deleted; slot L's insertion last: 0 .. 2L + 1 bytes
 * so a read depends on (seed, r) alone: [0, n1) is a prefix of [0, n2) and a
 * range split over two calls gives the same bytes.  Thresholds are
 * probabilities times 2^53, in [0, 2^53] with t_sub + t_del <= 2^53.  The
 * quality table has 1 <= nq <= 256 entries, q_lo ascending (equal neighbours
 * allowed) from q_lo[0] = 0: entry i is drawn with probability
 * (q_lo[i+1] - q_lo[i]) / 2^32.
 *
 * Outputs: read r - r0 starts at byte (r - r0) * ldpc_dna_sim_stride(strand_nt)
 * of `reads` (the stride is 2 * strand_nt + 1 rounded up to a multiple of 16;
 * 0 for a strand_nt outside 1..399); bytes of a slot beyond the read's length
 * are unspecified.  lengths / quals [n_reads]; strand_of [n_reads] may be NULL.
 * With offsets[i] = i * stride this is the planner's input.  Null pointers,
 * sizes and thresholds outside their ranges, a strand byte outside ACGT and a
 * descending q_lo are LDPC_ERR_ARG, reported before anything is written.
 * ldpc_dna_sim_reads_host runs on one CPU thread; ldpc_dna_sim_reads generates
 * in device memory (one wave per read) and copies down: the same bytes. */
int64_t ldpc_dna_sim_stride(int32_t strand_nt);
int ldpc_dna_sim_reads_host(const uint8_t *strands, int32_t n_strands, int32_t strand_nt, uint64_t seed, int64_t r0,
                            int64_t n_reads, int64_t t_sub, int64_t t_ins, int64_t t_del, const int32_t *q_val,
                            const uint32_t *q_lo, int32_t nq, uint8_t *reads, int32_t *lengths, int32_t *quals,
                            int32_t *strand_of);
int ldpc_dna_sim_reads(const uint8_t *strands, int32_t n_strands, int32_t strand_nt, uint64_t seed, int64_t r0,
                       int64_t n_reads, int64_t t_sub, int64_t t_ins, int64_t t_del, const int32_t *q_val,
                       const uint32_t *q_lo, int32_t nq, uint8_t *reads, int32_t *lengths, int32_t *quals,
                       int32_t *strand_of, int32_t device);

/* The strands a handle's simulated trials sample: uploaded once.  Needs
 * n_strands == N and 2 * (strand_nt - 16) == n_cw (else LDPC_ERR_ARG). */
int ldpc_trial_set_strands(ldpc_trial *t, const uint8_t *strands, int64_t n_strands, int32_t strand_nt);

/* Strands to trial result: the channel's reads [r0, r0 + n_reads) generated
 * into buffers the handle owns (grown on demand, reused), then
 * ldpc_trial_run_reads from its planner on with those reads as the source --
 * raw reads, payload_nt = strand_nt - 16, strand_index_vals [N] the planner's
 * `strands`.  No read crosses to the host but the candidates of ragged
 * strands, packed, for the aligner's merge.  t_llr_s covers generator +
 * planner + code kernel.  Without strands set: LDPC_ERR_ARG. */
int ldpc_trial_run_sim(ldpc_trial *t, uint64_t seed, int64_t r0, int64_t n_reads, int64_t t_sub, int64_t t_ins,
                       int64_t t_del, const int32_t *q_val, const uint32_t *q_lo, int32_t nq,
                       const int32_t *strand_index_vals, int32_t align, int64_t workspace_bytes, double eps,
                       int32_t max_iter, int32_t faithful, ldpc_trial_result *out);

/* Write soft<rs>_n18432_m1860_<i+1>.txt, i < n_files, into dir: row i of
 * llr as str(value)+' ' tokens (decoder.py:511-516, def_func.py:54-57);
 * int_mask (may be NULL) marks the int-0 entries.  Host only. */
int ldpc_write_soft_files(const char *dir, int32_t rs, const double *llr, const uint8_t *int_mask,
                          int32_t n_files, int32_t n_strands);

/* Python repr() of a double into out (NUL-terminated); returns its length. */
int ldpc_py_float_repr(double v, char *out, int32_t cap);

/* ------------------------------------------------------------------------ */
/* Error-rate simulation (the reference's                */
/* Run_Simulation / Check_End loop, DNA_main.cpp:756-914, and channel.cpp)    */
/* ------------------------------------------------------------------------ */
/* The channel: symmetric, memoryless, at most 255 outputs, given as data.
 * thr[254]: u64 thresholds, non-decreasing, each <= 2^53.  For frame b < 2^40
 * and bit j < 2^24 (so N < 2^24):
 *   u    = splitmix64(((b << 24) | j) ^ splitmix64(seed ^ 0x4348414e4e454c31)) >> 11
 *   k0   = -127 + #{i : u >= thr[i]}
 *   code = cw[b][j] ? -k0 : k0                    (int8, -127 .. 127)
 * and the channel value of a code is table[code + 128], as for
 * ldpc_decode_codes.  Integer compares only: the host form, the kernel and a
 * numpy replica give the same bytes, and a range of frames gives the same rows
 * however it is split.  The message of frame b is bit k = the low bit of
 * splitmix64(((b << 24) | k) ^ splitmix64(seed)), encoded systematically.
 *
 * ldpc_channel_codes_host: codes [B][N] of frames [b0, b0 + B) on one CPU
 * thread; cw [B][N] u8 (bit 0 is used) or NULL: the zero codeword.  A NULL or
 * non-monotone thr, a threshold above 2^53, N outside 1 .. 2^24 - 1, negative
 * b0 / B and frames past 2^40 are LDPC_ERR_ARG, before anything is written. */
int ldpc_channel_codes_host(const uint8_t *cw, int32_t N, int64_t b0, int64_t B, uint64_t seed, const uint64_t *thr,
                            int8_t *codes);

/* One frame's record.  bit_err: positions with hard != cw, over all N;
 * info_err: the same over the information positions; raw_err: positions where
 * the channel value read hard differs from cw, by the reference's rule
 * (DNA_main.cpp:1711-1748: an LLR >= 0, or a likelihood ratio >= 1, reads as
 * 0, anything else -- a NaN too -- as 1), over all N; erased: positions with
 * code == 0; iters / valid: the decoder's iteration count and *bIsCodeword. */
typedef struct ldpc_ber_record {
    int32_t bit_err, info_err, raw_err, erased, iters, valid;
} ldpc_ber_record;

/* The error counter on one CPU thread: records [B] from hard / codes [B][N],
 * cw [B][N] or NULL (zeros), info_mask [N] (1 at an information position) or
 * NULL (every position), the code table, and iters / valid [B] (NULL: 0). */
int ldpc_frame_errors_host(const uint8_t *hard, const uint8_t *cw, const int8_t *codes, int32_t N, int64_t B,
                           const uint8_t *info_mask, const double *table, int32_t table_kind, const int32_t *iters,
                           const uint8_t *valid, ldpc_ber_record *records);

/* The totals of a run.  frame_err: frames with bit_err > 0; undetected: those
 * among them the decoder called a codeword (DNA_main.cpp:871-874); detected:
 * frames with valid == 0; raw_frame_err: frames with raw_err > 0; iter_hist
 * (caller-owned, may be NULL; n_hist >= max_iter + 1 bins, else LDPC_ERR_ARG):
 * frames per iteration count.  A run resets every counter. */
typedef struct ldpc_ber_result {
    int64_t frames, bit_err, info_err, frame_err, undetected, detected;
    int64_t raw_bit_err, raw_frame_err, erased, iter_sum;
    int64_t *iter_hist;
    int32_t n_hist, reserved;
} ldpc_ber_result;

/* The stop rule of every run (Check_End, DNA_main.cpp:756-795).  Frames are
 * taken in index order from 0.  frames > 0: exactly that many.  frames == 0:
 * the run ends after the frame at which frame_err reaches target_frame_err
 * (>= 1), and after max_frames (>= 1) frames at the latest.  Batches run
 * whole; records past the cut are dropped, so the result does not depend on
 * the batch size.
 *
 * ldpc_ber_run_host: the loop on host buffers with the caller's decoder (the
 * library has no CPU decoder): decode frames [b0, b0 + B), codes [B][N] under
 * table, into hard [B][N], iters [B] (0 .. max_iter) and valid [B]; a nonzero
 * return ends the run with it.  enc: the messages above through
 * ldpc_encode_host, info_err over its info_pos; NULL: the zero codeword, and
 * info_err counts every position. */
typedef int (*ldpc_ber_decode_fn)(void *user, const int8_t *codes, const double *table, int32_t table_kind,
                                  int64_t b0, int64_t B, int32_t max_iter, uint8_t *hard, int32_t *iters,
                                  uint8_t *valid);
int ldpc_ber_run_host(int32_t N, const ldpc_encoder *enc, ldpc_ber_decode_fn decode, void *user, const uint64_t *thr,
                      const double *table, int32_t table_kind, uint64_t seed, int64_t batch, int32_t max_iter,
                      int64_t frames, int64_t target_frame_err, int64_t max_frames, ldpc_ber_result *result);

/* The device handle: one engine (any algo; its lane pool sized as
 * ldpc_decode_codes sizes it for `batch` codewords), the buffers of one batch
 * (messages, codewords, codes, hard bits, iters, valid, records) on `device`
 * and pinned host records, created once.  A batch never leaves the device:
 * message kernel -> ldpc_encoder_encode_device -> channel kernel ->
 * ldpc_engine_decode_codes -> error counter, all on the engine's stream; the
 * host reads 24 bytes per frame.  enc as for ldpc_ber_run_host.  The lane
 * pool is schedule->pool_tiles tiles of 64 codewords when that is set.  The
 * graph and the encoder must outlive the handle; a handle serves one thread
 * at a time.  1 <= batch <= 2^20.  Argument errors are reported before any
 * device call; without a GPU good arguments give LDPC_ERR_DEVICE. */
typedef struct ldpc_ber ldpc_ber;
ldpc_ber *ldpc_ber_create(const ldpc_graph *g, const ldpc_encoder *enc, int32_t device, int32_t algo,
                          const ldpc_schedule *schedule, int64_t batch, int *err);
void ldpc_ber_free(ldpc_ber *h);

/* ldpc_engine_set_params of the handle's engine (LDPC_ALGO_QMSA); the tie
 * hash of frame b keys on b itself. */
int ldpc_ber_set_params(ldpc_ber *h, int32_t msa_precision, double msa_step, int32_t msa_offset, uint64_t tie_seed);

/* Frames [b0, b0 + B) in batches: their records to records_out [B] (host).
 * What a caller that shards frames over devices needs. */
int ldpc_ber_run_range(ldpc_ber *h, const uint64_t *thr, const double *table, int32_t table_kind, uint64_t seed,
                       int64_t b0, int64_t B, int32_t max_iter, ldpc_ber_record *records_out);

/* The loop with the stop rule above, batches of the handle's size. */
int ldpc_ber_run(ldpc_ber *h, const uint64_t *thr, const double *table, int32_t table_kind, uint64_t seed,
                 int32_t max_iter, int64_t frames, int64_t target_frame_err, int64_t max_frames,
                 ldpc_ber_result *result);

/* Tests and tools.  ldpc_ber_read: rows [0, B) of the handle's last batch,
 * B <= batch, to host cw / hard [B][N] u8 and codes [B][N] int8 (any may be
 * NULL).  ldpc_ber_frame_errors: the error-counter kernel alone on host
 * arrays (as ldpc_frame_errors_host, the handle's information mask; cw /
 * iters / valid may be NULL: zeros), B <= batch.  ldpc_ber_profile /
 * ldpc_ber_stats: ldpc_engine_profile / ldpc_engine_stats of the handle's
 * engine; the three kernels of this section are launches of class "other". */
int ldpc_ber_read(ldpc_ber *h, int64_t B, uint8_t *cw, int8_t *codes, uint8_t *hard);
int ldpc_ber_frame_errors(ldpc_ber *h, const uint8_t *hard, const uint8_t *cw, const int8_t *codes,
                          const double *table, int32_t table_kind, const int32_t *iters, const uint8_t *valid,
                          int64_t B, ldpc_ber_record *records);
int ldpc_ber_profile(ldpc_ber *h, int32_t stride);
int ldpc_ber_stats(ldpc_ber *h, ldpc_kernel_stats *out);

/* ------------------------------------------------------------------------ */
/* misc                                                                      */
/* ------------------------------------------------------------------------ */
const char *ldpc_last_error(void); /* thread-local message for the last failing call */
int ldpc_device_count(void);
int ldpc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_AMD_H */
