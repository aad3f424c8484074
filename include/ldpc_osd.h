/*
 * ldpc_osd.h -- C ABI of libldpcosd.so: MI355X (gfx950) short-LDPC NMS + OSD decoder.
 *
 * This is the drop-in boundary for the reference's decoding hot path.  The reference
 * (lgw-frank/Short_LDPC_Decoding_OSD) has no FFI of its own -- its boundary is a Python
 * call surface -- so every entry point cites the reference function it replaces
 * (file:line relative to LDPC_128/ in the reference tree).  The Python mirror of that
 * surface lives in short_ldpc_decoding_osd_amd/ and binds these symbols with ctypes;
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C types only; `stream` is a hipStream_t passed as void* (NULL = default stream)
 *   - pointers named d_* are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); all other pointers are host memory
 *   - every call returns 0 on success or a negative LDPC_E_* code; ldpc_last_error()
 *     returns a thread-local message.  Nothing aborts or throws across the ABI.
 *   - device calls are asynchronous on `stream`; no allocation and no host sync happens
 *     inside a decode call (graph-capturable)
 *   - bit packing: bit v of a frame lives in word v/64, bit position v%64 (LSB first)
 */
#ifndef LDPC_OSD_H
#define LDPC_OSD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDPC_OSD_ABI_VERSION 5

enum {
    LDPC_OK = 0,
    LDPC_E_ARG = -1,         /* bad argument (null pointer, size, order ...)          */
    LDPC_E_IO = -2,          /* cannot read / parse a file                            */
    LDPC_E_CODE = -3,        /* H.G^T != 0, rank problems                             */
    LDPC_E_HIP = -4,         /* a HIP runtime call failed (message has the details)   */
    LDPC_E_UNSUPPORTED = -5, /* shape not handled by the kernels (e.g. OSD on n != 128) */
    LDPC_E_NOMEM = -6
};

/* OSD search algorithms for ldpc_osd_decode */
enum {
    LDPC_OSD_CONVENTIONAL = 0, /* FS_OSD/convention_osd.py:49-76  convention_osd_main */
    LDPC_OSD_FS = 1,           /* FS_OSD/fs_testing.py:129-161    fs_osd               */
    LDPC_OSD_PB = 2            /* PB_OSD/pb_testing.py:100-149    pb_osd               */
};

/* NMS kernel selection (0 = let the library choose) */
enum {
    LDPC_NMS_AUTO = 0,
    LDPC_NMS_GENERIC = 1, /* any code: one frame per wavefront, messages staged in LDS  */
    LDPC_NMS_QC16 = 2     /* 16x16-circulant codes of the CCSDS (128,64) shape: one frame
                             per 16-lane DPP row, messages in registers                  */
};

typedef struct ldpc_code ldpc_code; /* host-side code definition (H, G, Tanner graph) */
typedef struct ldpc_ctx ldpc_ctx;   /* per-device constants + scratch                  */

const char *ldpc_last_error(void);
int ldpc_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * Code definition (host, one-time).
 * Replaces Ldpc_128_testing/fill_matrix_info.py: Code.load_code :70-129 (alist -> H),
 * Code.gf2elim :7-42 and Code.generator_matrix :44-69 (systematic G, H.G^T = 0 check).
 * H may have redundant rows, as many as n or more: k = n - rank(H), and an H of rank n (no code) is LDPC_E_CODE.
 * ------------------------------------------------------------------------------------- */
int ldpc_code_from_alist(const char *path, ldpc_code **out);
int ldpc_code_from_dense(const int32_t *H /*[m][n] row-major 0/1*/, int32_t m, int32_t n, ldpc_code **out);
void ldpc_code_destroy(ldpc_code *code);
int ldpc_code_dims(const ldpc_code *code, int32_t *n, int32_t *m, int32_t *k, int32_t *max_chk_degree);
int ldpc_code_get_H(const ldpc_code *code, int32_t *H /*[m][n]*/);
int ldpc_code_get_G(const ldpc_code *code, int32_t *G /*[k][n]*/);

/* GF(2) Gauss-Jordan with the reference's pivot rule on one host matrix, in place.
 * Replaces full_gf2elim, PB_OSD/pb_testing.py:231-266 (used for code construction; the
 * per-frame eliminations of the OSD run on the device, see ldpc_osd_ge).
 * swaps: [n][2] pairs (j, col); *rows_out = rows left after deleting all-zero rows.     */
int ldpc_gf2elim_host(int32_t *M /*[m][n]*/, int32_t m, int32_t n, int32_t *swaps, int32_t *nswaps,
                      int32_t *rows_out);

/* Test-error-pattern table, FS_OSD/convention_osd.py:13-47 (generate_teps, query_boundary):
 * all supports of weight 0..order over k positions, each weight class in lexicographic
 * order stably re-sorted by descending index sum.  supports: [count][3] uint8, 0xFF padded
 * (NULL = only return the count).  boundaries: [order+1] cumulative counts (may be NULL).
 * Returns the number of patterns or a negative error.  order <= 3.                        */
int64_t ldpc_tep_table(int32_t k, int32_t order, uint8_t *supports, int64_t *boundaries);

/* FS-OSD visit order of one weight class, FS_OSD/fs_testing.py:32-49 (generate_sequential_teps):
 * lexicographic combinations of range(k) with the indicator vector reversed (support {k-1-p}).
 * supports: [C(k,weight)][3] uint8 ascending positions, 0xFF padded (NULL = only the count).   */
int64_t ldpc_tep_table_fs(int32_t k, int32_t weight, uint8_t *supports);

/* The code-only constants of ldpc_osdl_pb_search / _pb_decode for a code with 1 <= k <= 192 and 1 <= n-k <= 192, as
 * ldpc_ctx_create uploads them (host only): table[0..192] = P[Binomial(n-k, 1/2) <= b] by the float64 pmf recurrence (zero
 * beyond n-k), table[193..384] = (n-k-i) / (i+1), table[385..448] = (k-i) / (i+1), i < 64.  Returns the number of entries,
 * 449 (table may be NULL), or LDPC_E_ARG for another shape.                                            */
int64_t ldpc_osdl_pb_table(int32_t n, int32_t k, double *table);

/* CRC-32C of a host buffer: the record checksum of the TFRecord files the reference's stages
 * exchange (Ldpc_128_testing/data_generating.py:16-26, read_TFdata.py:18-29).                   */
uint32_t ldpc_crc32c(const void *data, uint64_t len);

/* ---------------------------------------------------------------------------------------
 * Device context: uploads the packed H/G, Tanner-graph tables and TEP tables of one code
 * to one GPU; one ctx per device.  The constants (and the event pool of ldpc_pipeline_run's
 * timing slots) are created here and never change afterwards.  The only state that decode calls
 * touch is scratch memory, and that is kept PER STREAM: a mutex-guarded map stream -> workspace
 * (front-end results of ldpc_osd_decode, PB-OSD frame lists and frontier areas), created on a
 * stream's first call and grown on demand.  Hence decode calls issued on DIFFERENT streams of one
 * context -- from one host thread or several -- may run concurrently, for every algorithm;
 * calls on the SAME stream are ordered by the stream.  ldpc_compact needs no scratch at all.
 * (ldpc_pipeline_timing slots are shared: concurrent pipelines must use different slots.)
 * Captured graphs: a hipGraph captured on a stream bakes in the addresses of THAT stream's workspace and
 * may later be launched on any stream.  The graph therefore owns the capture stream's workspace: do not
 * replay it concurrently with other work that uses the same workspace (eager calls on the capture stream,
 * a second replay of the same or of another graph captured on that stream); the library refuses to grow
 * (= move) a workspace once a capture has used it (LDPC_E_NOMEM: reserve enough before capturing), and
 * ldpc_osd_release_stream frees it when the graphs are gone or the stream is destroyed.
 * ------------------------------------------------------------------------------------- */
int ldpc_ctx_create(const ldpc_code *code, int32_t device, ldpc_ctx **out);
void ldpc_ctx_destroy(ldpc_ctx *ctx);
/* which NMS kernel LDPC_NMS_AUTO resolves to for this code (LDPC_NMS_GENERIC / _QC16) */
int ldpc_ctx_nms_kernel(const ldpc_ctx *ctx);

/* ---------------------------------------------------------------------------------------
 * Normalised min-sum BP, fixed T flooding iterations, no early stop.
 * Replaces Decoder_Layer.call / belief_propagation_op / compute_vc / compute_cv2 /
 * marginalize, Ldpc_128_testing/ms_test.py:99-242, and the hard decision + syndrome of
 * Decoding_model.get_eval :39,:45.
 *   d_llr     [B][n] f32 channel values (BPSK 0 -> +1, unscaled)
 *   alpha     host [T] effective check normalisers = softplus(stored weight) (:207-208);
 *             NMS-1 passes T copies of one value
 *   w_in/w_out effective bit weights of NMS-2/3 (:127-131, :222-225); 1.0f for NMS-1
 *   d_soft    [B][n] f32 posterior after iteration T (nullable)
 *   d_traj    [T][B][n] f32 posterior after iterations 1..T (nullable; the reference's
 *             soft_output_list without its slot 0, which is d_llr itself)
 *   d_hard    [B][ceil(n/64)] u64 packed hard decisions (soft > 0 ? 0 : 1) (nullable)
 *   d_fail    [B] u8, 1 = non-zero syndrome (nullable)
 * Each of the four outputs is switched off on its own; the others do not change.  With all four NULL the call still
 * succeeds (LDPC_OK): the kernel runs and writes nothing.  d_llr (B > 0) and alpha (T > 0) are required.
 * ------------------------------------------------------------------------------------- */
int ldpc_nms_decode(ldpc_ctx *ctx, const float *d_llr, int64_t B, int32_t T, const float *alpha, float w_in,
                    float w_out, float *d_soft, float *d_traj, uint64_t *d_hard, uint8_t *d_fail, int32_t kernel,
                    void *stream);

/* The trajectories of LISTED frames only, in the layout the reference buffers them: collect_failed_output_selective,
 * ms_test.py:55-64 (driven by Decoding_model.call :30-34 with the index of get_eval :51) -- T + 1 rows per failed
 * frame, row 0 the channel values (soft_output_list[0]), row t the posterior after iteration t.
 *   d_index / d_count  the frame list as ldpc_compact writes it; the number of frames is min(*d_count, F), read ON THE
 *                      DEVICE; F is the capacity of d_rows.  All of d_llr, d_index, d_count and d_rows are required
 *                      (F > 0); *d_count must be >= 0, as everywhere a count is read on the device (see the OSD section)
 *   d_rows             [F][T+1][n] f32
 * The frames are decoded again (same kernel, same arithmetic: every row equals the corresponding row of
 * ldpc_nms_decode's d_traj); nothing else is written.  At 2.5 dB a quarter of the frames fail: 1.4 KiB of rows per
 * input frame instead of the 5 KiB of a full [T][B][n] trajectory.                                                   */
int ldpc_nms_traj_rows(ldpc_ctx *ctx, const float *d_llr, const int32_t *d_index, const int32_t *d_count, int64_t F,
                       int32_t T, const float *alpha, float w_in, float w_out, float *d_rows, int32_t kernel, void *stream);

/* ---------------------------------------------------------------------------------------
 * NMS training step: loss and gradient of Decoding_model with respect to the EFFECTIVE factors, forward and backward
 * in one launch.  Replaces the training graph of Ldpc_128_training/ms_decoder_dense.py -- Decoder_Layer.call and the
 * unrolled loop :102-119, :232-241, compute_vc :121-134, compute_cv2 :177-208, marginalize :217-226,
 * calculation_loss :210-215 -- and the tape.gradient of training_block.
 *   L[f] = sum_{t=1..T} sum_v sigmoid_cross_entropy(logits = -soft_t[v], labels = bit[v])
 * The forward pass is ldpc_nms_decode's generic kernel, same device code and float order: d_traj / d_hard / d_fail
 * equal its outputs bit for bit, for either kernel of ldpc_nms_decode.  The gradient follows TensorFlow's rules for
 * the reference's ops (stop_gradient signs, top_k ties to the lower variable index, clip pass-through on [0, 1e30]);
 * they are not pinned against TensorFlow.  No gradient with respect to the channel values.
 *   d_llr         [B][n] f32 channel values, as ldpc_nms_decode
 *   d_label_bits  [B][ceil(n/64)] u64 packed code bits (the layout of ldpc_eval_counts)
 *   alpha         host [T] effective check normalisers; w_in / w_out as ldpc_nms_decode
 * Outputs, all nullable:
 *   d_loss        [B] f32 per-frame loss
 *   d_grad        [B][T+2] f32 per frame: dL/dalpha_0..T-1, dL/dw_in, dL/dw_out
 *   d_loss_sum    [1] f64, d_grad_sum [T+2] f64: the sums over the batch, a tree whose shape depends on B alone (no
 *                 atomics): repeated calls give the same bits on any stream
 *   d_traj / d_hard / d_fail  as ldpc_nms_decode
 * The backward pass keeps a tape of (n + (3 + 2 ceil(dc/32)) m) 4-B words per iteration next to the 4 (E + 2n) B of
 * messages of each frame in LDS: T <= 64, check degree dc <= 64, and one frame must fit LDPC_NMS_TRAIN_LDS_BUDGET bytes,
 * otherwise LDPC_E_UNSUPPORTED with the byte count (CCSDS (128,64): 3 KiB + 1.75 KiB per iteration, 115 KiB at T = 64).
 * ------------------------------------------------------------------------------------- */
#define LDPC_NMS_TRAIN_LDS_BUDGET (160u * 1024u)
int ldpc_nms_train_grad(ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label_bits, int64_t B, int32_t T,
                        const float *alpha, float w_in, float w_out, float *d_loss, float *d_grad, double *d_loss_sum,
                        double *d_grad_sum, float *d_traj, uint64_t *d_hard, uint8_t *d_fail, void *stream);

/* Error statistics, Decoding_model.get_eval, ms_test.py:36-54.
 * d_counts[5] += {frames, frames_in_error, bit_errors, undetected, syndrome_failures}.
 * The caller zeroes d_counts; d_fail may be NULL (then undetected/syndrome are not counted). */
int ldpc_eval_counts(ldpc_ctx *ctx, const uint64_t *d_hard, const uint64_t *d_label_bits, const uint8_t *d_fail,
                     int64_t B, int64_t *d_counts, void *stream);

/* Stream compaction of the failed-frame flags, the `tf.where(syndrome != 0)` of
 * ms_test.py:51: d_index[0..count) = ascending frame numbers with d_flag != 0.
 * d_index: [B] i32, d_count: [1] i32.                                                     */
int ldpc_compact(ldpc_ctx *ctx, const uint8_t *d_flag, int64_t B, int32_t *d_index, int32_t *d_count,
                 void *stream);

/* Bit (un)packing between the reference's one-integer-per-bit labels and packed words.
 * elem_size: bytes per element of d_bits (1 = u8, 4 = i32, 8 = i64).                      */
int ldpc_pack_bits(ldpc_ctx *ctx, const void *d_bits /*[B][n]*/, int32_t elem_size, int64_t B,
                   uint64_t *d_words /*[B][ceil(n/64)]*/, void *stream);
int ldpc_unpack_bits(ldpc_ctx *ctx, const uint64_t *d_words, int64_t B, void *d_bits, int32_t elem_size,
                     void *stream);

/* ---------------------------------------------------------------------------------------
 * Frame generator: random message . G, BPSK, AWGN or block Rayleigh fading, and the packed labels, in one launch.
 * Replaces Testing_data_gen_128/data_generating.py:13-51 and Training_data_gen_128/data_generating.py:41-81 on the
 * device.  Frame i of a call is a pure function of (seed, frame0 + i, sigma, mean, flags, fade_len) and of the code:
 * a set does not depend on how it is cut into calls, on the stream, or on the device count.
 *
 * The random stream (a contract: a change of any item below changes every frame).
 *   Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85,
 *   ten rounds.  Key = {seed low 32 bits, seed high 32 bits}; counter = {idx low, idx high, block, stream}; the four
 *   output words of a call are x0..x3.  Known answers (counter, key -> output):
 *     {0,0,0,0}, {0,0}                                             -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *     all ffffffff, all ffffffff                                   -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     {243f6a88,85a308d3,13198a2e,03707344}, {a4093822,299f31d0}   -> d16cfe09 94fdcceb 5001e420 24126ea1
 *   stream 0, message bits: idx = global frame number frame0 + i (64 bit); block b yields message bits 128 b .. 128 b + 127,
 *     word w of the block bits 32 w .., LSB first; bits at positions >= k are discarded.
 *   stream 1, noise: idx = global frame number; block b yields the normals of columns 4 b .. 4 b + 3 (columns >= n are
 *     discarded).  With ua(x) = float(x) 2^-32 + 2^-33 in f32, conversion and sum rounded to nearest, in (0, 1], and
 *     tb(x) = float(x >> 8) 2^-24, exact, in [0, 1):
 *       r = sqrtf(-2 logf(ua(x0))), z0 = r cospif(2 tb(x1)), z1 = r sinpif(2 tb(x1)); z2, z3 likewise from (x2, x3).
 *     |z| <= 6.77; ua = 1 gives radius 0, never an infinity.
 *   stream 2, fading amplitude: idx = fading-block number q = (frame n + column) / fade_len, an unsigned 64-bit division
 *     on the global sample index (taken modulo 2^64); block 0 only; a = sqrtf(-logf(ua(x0))), a Rayleigh amplitude with
 *     E[a^2] = 1 (in distribution the reference's |h| / sqrt(2), h complex normal, data_generating.py:30-37).  The
 *     fading blocks run on through frame boundaries and calls; there is no zero tail (the reference's h stays 0 past its
 *     last whole block).
 *   per sample: v = mean + sigma z (AWGN) or v = mean a + sigma z (Rayleigh), each product and sum rounded on its own
 *     (no FMA); y = bit ? -v : v, an exact negation.  The codeword is message . G mod 2 with the context's G.
 * The results of logf / sqrtf / sincospif are the device library's: a CPU restatement agrees to a few ULP, not bit for bit.
 *
 *   d_y           [B][n] f32 channel values (nullable)
 *   d_label_bits  [B][ceil(n/64)] u64 code bits, the layout of ldpc_pack_bits, pad bits zero (nullable)
 * Each output is switched off on its own; the other does not change.  B = 0 returns LDPC_OK without a launch.
 * With LDPC_GEN_F_ALL_ZEROS the labels are zero, stream 0 is not drawn and y = v: the values that the coded set negates.
 * LDPC_E_ARG: p NULL, B < 0, frame0 < 0, sigma negative or not finite, fade_len < 1 with LDPC_GEN_F_RAYLEIGH, unknown
 * flag bits.  One launch, no atomics, no workspace, nothing per stream: graph-capturable, and calls on different streams
 * of one context may run concurrently.
 * ------------------------------------------------------------------------------------- */
#define LDPC_GEN_F_ALL_ZEROS (1u << 0) /* ALL_ZEROS_CODEWORD_TESTING / _TRAINING of the reference's globalmap */
#define LDPC_GEN_F_RAYLEIGH  (1u << 1) /* Rayleigh_fading: block fading, fade_len samples per block          */

typedef struct ldpc_gen_params {
    uint64_t seed;      /* Philox key */
    int64_t  frame0;    /* global number of the batch's first frame, >= 0 */
    float    sigma;     /* noise standard deviation, >= 0 */
    float    mean;      /* channel mean (1.0f for test sets; the blended mean for training sets) */
    uint32_t flags;     /* LDPC_GEN_F_ALL_ZEROS | LDPC_GEN_F_RAYLEIGH */
    int32_t  fade_len;  /* samples per fading block, >= 1 (the reference's int(16 * duration)); read only with _RAYLEIGH */
} ldpc_gen_params;

int ldpc_gen_frames(ldpc_ctx *ctx, const ldpc_gen_params *p, int64_t B, float *d_y /*[B][n], nullable*/,
                    uint64_t *d_label_bits /*[B][ceil(n/64)], nullable*/, void *stream);

/* ---------------------------------------------------------------------------------------
 * OSD (n = 128, k = 64 codes).  Frames are addressed as d_y[ d_index ? d_index[f] : f ].
 * If d_count is non-NULL the number of frames is min(*d_count, F) read ON THE DEVICE (so a
 * compaction can feed the OSD without a host round trip); F is then the capacity: a count above F is truncated to F,
 * and nothing at or beyond frame min(*d_count, F) of any output is written.  *d_count must be >= 0 (ldpc_compact writes
 * nothing else); the kernels do not check for a negative count.
 * A NULL in a pointer that is not marked nullable is LDPC_E_ARG (the message names the entry point) before anything is
 * launched.
 * The entries of d_index are frame numbers of d_y and are NOT range-checked by default (the entry points do
 * not know how many frames d_y holds): a caller-made list must stay inside d_y; ldpc_compact /
 * ldpc_pipeline_run write only valid, ascending frame numbers.  Debug aid: ldpc_osd_params.y_frames.
 * ------------------------------------------------------------------------------------- */

/* Per-frame GF(2) elimination on the device: full_gf2elim, PB_OSD/pb_testing.py:231-266.
 * d_rows_in/out: [F][64][2] u64 (row r of frame f, columns 0..127); d_swaps: [F][64][2] u8
 * recorded (j, col) pairs; d_nswaps: [F] i32, the number of exchanges, or -1 for a rank-deficient
 * matrix (its reduced rows and exchange records are then unspecified: the kernel does not drop
 * all-zero rows as the host GE does).  d_rows_in and d_rows_out are required; d_swaps and
 * d_nswaps are nullable (each on its own).                                                    */
int ldpc_osd_ge(ldpc_ctx *ctx, const uint64_t *d_rows_in, int64_t F, uint64_t *d_rows_out, uint8_t *d_swaps,
                int32_t *d_nswaps, void *stream);

/* OSD front end: swapped_info + identify_mrb, PB_OSD/pb_testing.py:268-320
 * (reliability sort, column permutation of G, elimination, MRB/LRB bookkeeping).
 *   d_perm   [F][128] u8 : original bit index at primed position p (pi_1 o pi_2)
 *   d_parity [F][64] u64 : row r of P' in G' = [I | P']  (bit c = P'[r][c])
 *   d_nswaps [F] i32 (nullable)                                                            */
int ldpc_osd_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                   uint8_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream);

/* ldpc_osd_params.flags: routes that compute the same results as the default one (cross-checks and options).
 * Every call validates them before it launches anything (LDPC_E_ARG names the offending flag).
 *   flag                        algorithm     entry points        route
 *   LDPC_OSD_F_TABLE_SCAN       CONVENTIONAL  all                 the table-driven scan at order 2 (orders 0, 1, 3 take it anyway)
 *   LDPC_OSD_F_READLANE_SCAN    CONVENTIONAL  all                 order 2 only: the v_readlane-paired scan; not with TABLE_SCAN
 *   LDPC_OSD_F_PB_BLOCK         PB            all                 every frame through the sorted-chunk kernel from its first TEP
 *   LDPC_OSD_F_PB_REPLAY        PB            all                 every frame through the list replay; not with PB_BLOCK
 *   LDPC_OSD_F_PB_FRONT_INSIDE  PB            ldpc_osd_decode,    the front end inside the first PB kernel (no workspace
 *                                             ldpc_pipeline_run   traffic, 4-5 % slower); not with PB_REPLAY, not where the
 *                                             (d_perm/d_parity    caller supplies or wants the front-end results
 *                                             NULL)                                                                          */
#define LDPC_OSD_F_TABLE_SCAN       (1u << 0)
#define LDPC_OSD_F_PB_BLOCK         (1u << 1)
#define LDPC_OSD_F_PB_REPLAY        (1u << 2)
#define LDPC_OSD_F_READLANE_SCAN    (1u << 3)
#define LDPC_OSD_F_PB_FRONT_INSIDE  (1u << 4)

typedef struct ldpc_osd_params {
    int32_t order;       /* 0..3                                                          */
    int32_t algo;        /* LDPC_OSD_*                                                    */
    float snr_db;        /* PB-OSD: noise_variance = 10^(-snr/10), pb_testing.py:50-52     */
    float fs_beta;       /* FS-OSD beta, Main_FS_OSD.py:20 (0.1)                          */
    float fs_tau_e;      /* FS-OSD floor(d_min-1)/2 as the reference evaluates it (6.5)    */
    float fs_tau_psc;    /* FS-OSD tau_psc, FS_OSD/globalmap.py:50 (30)                    */
    int32_t fs_reference_quirk; /* 1: keep optimal_codeword un-updated on a tau_e hit (fs_testing.py:145) */
    int32_t flags;       /* LDPC_OSD_F_* (table above); 0 = the default route                                       */
    void *d_aux;         /* optional DEVICE [F][4] i32, PB-OSD statistics per frame: {frontier comparisons
                            (memory_sum, pb_testing.py:122), suc counter 1 (:138), suc counter 2 (:144),
                            stop reason 0 = none / 1 = promising rule (:129) / 2 = success rule (:145)} */
    int64_t y_frames;    /* 0 = d_index is trusted (default).  > 0 = debug bound: the number of frames d_y holds;
                            ldpc_osd_decode / ldpc_osd_search then run on a sanitised copy of d_index (entries outside
                            [0, y_frames) replaced by 0) and count the offenders, see ldpc_osd_index_errors.
                            It guards CALLER-MADE lists: ldpc_pipeline_run writes d_index itself (its compaction emits
                            valid, ascending frame numbers only), so there the field checks nothing that can be wrong, and
                            the pipeline's counting launch reads the list the library wrote              */
} ldpc_osd_params;

/* PB-OSD tuning of a context (ABI 4; rounds 1-3 read these from LDPC_PB_* environment variables on every call).
 * None of it changes a result -- TEP counts, stop reasons, winners and metrics are the same for every setting (the
 * tests run the kernels under several) -- only how the searches of pb_osd (PB_OSD/pb_testing.py:100-149) are cut into
 * chunks and when a long search moves from the one-wavefront kernel to the one-workgroup kernel:
 *   budget_s / budget_m / budget / budget_l / budget_xl
 *                  TEPs after which a search may be handed to the workgroup kernel, chosen on the device by the number of
 *                  frames still searching after the weight-1 head (a sixteenth of them: < 128 / < 448 / < 1400 / < 3000 /
 *                  more); >= 1.  Defaults 512 / 1024 / 4096 / 8192 / 24576 (measurements: DESIGN.md 3.4).
 *   t1, t2         target size of a frame's first / later chunks in the one-wavefront kernel, 32..832 (320, 600)
 *   t3             target chunk size of the workgroup kernel, 256..4096 (3072)
 *   late_min, late_maxlen, late_pct, late_div
 *                  the launch's tail: once the frames of a sub-list that have not finished are fewer than late_pct % of
 *                  the chip's wavefront slots (a sixteenth of 4096), a search leaves after budget / late_div TEPs, for
 *                  lists of more than late_min frames and sub-lists shorter than late_maxlen; late_div = 1 switches
 *                  it off.  Defaults 4608, 2^30, 20, 16.  With it, WHERE a search is handed on depends on timing.
 *   handoff_maxlen no search is handed on when the sub-list holds this many frames or more (default 2^30)
 * ldpc_ctx_set_pb_tuning validates (LDPC_E_ARG, nothing changed) and stores a copy; NULL restores the defaults.  It
 * applies to decode calls ISSUED afterwards (a captured graph keeps the values it was captured with); call it from
 * one thread, not concurrently with decode calls that should see a particular setting.                            */
typedef struct ldpc_pb_tuning {
    int32_t budget, budget_s, budget_m, budget_l, budget_xl;
    int32_t t1, t2, t3;
    int32_t late_min, late_maxlen, late_pct, late_div;
    int32_t handoff_maxlen;
} ldpc_pb_tuning;
int ldpc_ctx_get_pb_tuning(ldpc_ctx *ctx, ldpc_pb_tuning *out);
int ldpc_ctx_set_pb_tuning(ldpc_ctx *ctx, const ldpc_pb_tuning *tuning);

/* Pre-size OSD workspaces (640 B per frame: permutation + reduced parity rows) for up to max_frames
 * frames per ldpc_osd_decode call: ldpc_osd_reserve sizes the NULL stream's workspace immediately and every
 * other stream's when it is created.  Decode calls grow their stream's workspace on demand, which allocates
 * -- so before capturing calls on a stream into a hipGraph, size that stream's workspace with
 * ldpc_osd_reserve_stream: params = NULL sizes the front-end workspace only; with params it also sizes what
 * the search of (params->algo, params->order) needs (PB-OSD: frame lists, one 1536-byte record per frame, list-replay
 * areas, ~1.5 KiB per frame + 180 MB), so that the FIRST call on the stream may be the captured one.
 * ldpc_osd_release_stream frees the workspace of `stream` (idle, not capturing; graphs captured on it must
 * not be launched afterwards) -- for destroyed streams, whose handle the runtime may hand out again.     */
int ldpc_osd_reserve(ldpc_ctx *ctx, int64_t max_frames);
int ldpc_osd_reserve_stream(ldpc_ctx *ctx, int64_t max_frames, const ldpc_osd_params *params, void *stream);
int ldpc_osd_release_stream(ldpc_ctx *ctx, void *stream);

/* Ordered-statistics decoding of F frames (front end + search).
 *   d_cw      [F][2] u64  best codeword, ORIGINAL bit order
 *   d_metric  [F] f32     its weighted Hamming distance  sum_p (c_p xor h_p) |y_p|
 *   d_best    [F] i32     index of the winning TEP in the reference's table order
 *                         (conventional), or its rank in visit order (FS/PB; 0 = all-zero TEP)
 *   d_ntep    [F] i32     number of TEPs evaluated (FS: num_teps, fs_testing.py:141; PB: cost_tep_num
 *                         or N_max when no rule fired, pb_testing.py:152-155)
 * Any of d_metric/d_best/d_ntep may be NULL, and so may params->d_aux, each on its own: the other outputs do not change.
 * d_y, params and d_cw are required; d_index / d_count are optional as described above.
 * Concurrency: calls on different streams may overlap, whatever the algorithm (scratch is per stream,
 * see ldpc_ctx_create).                                                                       */
int ldpc_osd_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                    int32_t *d_ntep, void *stream);

/* Number of d_index entries found outside [0, y_frames) by calls that carried ldpc_osd_params.y_frames > 0, since the
 * context was created.  Synchronises the device (a debug aid, not for captured or timed regions).            */
int ldpc_osd_index_errors(ldpc_ctx *ctx, int64_t *count);

/* The search alone, on front-end results supplied by the caller (ldpc_osd_front, or any
 * (perm, P') pair: with perm = identity and d_y already in the primed order this is exactly
 * convention_osd_main / the fs_osd / pb_osd inner loops applied to (updated_inputs, reduced_G)).
 * Nullable as for ldpc_osd_decode; d_perm and d_parity are required.                               */
int ldpc_osd_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    const uint8_t *d_perm /*[F][128]*/, const uint64_t *d_parity /*[F][64]*/,
                    const ldpc_osd_params *params, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
                    void *stream);

/* One GIVEN test error pattern per frame on front-end results: one_tep_compare, FS_OSD/fs_testing.py:51-64
 * (re-encode the MRB hard decisions with the positions of d_mask[f] flipped; its (:58-62) Hamming and weighted
 * distances to the hard decisions of y').  Any weight.  Same LUT evaluation and float order as the searches.
 *   d_mask   [F] u64   bit p = flip MRB position p (primed order)
 *   d_cw     [F][2] u64 candidate codeword, ORIGINAL bit order;  d_metric [F] f32 (nullable);  d_hd [F] i32 (nullable) */
int ldpc_osd_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                      const uint8_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw,
                      float *d_metric, int32_t *d_hd, void *stream);

/* OSD statistics against labels: d_counts[3] += {frames, frames_wrong, teps_total}.
 * (the success test of convention_osd.py:65-66 / pb_testing.py:158 / fs_testing.py:162)
 * teps_total sums d_ntep and stays unchanged when d_ntep is NULL -- on every route, also where the search kernel counts
 * (ldpc_pipeline_run's d_osd_counts).  d_cw, d_label_bits and d_counts are required; d_index NULL = labels are
 * addressed directly (label f for codeword f); d_count NULL = exactly F frames.            */
int ldpc_osd_counts(ldpc_ctx *ctx, const uint64_t *d_cw, const uint64_t *d_label_bits, const int32_t *d_index,
                    const int32_t *d_count, const int32_t *d_ntep, int64_t F, int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * OSD for short codes of any shape, i.e. every code with 1 <= k <= 64 and 1 <= n-k <= 64 (hence n <= 128): the
 * reference's (96,48) and (121,60) alist codes, and (128,64) itself, where the results equal those of the entry
 * points above bit for bit.  Served:
 *   the front end               swapped_info / identify_mrb / full_gf2elim, PB_OSD/pb_testing.py:231-320
 *   the conventional search     convention_osd_main, FS_OSD/convention_osd.py:49-76, orders 0..3
 *   FS-OSD                      fs_osd, FS_OSD/fs_testing.py:129-161, orders 0..min(3, k)
 *   one given TEP per frame     one_tep_compare, FS_OSD/fs_testing.py:51-64
 *   PB-OSD                      pb_osd, PB_OSD/pb_testing.py:100-149, orders 0..min(3, k)
 * Everything else of this header that says OSD -- the PB tuning (ldpc_pb_tuning), the elimination primitive, the H-form
 * primitives, ldpc_pipeline_run (the one call on these shapes is ldpc_family_pipeline_run, at the end of this header), the LDPC_OSD_F_* flags (the LDPC_OSD_F_PB_* routes among them) and y_frames of
 * ldpc_osd_params, d_aux outside the PB pair, and the entry points above themselves -- stays with (n = 128, k = 64) and
 * keeps answering LDPC_E_UNSUPPORTED on other shapes.
 * Same rules as above for d_index / d_count (min(*d_count, F) frames, read on the device; nothing at or beyond that
 * frame is written), for ties of the sort (lower index first), the TEP table (the one of this code's k, orders 0..3,
 * first minimum) and the float order of the metric: flipped MRB weights ascending from 0.0f, then bytes of eight
 * parity positions from primed position k (the last may be partial), each ascending from 0.0f, added in order.
 *   d_y       [*][n] f32, stride n: the layout of ldpc_nms_decode's d_soft
 *   d_perm    [F][128] u8 : original bit at primed position p < n (MRB 0..k-1, parity k..n-1); 0 for p >= n
 *   d_parity  [F][64] u64 : row r < k, bit c < n-k = P'[r][c]; rows >= k and bits >= n-k are written as 0
 *             (as inputs, the search entry points ignore d_perm entries p >= n, d_parity rows >= k and bits >= n-k)
 *   d_nswaps  [F] i32 (nullable): recorded column exchanges
 *   d_cw      [F][ceil(n/64)] u64 best codeword, ORIGINAL bit order (the layout of ldpc_pack_bits)
 *   d_metric  [F] f32, d_best [F] i32 (index into the table), d_ntep [F] i32: nullable, each on its own
 *   d_label_bits [*][ceil(n/64)] u64 addressed through d_index, d_counts[3] += {frames, frames_wrong, teps_total}
 *             as the counting entry point above does: both or neither (nullable); teps_total moves only with d_ntep
 * The decode entry points are two launches through the caller's d_perm / d_parity, which are scratch AND outputs and
 * required: there is no library workspace and no per-stream state.  Before any launch: an unsupported shape is
 * LDPC_E_UNSUPPORTED (the message names the limits and the code's (n,k)), an order outside its range and a NULL in a
 * required pointer are LDPC_E_ARG, F == 0 is LDPC_OK.  The tables (G columns, the order-3 TEP table, the FS visit
 * order of k and the PB constants of k and n-k) are uploaded by ldpc_ctx_create; nothing is allocated and nothing synchronises in a call
 * (graph-capturable).
 * The FS entry points read `params` for order, algo, fs_beta, fs_tau_e, fs_tau_psc and fs_reference_quirk, with the
 * meaning they have in ldpc_osd_decode: the lower bound of weight w is the sum of the w least reliable MRB |y'|
 * (positions k-w .. k-1, ascending from 0.0f) plus (float)((double)fs_beta * (n-k)); d_best is the rank in visit
 * order (0 = the all-zero TEP), d_ntep is num_teps (:141); with fs_reference_quirk = 0 a tau_e stop returns the
 * stopping candidate, its own metric and its rank.  LDPC_E_ARG, naming the offender, for algo != LDPC_OSD_FS, an
 * order outside 0..min(3, k) (the bound has no meaning for w > k), flags != 0, d_aux != NULL and y_frames != 0.
 * The one-TEP entry point is ldpc_osd_tep_eval with the split at k: d_mask [F] u64, bit p < k flips MRB position p
 * (bits at or beyond k are ignored); d_cw [F][ceil(n/64)] u64; d_metric [F] f32 and d_hd [F] i32 are nullable.
 * The PB entry points read `params` for order, algo, snr_db and d_aux (nullable DEVICE [F][4] i32: {frontier comparisons,
 * suc1, suc2, stop reason}), with the meaning they have in ldpc_osd_decode and its float conventions with 64 replaced by
 * k and m = n-k: c4 = (float)(-4 / 10^(snr_db/10)); q_p = 1 / (1 + det_expf(-(c4 |y'_p|))) in float32; p1 and the mean
 * |y'| over the parity part divided by (float)m, pt over the MRB by (float)k, the product of 1 - q_p over the MRB, each
 * ascending; the binomial CDFs of (m, p1), (m, 1/2) and (k, pt) by the float64 pmf recurrence with q^N by left-to-right
 * square-and-multiply; beta clamped to 0..m; N_max = sum of C(k, w) over w <= order.  The frontier starts as {k-1}; a
 * step pops the first minimum by (reliability sum, insertion order) and appends the extended child e + {k-1}, then the
 * adjacent child.  d_best is the rank in visit order (0 = the all-zero TEP), d_ntep is cost_tep_num, or N_max when no
 * rule fired.  The frontier lives in LDS (one slot per run of adjacent children, at most 1 + (k-1) + C(k-1, 2) of them):
 * no workspace here either.  LDPC_E_ARG, naming the offender, for algo != LDPC_OSD_PB, an order outside
 * 0..min(3, k), flags != 0 and y_frames != 0.
 * ------------------------------------------------------------------------------------- */
int ldpc_osdx_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int ldpc_osdx_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    uint8_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream);
int ldpc_osdx_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     const uint8_t *d_perm, const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdx_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     int32_t order, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream);

int ldpc_osdx_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdx_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);
int ldpc_osdx_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                       const uint8_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw,
                       float *d_metric, int32_t *d_hd, void *stream);
int ldpc_osdx_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdx_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * OSD for high-rate short codes, i.e. every code with n <= 128 and 1 <= n-k <= 64 (hence every k from 1 to 127): the
 * reference's (121,80) array code, which the ldpc_osdx_* entry points above refuse for its k > 64.  Served: the front end,
 * the conventional search (orders 0..3), FS-OSD and PB-OSD (orders 0..min(3, k)) and one-TEP evaluation.  Codes with k <= 64
 * are served as well; there d_perm, d_cw, d_metric, d_best, d_ntep, d_hd, d_nswaps and d_aux equal those of the ldpc_osdx_*
 * call of the same name bit for bit, and the first 64 rows of d_parity equal the d_parity of those calls.  The staged PB
 * routes, ldpc_pb_tuning, the LDPC_OSD_F_PB_* flags and ldpc_pipeline_run stay with (128,64) (ldpc_family_pipeline_run serves this family); codes with n-k > 64 or
 * n > 128 are refused by every OSD entry point.
 * The contract is that of ldpc_osdx_front / _search / _decode -- d_index / d_count, ties of the sort, the pivot rule, the
 * TEP table of this code's k (first minimum), the float order of the metric, the nullable outputs, d_label_bits with
 * d_counts[3] as a pair or not at all, teps_total only with d_ntep -- with one layout changed:
 *   d_perm    [F][128] u8  : original bit at primed position p < n (MRB 0..k-1, parity k..n-1); 0 for p >= n
 *   d_parity  [F][128] u64 : row r < k, bit c < n-k = P'[r][c]; rows >= k and bits >= n-k are written as 0
 *             (as inputs, the search entry points ignore d_perm entries p >= n, d_parity rows >= k and bits >= n-k)
 *   d_cw      [F][ceil(n/64)] u64 best codeword, ORIGINAL bit order
 * ldpc_osdw_decode is two launches through the caller's d_perm / d_parity, which are scratch AND outputs and required:
 * no library workspace, no per-stream state.  Before any launch: an unsupported shape is LDPC_E_UNSUPPORTED (the message
 * names the limits 1 <= n-k <= 64 and n <= 128 and the code's (n,k)), an order outside 0..3 and a NULL in a required
 * pointer are LDPC_E_ARG (naming the entry point and the pointer), F == 0 is LDPC_OK.  The tables (G columns as two
 * words each, the order-3 TEP table of k: 341 504 entries at k = 127, and the FS visit order of k: 341 503 entries) are
 * uploaded by ldpc_ctx_create; nothing is allocated and nothing synchronises in a call (graph-capturable).
 * ldpc_osdw_fs_search / _fs_decode / _tep_eval: the contract of ldpc_osdx_fs_search / _fs_decode / _tep_eval, word for word
 * -- `params` read for order, algo, fs_beta, fs_tau_e, fs_tau_psc and fs_reference_quirk; the lower bound of weight w the
 * sum of |y'| at positions k-w .. k-1 (ascending from 0.0f, on either side of position 64) plus
 * (float)((double)fs_beta * (n-k)); d_best the rank in visit order (0 = the all-zero TEP), d_ntep num_teps; with
 * fs_reference_quirk = 0 a tau_e stop returns the stopping candidate, its own metric and its rank; LDPC_E_ARG, naming the
 * offender, for algo != LDPC_OSD_FS, an order outside 0..min(3, k), flags != 0, d_aux != NULL, y_frames != 0 and a NULL in
 * a required pointer; ldpc_osdw_fs_decode is ldpc_osdw_front plus the scan, two launches -- with d_parity [F][128] u64 as
 * above and
 *   d_mask    [F][2] u64 : bit p of word 0 flips MRB position p, bit p of word 1 flips position 64 + p; bits at or
 *                          beyond k are ignored (for k <= 64 that is all of word 1)
 *   d_metric  [F] f32 and d_hd [F] i32 of ldpc_osdw_tep_eval: nullable, each on its own
 * ldpc_osdw_pb_search / _pb_decode: the contract of ldpc_osdx_pb_search / _pb_decode, word for word -- `params` read for
 * order (0..min(3, k)), algo (LDPC_OSD_PB), snr_db and d_aux ([F][4] i32, nullable: {frontier comparisons, suc1, suc2, stop
 * reason}); the float conventions stated there with the chains over the MRB running over all k <= 127 positions;
 * N_max = sum of C(k, w) over w <= order (341 504 at k = 127, order 3); d_best the rank in visit order, d_ntep cost_tep_num,
 * or N_max when no rule fired; outputs nullable, each on its own; labels and counts as a pair or not at all; LDPC_E_ARG,
 * naming the offender, for algo != LDPC_OSD_PB, an order outside 0..min(3, k), flags != 0, y_frames != 0 and a NULL in a
 * required pointer; ldpc_osdw_pb_decode is ldpc_osdw_front plus the scan, two launches -- with d_parity [F][128] u64 as
 * above.  The frontier lives in LDS, at most 1 + (k-1) + C(k-1, 2) = 8002 slots of 8 bytes at k = 127: an order-3 launch
 * takes 28, 44 or 75 KiB of LDS per workgroup for k <= 64, k <= 91 and k <= 127; no workspace, no per-stream state.
 * ------------------------------------------------------------------------------------- */
int ldpc_osdw_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int ldpc_osdw_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    uint8_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream);
int ldpc_osdw_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     const uint8_t *d_perm, const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdw_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     int32_t order, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream);

int ldpc_osdw_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdw_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);
int ldpc_osdw_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                       const uint8_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw,
                       float *d_metric, int32_t *d_hd, void *stream);
int ldpc_osdw_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint8_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdw_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint8_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * OSD for longer and low-rate codes, i.e. every code with n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192: the reference's
 * wimax-like (384,192) code and the codes with n <= 128 and n-k > 64, which the two families above refuse.  Served: the
 * front end, the conventional search (orders 0..3), FS-OSD and PB-OSD (orders 0..min(3, k)) and one-TEP evaluation.  The
 * H-form primitives, the staged PB routes, ldpc_pb_tuning, the LDPC_OSD_F_PB_* flags and ldpc_pipeline_run
 * are not served for these shapes (ldpc_family_pipeline_run is); codes with n > 384, k > 192 or n-k > 192 -- wimax (1056,880) among them -- are refused
 * by every OSD entry point.
 * The contract is that of ldpc_osdx_front / _search / _decode -- d_index / d_count read on the device and nothing written at
 * or beyond frame min(*d_count, F), ties of the sort to the lower index, the reference's pivot and exchange rule, the TEP
 * table of this code's k (orders 0..3, first minimum), the float order of the metric (flipped MRB weights ascending from
 * 0.0f, then the parity positions in bytes of eight from primed position k, each byte ascending from 0.0f, added in
 * order), the nullable outputs, d_label_bits with d_counts[3] as a pair or not at all, teps_total only with d_ntep -- with
 * the layouts changed.  With S = ceil(n/64), W = ceil(k/64) and Wp = ceil((n-k)/64):
 *   d_perm    [F][64 S] u16     : original bit at primed position p < n (MRB 0..k-1, parity k..n-1); 0 for p >= n
 *   d_parity  [F][64 W][Wp] u64 : row r < k, bit c of word w = P'[r][64 w + c]; rows >= k and bits >= n-k are written as 0
 *             (as inputs, the search ignores those padded rows and bits; a d_perm entry >= n is the caller's error: that
 *             frame's result is unspecified, but nothing is read or written outside the buffers)
 *   d_cw      [F][ceil(n/64)] u64 best codeword, ORIGINAL bit order
 * For a code that ldpc_osdx_* or ldpc_osdw_* also serves d_parity is byte for byte theirs ([F][64] beside ldpc_osdx_*,
 * [F][128] beside ldpc_osdw_* with k > 64) and every other output equals theirs bit for bit, d_perm value for value.  (One
 * case is settled here as the CPU oracle has it: when every cost of a frame is +inf the first TEP of the table wins.)
 * ldpc_osdl_decode is two launches through the caller's d_perm / d_parity, which are scratch AND outputs and required: no
 * library workspace, no per-stream state.  Before any launch: an unsupported shape is LDPC_E_UNSUPPORTED (the message names
 * the limits n <= 384, 1 <= k <= 192 and 1 <= n-k <= 192 and the code's (n,k)), an order outside 0..3 and a NULL in a
 * required pointer are LDPC_E_ARG (naming the entry point and the offender), F == 0 is LDPC_OK.  The tables (G columns as W
 * words each, the order-3 TEP table of k: 1 179 809 entries, 4.7 MB, at k = 192, and the FS visit order of k: 1 179 808
 * entries; the tables another family keeps for this k are shared) are uploaded by ldpc_ctx_create; nothing is allocated and
 * nothing synchronises in a call (graph-capturable).
 * ldpc_osdl_fs_search / _fs_decode / _tep_eval: the contract of ldpc_osdw_fs_search / _fs_decode / _tep_eval, word for word
 * -- `params` read for order, algo, fs_beta, fs_tau_e, fs_tau_psc and fs_reference_quirk; the lower bound of weight w the
 * sum of |y'| at positions k-w .. k-1 (ascending from 0.0f, in whichever words of the MRB they lie) plus
 * (float)((double)fs_beta * (n-k)); d_best the rank in visit order (0 = the all-zero TEP), d_ntep num_teps; with
 * fs_reference_quirk = 0 a tau_e stop returns the stopping candidate, its own metric and its rank; outputs nullable, each on
 * its own; labels and counts as a pair or not at all; LDPC_E_ARG, naming the offender, for algo != LDPC_OSD_FS, an order
 * outside 0..min(3, k), flags != 0, d_aux != NULL, y_frames != 0 and a NULL in a required pointer; LDPC_E_UNSUPPORTED with
 * the limits above; F == 0 is LDPC_OK; ldpc_osdl_fs_decode is ldpc_osdl_front plus the scan, two launches -- with the
 * layouts of ldpc_osdl_front and
 *   d_mask    [F][W] u64 : bit p of word w flips MRB position 64 w + p; bits at or beyond k are ignored
 *   d_metric  [F] f32 and d_hd [F] i32 of ldpc_osdl_tep_eval: nullable, each on its own; HD = the weight of the TEP plus the
 *                          set bits of all Wp words of its parity discrepancy
 * The metric's float order is that of ldpc_osdl_search.  For a code that ldpc_osdx_* or ldpc_osdw_* also serves every output
 * equals that of their call of the same name bit for bit (d_mask: [F] beside ldpc_osdx_*, [F][2] beside ldpc_osdw_*).
 * ldpc_osdl_pb_search / _pb_decode: the contract of ldpc_osdw_pb_search / _pb_decode, word for word, in the layouts of
 * ldpc_osdl_front -- `params` read for algo (LDPC_OSD_PB), order (0..min(3, k)), snr_db and d_aux ([F][4] i32, nullable:
 * {frontier comparisons, suc1, suc2, stop reason}); d_best the rank of the winner in visit order (0 = the all-zero TEP), d_ntep
 * the number of TEPs visited; outputs nullable, each on its own; labels and counts as a pair or not at all; nothing written at
 * or beyond frame min(*d_count, F); LDPC_E_ARG, naming the entry point and the offender, for a wrong algo, an order out of
 * range, flags != 0, y_frames != 0 or a NULL in a required pointer; LDPC_E_UNSUPPORTED with the limits above and the code's
 * (n,k); F == 0 is LDPC_OK; ldpc_osdl_pb_decode is ldpc_osdl_front plus the scan, two launches through the caller's d_perm /
 * d_parity, no workspace, no per-stream state, nothing allocated, nothing synchronised (graph-capturable).  The search is the
 * literal replay of pb_osd that ldpc_osdw_pb_search is (first minimum of the frontier by sum and insertion order, extended
 * child before adjacent child, the deterministic exp and the float64 CDF recurrences), with the four per-frame chains over up
 * to 192 positions, beta clamped to n-k and the success product ascending over all n-k parity positions; its constants
 * (cdfH[193] of n-k, the binomial ratios of n-k and k) are uploaded by ldpc_ctx_create.  For a code that ldpc_osdx_* or
 * ldpc_osdw_* also serves every output, d_aux included, equals that of their call of the same name bit for bit; the older
 * families stay the ones to call for their shapes.
 * ------------------------------------------------------------------------------------- */
int ldpc_osdl_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int ldpc_osdl_front(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                    uint16_t *d_perm, uint64_t *d_parity, int32_t *d_nswaps, void *stream);
int ldpc_osdl_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     const uint16_t *d_perm, const uint64_t *d_parity, int32_t order, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdl_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                     int32_t order, uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw, float *d_metric,
                     int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits, int64_t *d_counts, void *stream);

int ldpc_osdl_fs_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint16_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdl_fs_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);
int ldpc_osdl_tep_eval(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                       const uint16_t *d_perm, const uint64_t *d_parity, const uint64_t *d_mask, uint64_t *d_cw,
                       float *d_metric, int32_t *d_hd, void *stream);
int ldpc_osdl_pb_search(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const uint16_t *d_perm, const uint64_t *d_parity, const ldpc_osd_params *params, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, void *stream);
int ldpc_osdl_pb_decode(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F,
                        const ldpc_osd_params *params, uint16_t *d_perm, uint64_t *d_parity, uint64_t *d_cw,
                        float *d_metric, int32_t *d_best, int32_t *d_ntep, const uint64_t *d_label_bits,
                        int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * H-form OSD primitives for the DL-OSD stage (n = 128, m = k = 64, full-rank H; other shapes: ldpc_hosdx_* below):
 * DL_OSD_Testing_serial/ordered_statistics_decoding.py and nn_net.py: the per-frame sort / elimination /
 * candidate scan, the scan with the sliding-window early stop, and the bit-wise CNN.
 * ------------------------------------------------------------------------------------- */

/* Host: the TEPs of one order pattern, osd.error_pattern_gen (:81-98): pattern[s] flips inside
 * segment [bounds[s], bounds[s+1]) of the MRB positions (bounds within 0..128), for s = 0..nseg-1; itertools.product
 * over the segments (leftmost slowest) of itertools.combinations inside each.
 * teps: [count][4] u8 {p0, p1, p2, weight} (ascending positions, unused = 0), or NULL to get the
 * count.  Patterns of total weight > 3 are LDPC_E_UNSUPPORTED.                               */
int64_t ldpc_hosd_pattern_teps(int32_t nseg, const int32_t *bounds, const int32_t *pattern, uint8_t *teps);

/* check_matrix_reorder + identify_mrb (:25-80, full_gf2elim :222-257) per frame:
 * positions sorted by ASCENDING |d_order_llr| (ties: lower index first), the columns of H gathered in
 * that order, Gauss-Jordan with the reference's pivot rule -> [I | M], MRB (last 64) sorted ascending.
 *   d_lri    [F][128] u8  : lri_p, original bit index at sorted position s                 (:34)
 *   d_uidx   [F][128] u8  : updated_index_order, sorted position at updated position p       (:67-68)
 *   d_M      [F][64] u64  : row r of updated_M (bit j = M[r][j], j = updated MRB position)   (:69)
 *   d_nswaps [F] i32 (nullable): recorded column exchanges, -1 = rank-deficient H (outputs undefined)
 * The original bit index at updated position p is d_lri[d_uidx[p]]; positions 0..63 are the LRB
 * (identity part, in the order the elimination left them), 64..127 the MRB.                  */
int ldpc_hosd_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx,
                    uint64_t *d_M, int32_t *d_nswaps, void *stream);

/* Block minima of sliding_osd / acquire_min (:153-186): for every frame and every TEP block b
 * (TEPs d_teps[d_block_off[b] .. d_block_off[b+1]) ), the smallest weighted Hamming distance of
 *   candidate = [ M . (e xor mrb0), e xor mrb0 ],  mrb0 = hard(d_order_llr) on the MRB     (:154-156,186-187)
 * to the hard decisions of d_metric_llr, weights |d_metric_llr|                              (:159-160,180-182).
 * Float order of the metric: positions in updated order, bytes of 8, each byte summed ascending
 * from 0, the 16 byte sums added ascending (oracle/np_oracle.py hosd_cost).
 *   d_block_min [F][nblk] f32 (required when nblk > 0: it is the call's primary output and is stored unguarded),
 *   d_block_arg [F][nblk] i32 (nullable; index into d_teps of the first minimum)
 *   d_truth  [F] f32 (nullable, needs d_label_bits [F][2] u64): the metric of the label      (:181-183)
 *   d_cw     [F][2] u64 (nullable): best candidate over all blocks, ORIGINAL bit order
 *   d_metric [F] f32, d_best [F] i32 (nullable): its metric and index into d_teps (first minimum)
 * d_cw, d_metric and d_best are nullable each on its own.
 * d_teps: DEVICE [ntep][4] u8 as ldpc_hosd_pattern_teps writes them (required when nblk > 0); d_block_off: DEVICE [nblk+1] i32
 * (required).                                                                                                         */
int ldpc_hosd_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                     const uint8_t *d_lri, const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                     const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                     int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                     void *stream);

/* The block scan of ldpc_hosd_search with the sliding-window early stop of the reference's lazy loop
 * (sliding_osd :187-218, sliding_window_ops :140-151; the classifier is Predict_outlier_light,
 * nn_net.py:136-149).  Same frame inputs and TEP blocks as ldpc_hosd_search (block minima and first-minimum
 * keys bit-identical to it), plus:
 *   win          the window width (1..15, nblk >= win)
 *   soft_margin  stop when p1 > soft_margin (compared in double)
 *   fcn_weights  HOST f32: dense1 kernel [win+1][win+1] then dense2 kernel [win+1][2], no biases;
 *                n_weights must be (win+1)^2 + 2(win+1).  Copied by value into the kernel arguments.
 *   group        blocks scanned together before the decisions they allow are replayed; 0 = the default
 *                (blocks until 256 TEPs and the first window); results do not depend on it.
 * The decisions: the first `win` blocks, then block by block; decision k (window = blocks k..k+win-1)
 * is skipped for k > 0 when block k+win-1's minimum is > global_min; otherwise the classifier runs on
 * the ascending window with float(k) appended -- h = x.W1 and z = h.W2, each output a sequential f32
 * sum over its input index starting from the first product; p1 = e1/(e0+e1), e_c = expf(z_c - max(z))
 * -- global_min = min(global_min, min(window)), and the frame stops when p1 > soft_margin.
 * Per-frame outputs (all nullable):
 *   d_deep_limit [F] i32  blocks the reference evaluates (windows = deep_limit - win + 1;
 *                          its complexity is acc_block_size[deep_limit])
 *   d_global_min [F] f32
 *   d_truth [F] f32, d_success [F] u8 (global_min == truth): need d_label_bits [F][2] u64   (:181-183, :213)
 *   d_cw [F][2] u64, d_metric [F] f32, d_best [F] i32: first minimum over blocks 0..deep_limit-1
 *   d_teps_evaluated [F] i32  TEPs the kernel scanned (>= the reference's complexity by the
 *                          speculative part of the last group)                                      */
int ldpc_hosd_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                      const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                      int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                      int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                      float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      int32_t *d_teps_evaluated, void *stream);

/* ---------------------------------------------------------------------------------------
 * H-form OSD primitives for short codes of any shape: ldpc_hosdx_*.
 *
 * Shapes served: every code with 1 <= k <= 64 and 1 <= m = n-k <= 64 (hence n <= 128) whose H, as given, has exactly n-k
 * rows, i.e. full row rank: (96,48), (64,32), (128,64), ...  Everything else is refused with LDPC_E_UNSUPPORTED before any
 * launch, and the message names the row count, n-k and (n,k); ldpc_hosdx_supported tells beforehand.
 * The limit: an H with redundant rows (the array codes: (121,60) has 66 rows of rank 61) is not served.  The reference's
 * full_gf2elim deletes zero rows as it meets them (ordered_statistics_decoding.py:239-242), so its column-exchange choice
 * depends on the order of the redundant rows; serving that exactly needs columns of more than 64 rows.  Those codes, and
 * k > 64, are served by ldpc_hosdw_* below (two-word columns); eliminating a row basis of H instead would be a different
 * decoder.
 *
 * The contract is that of ldpc_hosd_front / _search / _sliding above, parameter for parameter, with 128 / 64 replaced:
 *
 * Sort.  Positions p < n are sorted by ascending |d_order_llr| ([F][n] f32); ties go to the lower index first.  Positions
 * >= n do not exist: no padded lane ever sorts in front of a real one.
 * Front end.  The columns of H are gathered in sorted order; the elimination follows the reference's rule (:222-257) on m
 * rows -> [I_m | M]; updated positions 0..m-1 are the LRB in the order the elimination left them, m..n-1 the MRB, sorted
 * ascending.
 *   d_lri    [F][128] u8  : original bit at sorted position s < n; entries >= n are written as 0
 *   d_uidx   [F][128] u8  : sorted position at updated position p < n; entries >= n are written as 0
 *   d_M      [F][64] u64  : row r < m, bit j < k = updated_M[r][j]; rows >= m and bits >= k are written as 0.  As inputs
 *                           the search calls ignore them (and the entries >= n of d_lri / d_uidx).
 *   d_nswaps [F] i32 (nullable)
 * Metric.  d_metric_llr is [F][n] f32.  The metric runs over the n updated positions as ONE sequence, LRB first, summed in
 * bytes of eight positions (the last may be partial; a byte may straddle position m when m % 8 != 0), each byte ascending
 * from 0.0f, the ceil(n/8) byte sums added ascending from byte 0: np_oracle.hosd_cost wherever n % 8 == 0, and the rule of
 * the G-form families for the other shapes.
 * Scan outputs.  d_cw and d_label_bits are [F][ceil(n/64)] u64 in original bit order.  d_block_min, d_block_arg, d_truth,
 * d_metric, d_best, the sliding call's outputs, win, soft_margin, fcn_weights, group and the limit of 1024 TEP blocks are
 * those of ldpc_hosd_search / ldpc_hosd_sliding, including which outputs are nullable.
 * TEPs.  d_teps [ntep][4] u8 with positions < k, as ldpc_hosd_pattern_teps writes them for bounds within 0..k.  A position
 * >= k is the caller's error: that frame's result is unspecified, but nothing is read or written outside the buffers.
 * Validation and launch.  F == 0 is LDPC_OK.  A NULL in a required pointer is LDPC_E_ARG and the message names the entry
 * point and the pointer; all validation happens before the first launch.  ldpc_ctx_create uploads the tables (the H
 * columns as m-bit words); a call allocates nothing and synchronises nothing, so it can be captured in a graph.
 * On (128,64) every output of every ldpc_hosdx_* call equals that of the ldpc_hosd_* call of the same name, bit for bit.
 * ------------------------------------------------------------------------------------- */
int ldpc_hosdx_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int ldpc_hosdx_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx,
                     uint64_t *d_M, int32_t *d_nswaps, void *stream);
int ldpc_hosdx_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                      const uint8_t *d_lri, const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                      const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                      int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      void *stream);
int ldpc_hosdx_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream);

/* ---------------------------------------------------------------------------------------
 * H-form OSD primitives for high-rate codes and for an H with redundant rows: ldpc_hosdw_*, a superset of ldpc_hosdx_* as
 * ldpc_osdw_* is one of ldpc_osdx_*.
 *
 * Shapes served: n <= 128; H as given has R rows, 1 <= R <= 127, of rank m, 1 <= m <= 64; k = n - m, 1 <= k <= 127.  That is
 * every code ldpc_hosdx_* serves, the array codes ((121,60): 66 rows of rank 61; (121,80): 44 rows of rank 41) and
 * (87,70), (128,112), ...  Everything else (n > 128, a rank above 64, more than 127 rows) is refused with
 * LDPC_E_UNSUPPORTED before any launch, and the message names the entry point, R, n-k and (n,k); ldpc_hosdw_supported tells
 * beforehand.
 *
 * Redundant rows.  The elimination runs on all R rows of H as given and follows full_gf2elim (:222-257) to the letter: when
 * column i has no 1 in the rows from i on and row i is all-zero, row i is deleted, the later rows move up, and step i is
 * tried again; otherwise column i is exchanged with the first later column that has a 1 in row i.  Which exchanges happen
 * therefore depends on the order of the rows of H, as it does in the reference.  d_nswaps counts the recorded column
 * exchanges; deleted rows are not counted.
 *
 * The contract is that of ldpc_hosdx_front / _search / _sliding above, parameter for parameter (validation order, the
 * messages that name the NULL pointer, F == 0, nullable outputs, the limit of 1024 TEP blocks; a call allocates nothing and
 * synchronises nothing, so it can be captured in a graph), with m the RANK of H and these differences:
 *   d_M  [F][128] u64 : entry r < m holds bits j = 0..63 of row r of updated_M, entry 64 + r bits j = 64..k-1; everything
 *                       else (rows >= m, bits >= k) is written as 0, and ignored by the search calls as an input.  On a code
 *                       that ldpc_hosdx_* serves the first 64 entries are its d_M and the rest are zero.
 *   d_teps            : positions < k <= 127, as ldpc_hosd_pattern_teps writes them for bounds within 0..k; they are taken
 *                       modulo 128, and a position >= k is the caller's error: that frame's result is unspecified, but
 *                       nothing is read or written outside the buffers.
 * ldpc_ctx_create uploads the H columns as two-word R-bit columns ([128][2] u64) when the code is in the family.
 * Wherever ldpc_hosdx_* serves the code every other output of every ldpc_hosdw_* call equals that of the ldpc_hosdx_* call of
 * the same name, bit for bit.
 * ------------------------------------------------------------------------------------- */
int ldpc_hosdw_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int ldpc_hosdw_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint8_t *d_lri, uint8_t *d_uidx,
                     uint64_t *d_M, int32_t *d_nswaps, void *stream);
int ldpc_hosdw_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                      const uint8_t *d_lri, const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                      const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                      int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      void *stream);
int ldpc_hosdw_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint8_t *d_lri,
                       const uint8_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream);

/* ---------------------------------------------------------------------------------------
 * H-form OSD primitives for longer and low-rate codes: ldpc_hosdl_*, a superset of ldpc_hosdw_* (for an H of at most 192
 * rows) as ldpc_osdl_* is one of ldpc_osdw_*.
 *
 * Shapes served: n <= 384; H as given has R rows, 1 <= R <= 192, of rank m = n - k, 1 <= m <= 192; 1 <= k <= 192.  That is
 * every code ldpc_hosdx_* and ldpc_hosdw_* serve, plus (384,192), (256,192), (193,1), ...  Everything else is refused with
 * LDPC_E_UNSUPPORTED before any launch, and the message names the entry point, R, n-k and (n,k); ldpc_hosdl_supported tells
 * beforehand.
 *
 * The contract is that of ldpc_hosdw_front / _search / _sliding above, parameter for parameter (validation order, the
 * messages that name the NULL pointer, F == 0, every nullable output on its own, the limit of 1024 TEP blocks, win 1..15,
 * group, soft_margin compared in double, the classifier's float order, the row deletion of the elimination; a call
 * allocates nothing and synchronises nothing, so it can be captured in a graph), with these layouts, S = ceil(n/64),
 * Wm = ceil(m/64), Wk = ceil(k/64):
 *   d_lri, d_uidx       [F][64 S] u16 : entries >= n are written as 0 and ignored as inputs.
 *   d_M            [F][64 Wm][Wk] u64 : entry [r][w] holds bits j = 64w .. 64w+63 of row r of updated_M; rows >= m and
 *                                       bits >= k are written as 0 and ignored as inputs.
 *   d_cw, d_label_bits      [F][S] u64, original bit order.
 *   d_teps            [ntep][4] u8    : positions < k <= 192, as ldpc_hosdl_pattern_teps writes them for bounds within 0..k;
 *                                       a position >= k is the caller's error: that frame's result is unspecified, but nothing
 *                                       is read or written outside the buffers.
 * The metric is the any-shape rule over the n updated positions, LRB first, in bytes of eight: each byte is summed ascending
 * from 0.0f and the ceil(n/8) byte sums are added ascending.
 * ldpc_hosdl_pattern_teps is ldpc_hosd_pattern_teps with bounds within 0..192.
 * ldpc_ctx_create uploads the H columns as three-word R-bit columns ([384][3] u64) when the code is in the family.
 * Wherever ldpc_hosdw_* serves the code every output of every ldpc_hosdl_* call equals that of the ldpc_hosdw_* call of the
 * same name, bit for bit, once the layouts are converted.
 * ------------------------------------------------------------------------------------- */
int ldpc_hosdl_supported(const ldpc_ctx *ctx); /* 1: the entry points below serve this code; 0: they refuse it */
int64_t ldpc_hosdl_pattern_teps(int32_t nseg, const int32_t *bounds, const int32_t *pattern, uint8_t *teps);
int ldpc_hosdl_front(ldpc_ctx *ctx, const float *d_order_llr, int64_t F, uint16_t *d_lri, uint16_t *d_uidx,
                     uint64_t *d_M, int32_t *d_nswaps, void *stream);
int ldpc_hosdl_search(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F,
                      const uint16_t *d_lri, const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps,
                      const int32_t *d_block_off, int32_t nblk, const uint64_t *d_label_bits, float *d_block_min,
                      int32_t *d_block_arg, float *d_truth, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                      void *stream);
int ldpc_hosdl_sliding(ldpc_ctx *ctx, const float *d_order_llr, const float *d_metric_llr, int64_t F, const uint16_t *d_lri,
                       const uint16_t *d_uidx, const uint64_t *d_M, const uint8_t *d_teps, const int32_t *d_block_off,
                       int32_t nblk, int32_t win, double soft_margin, const float *fcn_weights, int32_t n_weights,
                       int32_t group, const uint64_t *d_label_bits, int32_t *d_deep_limit, float *d_global_min,
                       float *d_truth, uint8_t *d_success, uint64_t *d_cw, float *d_metric, int32_t *d_best,
                       int32_t *d_teps_evaluated, void *stream);

/* The bit-wise CNN of the DL-OSD stage, conv_bitwise.call (nn_net.py:174-197): for every frame f and
 * bit v, the sequence rows[f][0..L-1][v] (the retest layout of ldpc_nms_traj_rows, row 0 = channel
 * values, L = T+1 >= 7; preprocessing_inputs :198-211 without the transpose) through
 *   Conv1D 1->8, Conv1D 8->4, Conv1D 4->2 (kernel 3, valid, no bias), Flatten, Dense(2(L-6) -> 1) + bias.
 * (The model's PReLU is never applied in call.)
 * weights: HOST f32, packed in Keras layouts: conv1 [3][1][8], conv2 [3][8][4], conv3 [3][4][2],
 *   dense kernel [2(L-6)][1] (Flatten order: position-major, channel-minor), dense bias [1] --
 *   n_weights = 24 + 96 + 24 + 2(L-6) + 1.  Copied by value into the kernel arguments.
 * Float order: every conv output is a sequential f32 sum over the flattened (tap, in-channel) index,
 * tap-major, starting from the first product; the dense output the sequential sum over the flattened
 * index starting from the first product, then + bias.  No fused multiply-adds.
 *   d_rows [F][L][n] f32, d_out [F][n] f32.                                                          */
int ldpc_dia_cnn(ldpc_ctx *ctx, const float *d_rows, int64_t F, int32_t L, const float *weights, int32_t n_weights,
                 float *d_out, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training step of the bit-wise CNN: the loss of the DL-OSD training stage and its gradient with respect to EVERY
 * weight, in one call.  Replaces, relative to LDPC_128/DL_Training_serial/ of the reference, conv_bitwise.call
 * nn_net.py:173-196 under the tf.GradientTape of nn_training.py:390-398 with calculate_loss :293-297:
 *   loss = sum_{f,v} max(z,0) - z y + log1p(exp(-|z|)),   z = -out[f][v],  y = label bit of (f, v)
 * (tf.nn.sigmoid_cross_entropy_with_logits(logits = -out, labels = bit), summed over frames and bits).
 * The forward pass is ldpc_dia_cnn's, same device code and float order: d_out equals its output bit for bit.
 * The network has no activation, so out = bias + sum_r E[r] x[r] with an effective filter E of the weights alone; with
 * g = dloss/dout = y - sigmoid(-out) (computed as y ? sigmoid(out) : -sigmoid(-out), each 1 / (1 + exp(-t)), f32)
 *   dloss/dtheta = sum_r dE[r]/dtheta m[r],  m[r] = sum_{f,v} g[f][v] rows[f][r][v];   dloss/dbias = sum_{f,v} g[f][v]
 * The products g x are f32 (one rounding each), every sum is f64, and the back-propagation at m runs in f64.  These are
 * the gradient rules of the ops the reference uses; they are not pinned against TensorFlow, which is not available to
 * check them, as for ldpc_nms_train_grad.
 *   d_rows        [F][L][n] f32, weights / n_weights: as ldpc_dia_cnn (7 <= L <= 64, n_weights = 145 + 2(L-6))
 *   d_label_bits  [F][ceil(n/64)] u64 packed code bits (the layout of ldpc_eval_counts)
 * Outputs, any subset of them NULL:
 *   d_out         [F][n] f32 refined values
 *   d_loss_sum    [1] f64
 *   d_grad_sum    [n_weights] f64, in the packed order of the weights
 * No atomics: per-workgroup partial sums and a fixed tree whose shape depends on (F, n, L) alone, so repeated calls give
 * the same bits on any stream.  Scratch for the partials (at most 2 MiB) is allocated and freed in stream order; the
 * call makes no host-device copy and does not synchronise.  F = 0 writes nothing.  Refusals (LDPC_E_ARG, before any
 * launch) name the call and the offending argument.
 * ------------------------------------------------------------------------------------- */
int ldpc_dia_cnn_grad(ldpc_ctx *ctx, const float *d_rows, const uint64_t *d_label_bits, int64_t F, int32_t L,
                      const float *weights, int32_t n_weights, float *d_out, double *d_loss_sum, double *d_grad_sum,
                      void *stream);

/* ---------------------------------------------------------------------------------------
 * Training of the sliding-window early-stop classifier (Predict_outlier_light, the `fcn` of ldpc_hosd_sliding).
 * Relative to LDPC_128/DL_Training_serial/ of the reference: reform_inputs interval_boundary.py:224-249 and the
 * loss / tape / validation of predict_phase.py:104-135, :203-212, :236-260.
 *
 * Windows.  A record is the nblk block minima of one frame (a row of a search call's d_block_min); d_index [R] (nullable:
 * frames 0..R-1) selects the kept frames, as ldpc_compact writes them, and d_success[f] says whether frame f's overall
 * minimum is the label's metric (locate_phase != -1).  For window position i = 0 .. nblk-win and record r, output row
 * i*R + r (window-major) holds
 *   d_inputs [(nblk-win+1)*R][win+1] f32 : record[i .. i+win-1] in ascending order, then (float)i
 *   d_labels [(nblk-win+1)*R] u8         : min(window) == min(record) && d_success[frame]
 *   d_class_count [2] i64 (nullable)      : WRITTEN (not accumulated): rows with label 0, rows with label 1
 * 1 <= win <= 15 and win <= nblk <= 1024, the limits of ldpc_hosd_sliding.  Sort, minimum and equality are exact, so the
 * result is defined bit for bit; +inf is an ordinary value, a NaN makes that record's rows unspecified (nothing is read
 * or written outside the buffers).  The entries of d_index are the caller's: each must name a row of d_block_min.
 * Scratch (R floats) is allocated and freed in stream order; no host-device copy, no synchronisation.  R = 0 writes
 * nothing.  Refusals (LDPC_E_ARG, before any launch) name the call and the argument.                                  */
int ldpc_fcn_windows(ldpc_ctx *ctx, const float *d_block_min, const uint8_t *d_success, const int32_t *d_index, int64_t R,
                     int32_t nblk, int32_t win, float *d_inputs, uint8_t *d_labels, int64_t *d_class_count, void *stream);

/* Loss, gradient and counts of one batch of windows.  Sample b = 0..B-1 is row d_index[b] (nullable: row b; entries may
 * repeat and come in any order, each must name a row) of
 *   d_inputs [N][win+1] f32, d_labels [N] u8 (0 = continue, 1 = stop), d_weight [N] f32 (nullable: 1).
 * fcn_weights / n_weights: HOST, as ldpc_hosd_sliding (dense1 [win+1][win+1] then dense2 [win+1][2]; (win+1)^2 + 2(win+1)).
 * Forward, in the float order of ldpc_hosd_sliding: h = x.W1 and z = h.W2, each output a sequential f32 sum over its
 * input index from the first product; m = max(z), e_c = expf(z_c - m), p_c = e_c / (e0 + e1); no fused multiply-adds.
 * Per sample, with y the label, sw the weight, pred = p0 < p1, pen = (pred && y == 0) ? penalty : 1 (no gradient flows
 * through it) and s = (double)sw * pen:
 *   loss term  -s * log((double)max(p_y, 1e-30f))
 *   g_c = p_y >= 1e-30f ? s * ((double)p_c - [c == y]) : 0          (dloss/dz_c)
 * The network is linear up to the softmax: with the moments m[i][c] = sum_b x_i g_c (f64 products and sums)
 *   dW1[i][j] = sum_c m[i][c] W2[j][c],   dW2[j][c] = sum_i W1[i][j] m[i][c]      (f64, ascending index).
 * The kernel_regularizer of dense1 has no part in the reference's loss (model.losses is never added) and none here.
 * Outputs, any subset of them NULL; the others keep their bits:
 *   d_p        [B][2] f32
 *   d_loss_sum [1] f64
 *   d_grad_sum [n_weights] f64, in the packed order of the weights
 *   d_acc      [2] f64 : sum sw [pred == y], sum sw     (the weighted CategoricalAccuracy's numerator and denominator)
 *   d_counts   [3] i64 : #[y == pred], #[y > pred], #[y < pred]                      (S, F1, F2 of the validation)
 * d_labels is required when any output but d_p is asked for.  No float atomics: per-workgroup partial sums and a fixed
 * tree whose shape depends on (B, win) alone, so repeated calls give the same bits on any stream.  Scratch for the
 * partials (at most 76 KiB) is allocated and freed in stream order; no host-device copy, no synchronisation.  B = 0
 * writes nothing.  Refusals (LDPC_E_ARG, before any launch) name the call and the argument.                            */
int ldpc_fcn_grad(ldpc_ctx *ctx, const float *d_inputs, const uint8_t *d_labels, const float *d_weight, const int32_t *d_index,
                  int64_t B, int32_t win, const float *fcn_weights, int32_t n_weights, float penalty, float *d_p,
                  double *d_loss_sum, double *d_grad_sum, double *d_acc, int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * One batch through the whole path with a single host call: the body of the reference drivers'
 * per-batch loops (ldpc_128_testing.py:117-131 then pb_testing.py / fs_testing.py per failed frame):
 *   NMS-T -> error counters -> failed-frame compaction -> OSD (front end + search) on the failures
 *   -> OSD counters.
 * The results of the sequence ldpc_nms_decode, ldpc_eval_counts, ldpc_compact, ldpc_osd_front,
 * ldpc_osd_search, ldpc_osd_counts on one stream (the counters ride in the compaction's counting pass), without a host round trip in between (the OSD
 * kernels read the failure count on the device).  Nullable members switch their stage off: without d_label_bits or
 * d_nms_counts no NMS counters, without d_label_bits or d_osd_counts no OSD counters (teps_total moves only with d_ntep, on
 * every route); the other outputs do not change.  With osd_enable = 0 every member from `osd` on is ignored and may be NULL.
 * d_llr, alpha (T > 0), d_hard and d_fail are always required, d_index, d_count and d_cw when the OSD stage is on.
 * With timing_slot >= 0 the library brackets the three hot kernels with its own HIP events on
 * `stream`; after synchronising, ldpc_pipeline_timing returns their durations.
 * ------------------------------------------------------------------------------------- */
typedef struct ldpc_pipeline {
    const float *d_llr;            /* [B][n]                                               */
    int64_t B;
    int32_t T, nms_kernel;
    const float *alpha;            /* host [T]                                             */
    float w_in, w_out;
    float *d_soft;                 /* [B][n] nullable                                      */
    uint64_t *d_hard;              /* [B][n/64]                                            */
    uint8_t *d_fail;               /* [B]                                                  */
    const uint64_t *d_label_bits;  /* [B][n/64] nullable: no counters                      */
    int64_t *d_nms_counts;         /* [5] accumulated, nullable                            */
    int32_t osd_enable, timing_slot;
    ldpc_osd_params osd;
    int32_t *d_index, *d_count;    /* [B], [1]                                             */
    uint8_t *d_perm;               /* [B][128] nullable: both NULL = ldpc_osd_decode on the     */
    uint64_t *d_parity;            /* [B][64]  context workspace (no per-kernel OSD timing);
                                      exactly ONE of the two NULL is LDPC_E_ARG (OSD stage on)  */
    uint64_t *d_cw;                /* [B][2]                                               */
    float *d_metric;               /* [B] nullable                                         */
    int32_t *d_best, *d_ntep;      /* [B] nullable / [B]                                   */
    int64_t *d_osd_counts;         /* [3] accumulated, nullable (as ldpc_osd_counts)       */
} ldpc_pipeline;

#define LDPC_TIMING_SLOTS 64
int ldpc_pipeline_run(ldpc_ctx *ctx, const ldpc_pipeline *p, void *stream);
/* ms[3] = {NMS, OSD front end, OSD search} of the run that used `slot` (call after the stream is idle);
 * when d_perm/d_parity were NULL the OSD ran through ldpc_osd_decode: ms[1] = 0, ms[2] = whole OSD stage */
int ldpc_pipeline_timing(ldpc_ctx *ctx, int32_t slot, float *ms);

/* ---------------------------------------------------------------------------------------
 * The decoder's final output: the OSD codewords back among the NMS decisions, and the bit errors before and after.
 * For every j < min(*d_count, F) (read on the device), with f = d_index[j]:
 *   d_hard    [*][W] u64, W = ceil(n/64), nullable: d_hard[f] = d_cw[j], all W words, in place; no other row is touched
 *   d_counts  [4] i64 += {frames merged, frames with d_cw[j] != label[f], bit errors of d_cw[j] against label[f],
 *             bit errors of the OLD d_hard[f] against label[f]} -- with d_label_bits ([*][W] u64, addressed through
 *             d_index) and d_counts as a pair, or neither (the rule of the family decode calls); the fourth stays 0
 *             when d_hard is NULL
 * Every code a context exists for is served (no OSD family is needed).  The old word is read before it is replaced, by
 * the same thread; the entries of d_index are trusted and distinct, as everywhere in this header.  End-to-end bit
 * errors of a batch: nms bit_err - before + after; end-to-end frame errors: undetected + frames wrong.
 * One launch with work proportional to the failures; no workspace, nothing synchronises (graph-capturable).
 * F == 0 is LDPC_OK without a launch, and so is d_hard NULL with no counters; d_cw, d_index or d_count NULL with
 * F > 0 is LDPC_E_ARG naming the pointer.                                                                         */
int ldpc_osd_merge(ldpc_ctx *ctx, const uint64_t *d_cw /*[F][W]*/, const int32_t *d_index, const int32_t *d_count,
                   int64_t F, uint64_t *d_hard, const uint64_t *d_label_bits, int64_t *d_counts, void *stream);

/* ---------------------------------------------------------------------------------------
 * The one-call pipeline on the three G-form OSD families, i.e. for every code the ldpc_osdx_*, ldpc_osdw_* or
 * ldpc_osdl_* entry points serve (up to (384,192)); ldpc_pipeline_run above stays with (n = 128, k = 64).
 * The results of this sequence on one stream, with no host round trip, no allocation and no synchronisation:
 *   ldpc_nms_decode
 *   ldpc_eval_counts + ldpc_compact     (one launch when d_label_bits and d_nms_counts are given)
 *   ldpc_osd{x,w,l}_decode, _fs_decode or _pb_decode by osd.algo, on d_llr as ldpc_pipeline_run does, with
 *                                       d_label_bits and d_osd_counts riding in the scan
 *   ldpc_osd_merge into d_hard          (with `merge`), d_final_counts its counters
 * The members ldpc_pipeline has keep their meaning, and the nullable ones switch their stage off, each on its own.
 *   family        LDPC_OSD_FAMILY_AUTO: ldpc_osdx_* where it serves the code, else ldpc_osdw_*, else ldpc_osdl_*; or one
 *                 family by name.  A forced family that refuses the code, or AUTO on a code none serves (then with the
 *                 sentence of ldpc_osdl_*), is LDPC_E_UNSUPPORTED with "; this code is (n,k)".
 *   d_perm, d_parity   in the layouts of the chosen family's _front; REQUIRED with the OSD stage on: the caller's scratch
 *                 and output, as in the family decode calls (no library workspace).
 *   osd_capacity  the frames that d_perm, d_parity, d_cw, d_metric, d_best, d_ntep and osd.d_aux hold; 0 = B.  The OSD
 *                 stage and the merge run on min(*d_count, osd_capacity) frames and write nothing at or beyond that
 *                 frame; *d_count stays the number of syndrome failures, so frames were left out exactly when
 *                 d_osd_counts[0] < d_nms_counts[4].
 *   osd           order, algo and the FS / PB members as the family's entry points read them; flags and y_frames must be
 *                 0 and d_aux NULL outside LDPC_OSD_PB (LDPC_E_ARG naming the offender).
 * Everything is checked before the first launch.  With osd_enable = 0 every code a context exists for is served and
 * every member from `osd` on is ignored (NMS and its counters alone).  With B = 0 and the OSD stage on, *d_count is
 * zeroed.  timing_slot and ldpc_pipeline_timing serve both pipelines: ms = {NMS, front end, search}.
 * ------------------------------------------------------------------------------------- */
#define LDPC_OSD_FAMILY_AUTO 0   /* osdx where it serves the code, else osdw, else osdl */
#define LDPC_OSD_FAMILY_X 1
#define LDPC_OSD_FAMILY_W 2
#define LDPC_OSD_FAMILY_L 3
typedef struct ldpc_family_pipeline {
    const float *d_llr;            /* [B][n]                                               */
    int64_t B;
    int32_t T, nms_kernel;
    const float *alpha;            /* host [T]                                             */
    float w_in, w_out;
    float *d_soft;                 /* [B][n] nullable                                      */
    uint64_t *d_hard;              /* [B][ceil(n/64)]                                      */
    uint8_t *d_fail;               /* [B]                                                  */
    const uint64_t *d_label_bits;  /* [B][ceil(n/64)] nullable: no counters                */
    int64_t *d_nms_counts;         /* [5] accumulated, nullable                            */
    int32_t osd_enable, timing_slot;
    ldpc_osd_params osd;
    int32_t family, merge;         /* LDPC_OSD_FAMILY_*; merge != 0: ldpc_osd_merge into d_hard */
    int32_t *d_index, *d_count;    /* [B], [1]                                             */
    void *d_perm;                  /* [C][...] the family's perm rows, C = osd_capacity    */
    uint64_t *d_parity;            /* [C][...] the family's parity rows                    */
    int64_t osd_capacity;          /* C; 0 = B                                             */
    uint64_t *d_cw;                /* [C][ceil(n/64)]                                      */
    float *d_metric;               /* [C] nullable                                         */
    int32_t *d_best, *d_ntep;      /* [C] nullable, each on its own                        */
    int64_t *d_osd_counts;         /* [3] accumulated, nullable (as the family decode calls) */
    int64_t *d_final_counts;       /* [4] accumulated, nullable (as ldpc_osd_merge)        */
} ldpc_family_pipeline;
int ldpc_family_pipeline_run(ldpc_ctx *ctx, const ldpc_family_pipeline *p, void *stream);

/* ---------------------------------------------------------------------------------------
 * The one-call pipeline with the DL-OSD stage on the four H-form families, i.e. for every code the ldpc_hosd_*,
 * ldpc_hosdx_*, ldpc_hosdw_* or ldpc_hosdl_* entry points serve (up to (384,192)): the counterpart of
 * ldpc_family_pipeline_run for the decoder of nn_testing.Testing_OSD, from channel frames.
 * The results of this sequence on one stream, with no host round trip, no allocation and no synchronisation (the frame
 * count of every step after the compaction is min(*d_count, C), read on the device; C = osd_capacity):
 *   ldpc_nms_decode
 *   ldpc_eval_counts + ldpc_compact     (one launch when d_label_bits and d_nms_counts are given)
 *   ldpc_nms_traj_rows on the list      -> d_rows [C][T+1][n]                       (with a CNN only)
 *   ldpc_dia_cnn                        -> d_order_llr [C][n]                       (with a CNN only)
 *   gather (one launch)                 -> d_metric_llr [C][n] = d_llr[d_index[j]], d_list_labels [C][W] = d_label_bits[d_index[j]]
 *   ldpc_hosd{,x,w,l}_front  on the ordering values      -> d_lri, d_uidx, d_M, d_nswaps
 *   ldpc_hosd{,x,w,l}_sliding on them and d_metric_llr   -> d_deep_limit, d_global_min, d_truth, d_success, d_cw, d_metric,
 *                                                           d_best, d_teps_evaluated
 *   stage counters (one launch)         -> d_dl_counts
 *   ldpc_osd_merge into d_hard          (with `merge`), d_final_counts its counters
 * The members up to timing_slot, d_index, d_count, osd_capacity, merge and d_final_counts are those of
 * ldpc_family_pipeline, with the same meaning and the same nullable rules.  The stage and the merge run on
 * min(*d_count, C) frames and write nothing at or beyond that row of any list buffer; *d_count stays the number of
 * syndrome failures, so frames were left out exactly when d_dl_counts[0] < d_nms_counts[4].
 *   family        LDPC_HOSD_FAMILY_AUTO: ldpc_hosd_* on (128,64), else ldpc_hosdx_*, else ldpc_hosdw_*, else ldpc_hosdl_*
 *                 (what Decoder.hosd_stage_family() picks on every code a family serves; on a code none serves that
 *                 method names hosdw and AUTO ends at hosdl, the last one tried: both refuse); or one family by name.  A forced family that refuses the code
 *                 is LDPC_E_UNSUPPORTED with that family's own sentence, AUTO on a code none serves with the sentence of
 *                 ldpc_hosdl_*.
 *   cnn_weights   host [n_cnn_weights], as ldpc_dia_cnn takes them (L = T + 1 >= 7, checked before any launch).  NULL is
 *                 DIA = False: no trajectory is decoded, d_rows is neither read nor written and may be NULL, and the
 *                 ordering values are the channel values.  d_order_llr may then be NULL -- it aliases d_metric_llr: front
 *                 end and scan read that buffer for both of their inputs -- or a buffer of its own, which the gather fills
 *                 with the same rows.
 *   d_teps, d_block_off, nblk, win, soft_margin, fcn_weights, n_fcn_weights, group   as ldpc_hosd_sliding takes them.
 *                 Both weight blocks are HOST memory and are copied by value into the kernel arguments at the call, and
 *                 hence at capture: a captured graph keeps the weights it was captured with.
 *   d_lri, d_uidx, d_M   C rows each in the layouts of the chosen family's _front (u8 [128] / u16 [64 ceil(n/64)] indices);
 *                 the caller's scratch and output.  Required with the stage on, as are d_index, d_count, d_metric_llr,
 *                 d_cw, d_teps, d_block_off and fcn_weights; d_rows and d_order_llr with a CNN.
 *   d_nswaps, d_deep_limit, d_global_min, d_truth, d_success, d_metric, d_best, d_teps_evaluated   [C], nullable, each on
 *                 its own (d_truth and d_success are written with d_label_bits only); d_deep_limit is required whenever
 *                 d_dl_counts is given.  d_list_labels [C][W] is required when d_label_bits is given, and ignored without.
 *   d_dl_counts   [6] i64 += {frames through the stage, frames with global_min == truth (the reference's S), the others
 *                 (its F), sum of deep_limit - win + 1 (windows), sum of d_block_off[deep_limit] (the reference's
 *                 complexity, acc_block_size[deep_limit]), sum of d_teps_evaluated}.  [1] and [2] need d_label_bits and
 *                 somewhere the scan's verdict lands: d_success, or d_global_min and d_truth together (the counters then
 *                 compare the two floats as the scan does); with labels and none of these they stay.  [5] moves with
 *                 d_teps_evaluated only.
 * Everything is checked before the first launch; a refusal begins "ldpc_dlosd_pipeline_run: " and names the member (an
 * unsupported shape is the family's sentence).  With osd_enable = 0 every code a context exists for is served and every
 * member from `family` on is ignored (NMS and its counters alone).  With B = 0 and the stage on, *d_count is zeroed.
 * timing_slot and ldpc_pipeline_timing serve this pipeline too: ms = {NMS, rows + CNN + gather + front end, sliding scan}.
 * ------------------------------------------------------------------------------------- */
#define LDPC_HOSD_FAMILY_AUTO 0   /* hosd on (128,64), else hosdx, else hosdw, else hosdl */
#define LDPC_HOSD_FAMILY_128 1
#define LDPC_HOSD_FAMILY_X 2
#define LDPC_HOSD_FAMILY_W 3
#define LDPC_HOSD_FAMILY_L 4
typedef struct ldpc_dlosd_pipeline {
    const float *d_llr;            /* [B][n]                                               */
    int64_t B;
    int32_t T, nms_kernel;
    const float *alpha;            /* host [T]                                             */
    float w_in, w_out;
    float *d_soft;                 /* [B][n] nullable                                      */
    uint64_t *d_hard;              /* [B][ceil(n/64)]                                      */
    uint8_t *d_fail;               /* [B]                                                  */
    const uint64_t *d_label_bits;  /* [B][ceil(n/64)] nullable: no counters                */
    int64_t *d_nms_counts;         /* [5] accumulated, nullable                            */
    int32_t osd_enable, timing_slot;
    int32_t family, merge;         /* LDPC_HOSD_FAMILY_*; merge != 0: ldpc_osd_merge into d_hard */
    int32_t *d_index, *d_count;    /* [B], [1]                                             */
    int64_t osd_capacity;          /* C; 0 = B                                             */
    const float *cnn_weights;      /* host [n_cnn_weights]; NULL: no CNN (DIA = False)     */
    const float *fcn_weights;      /* host [n_fcn_weights]                                 */
    int32_t n_cnn_weights, n_fcn_weights;
    const uint8_t *d_teps;         /* [d_block_off[nblk]][4]                               */
    const int32_t *d_block_off;    /* [nblk + 1]                                           */
    int32_t nblk, win, group;
    double soft_margin;
    float *d_rows;                 /* [C][T+1][n], with a CNN                              */
    float *d_order_llr;            /* [C][n]; required with a CNN, nullable without        */
    float *d_metric_llr;           /* [C][n]                                               */
    uint64_t *d_list_labels;       /* [C][ceil(n/64)], required with d_label_bits          */
    void *d_lri, *d_uidx;          /* [C][...] the family's index rows                     */
    uint64_t *d_M;                 /* [C][...] the family's M rows                         */
    int32_t *d_nswaps;             /* [C] nullable                                         */
    int32_t *d_deep_limit;         /* [C] nullable without d_dl_counts                     */
    float *d_global_min, *d_truth; /* [C] nullable                                         */
    uint8_t *d_success;            /* [C] nullable                                         */
    uint64_t *d_cw;                /* [C][ceil(n/64)]                                      */
    float *d_metric;               /* [C] nullable                                         */
    int32_t *d_best, *d_teps_evaluated;   /* [C] nullable, each on its own                 */
    int64_t *d_dl_counts;          /* [6] accumulated, nullable                            */
    int64_t *d_final_counts;       /* [4] accumulated, nullable (as ldpc_osd_merge)        */
} ldpc_dlosd_pipeline;
int ldpc_dlosd_pipeline_run(ldpc_ctx *ctx, const ldpc_dlosd_pipeline *p, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LDPC_OSD_H */
