// Internal declarations shared by the translation units of libldpcosd.so (not installed): error reporting (fail, LDPC_HIP,
// first_null), the code and the context (which owns the OSD tables of ldpc_osd_tables.h), the host helpers and the launchers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ldpc_osd.h"
#include "ldpc_osd_tables.h"

namespace ldpc {

// thread-local error text behind ldpc_last_error()
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char *what);

// "<who>: <name> is NULL" (LDPC_E_ARG) for the first NULL among the required pointers, in the order given; LDPC_OK if none is
struct NamedPtr {
    const char *name;
    const void *ptr;
};
inline int first_null(const char *who, std::initializer_list<NamedPtr> required)
{
    for (const NamedPtr &r : required)
        if (!r.ptr) return fail(LDPC_E_ARG, "%s: %s is NULL", who, r.name);
    return LDPC_OK;
}

#define LDPC_HIP(call)                                      \
    do {                                                    \
        hipError_t e__ = (call);                            \
        if (e__ != hipSuccess) return ::ldpc::hip_fail(e__, #call); \
    } while (0)

// The grid of every kernel that runs one wavefront per workgroup: a workgroup per frame up to 65536, then strided (a wavefront
// decodes several frames in turn).
inline unsigned frame_grid(int64_t F) { return (unsigned)(F < 65536 ? F : 65536); }

// The grid of osd_front_kernel, a frame pipeline (ldpc_osd_small.h): kFrontGridX times the wavefronts that are resident at once,
// 32 per CU (8 per SIMD: 64 VGPRs and 4.6 KiB of LDS per one-wavefront workgroup), and no more than F.  Workgroup b decodes
// frames b, b + grid, b + 2 grid, ... below the device-side count, with the loads of the next frames in flight.  The time per
// frame hardly varies, so the dispatcher has nothing to even out: 1x was the fastest of 1x, 2x and 4x (profiles/front_pipeline/).
constexpr int kFrontGridX = 1;
inline unsigned front_grid(int cu_count, int64_t F)
{
    const int64_t g = (int64_t)cu_count * 32 * kFrontGridX;
    return (unsigned)(F < g ? F : g);
}

constexpr int kMaxIters = 64;  // alpha[] travels by value in the kernel arguments

struct AlphaArg {
    float a[kMaxIters];
};

// QC structure of a code whose H is an array of 16x16 circulants (CCSDS (128,64) shape):
// check (br, i) is joined to variable (bc, (i + s) mod 16) for every term (br, bc, s).
struct QcTerm {
    int br, bc, s;
};

}  // namespace ldpc

struct ldpc_code {
    int n = 0, m = 0, k = 0, max_chk_degree = 0, max_var_degree = 0, E = 0;
    std::vector<int32_t> H;         // [m][n]
    std::vector<int32_t> G;         // [k][n]
    std::vector<int32_t> chk_ptr;   // [m+1]   edges are numbered check-major
    std::vector<int32_t> chk_var;   // [E]     variable of edge e
    std::vector<int32_t> var_ptr;   // [n+1]
    std::vector<int32_t> var_edge;  // [E]     edge ids of variable v, ascending check index
    bool qc16_ccsds = false;        // H equals the compiled-in CCSDS (128,64) circulant table
};

struct ldpc_ctx {
    int device = 0, cu_count = 256;
    ldpc_code code;
    // generic NMS tables
    int32_t *d_chk_ptr = nullptr, *d_chk_var = nullptr, *d_var_ptr = nullptr, *d_var_edge = nullptr;
    ldpc::OsdTables osd_tables;    // G columns and TEP tables of any shape with k, n-k <= 64: read by every OSD family
    ldpc::OsdwTables osdw_tables;  // two-word G columns and the TEP table of k <= 127 (n <= 128, n-k <= 64): the ldpc_osdw_* family
    ldpc::OsdlTables osdl_tables;  // W-word G columns and the TEP table of k <= 192 (n <= 384, n-k <= 192): the ldpc_osdl_* family
    uint64_t *d_Hcols = nullptr;   // [128] column v < n of H as an m-bit word (bit r = H[r][v]), zero beyond n; with hosdx_ok only
    uint32_t *d_gen_G = nullptr;   // [ceil(k/32)][4][ceil(n/4)] G's columns packed over k, transposed for ldpc_gen_frames (ldpc_gen.hip)
    uint64_t *d_HcolsW = nullptr;  // [128][2] column v < n of H as given, rows 0..63 / 64..127, zero beyond n; with hosdw_ok only
    uint64_t *d_HcolsL = nullptr;  // [384][3] column v < n of H as given, rows 0..63 / 64..127 / 128..191, zero beyond n; with hosdl_ok only
    bool dpp_ror_up = true;       // probed: row_ror:n moves data towards higher lanes
    int dpp_wave_rol_dir = 0;      // probed: wave_rol:1 -- +1 lane j receives lane j-1, -1 lane j+1, 0 unusable
    bool osd_ok = false;
    bool hosd_ok = false;          // (128,64): ldpc_hosd_*
    bool hosdx_ok = false;         // 1 <= k <= 64, an H of exactly n - k <= 64 rows: ldpc_hosdx_*
    bool hosdw_ok = false;         // n <= 128, an H of 1 <= R <= 127 rows and rank 1 <= n - k <= 64: ldpc_hosdw_*
    bool hosdl_ok = false;         // n <= 384, an H of 1 <= R <= 192 rows, rank 1 <= n - k <= 192, 1 <= k <= 192: ldpc_hosdl_*
    void *osd_state = nullptr;    // ldpc::OsdState ((128,64) constants; per-stream workspaces behind its mutex)
    hipEvent_t *timing = nullptr;  // [LDPC_TIMING_SLOTS][6] events of ldpc_pipeline_run, created with the context
    unsigned timing_recorded[LDPC_TIMING_SLOTS] = {};   // bit i: event i of the slot was recorded by the last run that used it
};

namespace ldpc {

// host helpers (ldpc_host.cpp)
int gf2elim(int32_t *M, int m, int n, std::vector<int32_t> *swaps);  // returns rows left
int build_code(ldpc_code &c);  // fills G, graph tables, qc flag from c.H/m/n
int64_t tep_table(int k, int order, uint8_t *supports, int64_t *boundaries);
int64_t tep_table_fs(int k, int w, uint8_t *supports);
// (pack_osd_tables, which packs both into the context's tables: ldpc_osd_tables.h)
int64_t hosd_pattern_teps(int nseg, const int32_t *bounds, const int32_t *pattern, uint8_t *teps, int max_bound = 128);

// launchers (one per .hip file)
int launch_nms(ldpc_ctx *ctx, const float *d_llr, int64_t B, int T, const float *alpha, float w_in, float w_out,
               float *d_soft, float *d_traj, uint64_t *d_hard, uint8_t *d_fail, int kernel, hipStream_t st,
               const int32_t *d_index = nullptr, const int32_t *d_count = nullptr, float *d_rows = nullptr);
int probe_dpp(bool *ror_up, int *wave_rol_dir);
// NMS training forward + backward and the batch sums (ldpc_nms_train.hip); arguments validated by the caller
int launch_nms_train(ldpc_ctx *ctx, const float *d_llr, const uint64_t *d_label, int64_t B, int T, const float *alpha,
                     float w_in, float w_out, float *d_loss, float *d_grad, double *d_loss_sum, double *d_grad_sum,
                     float *d_traj, uint64_t *d_hard, uint8_t *d_fail, hipStream_t st);
// OSD (ldpc_osd.hip).  check_params runs first on every OSD entry point: the order, the algorithm and the flags
// (LDPC_OSD_F_*) against each other and against front_outside -- the caller supplies or wants the front-end results
// (ldpc_osd_search; ldpc_pipeline_run with d_perm and d_parity) -- before anything is launched.
int check_params(ldpc_ctx *ctx, const ldpc_osd_params *p, bool front_outside, const char *who);
// The kernel sequence of an OSD call; select_route reads the flags of params that check_params accepted.
enum class OsdRoute {
    Fused2r,        // conventional order 2, front end and scan in one kernel (osd_fused2r_kernel)
    Search2r,       // front end + osd_search2r_kernel (conventional order 2 on the caller's front-end results)
    Search2,        // front end + osd_search2_kernel (READLANE_SCAN, or no usable wave rotation)
    Table,          // front end + osd_search_kernel (orders 0, 1, 3; TABLE_SCAN at order 2)
    Fs,             // front end + osd_fs_kernel
    PbStaged,       // front end + the PB kernels (pb_mode 0 = staged, 1 = PB_BLOCK, 2 = PB_REPLAY)
    PbFrontInside,  // the PB kernels with the front end inside pb_singles_kernel (pb_mode 0 or 1)
};
struct OsdPlan {
    OsdRoute route;
    int pb_mode;
};
OsdPlan select_route(const ldpc_ctx *ctx, const ldpc_osd_params *p, bool front_outside);
// The OSD of ldpc_osd_search (d_perm, d_parity: the caller's front-end results) or of ldpc_osd_decode (both NULL) on
// validated params.  With d_label and d_counts, *counted tells whether the search kernel accumulated the counters of
// ldpc_osd_counts itself (the caller launches ldpc_osd_counts otherwise).
int osd_launch(ldpc_ctx *ctx, const float *d_y, const int32_t *d_index, const int32_t *d_count, int64_t F, const uint8_t *d_perm,
               const uint64_t *d_parity, const ldpc_osd_params *p, uint64_t *d_cw, float *d_metric, int32_t *d_best, int32_t *d_ntep,
               const uint64_t *d_label, int64_t *d_counts, hipStream_t s, bool *counted);
int eval_and_compact(ldpc_ctx *ctx, const uint64_t *d_hard, const uint64_t *d_label, const uint8_t *d_fail, int64_t B,
                     int64_t *d_counts, int32_t *d_index, int32_t *d_count, hipStream_t st);
// frame generator (ldpc_gen.hip): the context's packed G, and the launch on params that ldpc_gen_frames validated (B > 0)
int gen_ctx_init(ldpc_ctx *ctx);
void gen_ctx_release(ldpc_ctx *ctx);
int launch_gen(ldpc_ctx *ctx, const ldpc_gen_params *p, int64_t B, float *d_y, uint64_t *d_label_bits, hipStream_t st);

}  // namespace ldpc
