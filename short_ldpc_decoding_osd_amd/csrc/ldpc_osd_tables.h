// The OSD tables of a context (host side): G columns, the conventional TEP table, the FS visit-order table of the code's k and
// the code-only constants of the any-shape PB-OSD kernel.
// ONE set per context, for every code with 1 <= k <= 64 and 1 <= n - k <= 64: the (128,64) kernels (ldpc_osd.hip,
// ldpc_osd_pb.hip) and the any-shape kernels (ldpc_osdx.hip) read the same device copies.  Packed by pack_osd_tables
// (ldpc_host.cpp), uploaded by ldpc_ctx_create and freed by ldpc_ctx_destroy (ldpc_api.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/ldpc_osd.h"

namespace ldpc {

typedef unsigned long long u64;   // (as ldpc_wave.h; this header is also part of the host-only build, which has no ldpc_wave.h)

struct OsdTables {
    int n = 0, k = 0;            // the shape the tables were built for; k = 0: no tables (the OSD entry points report UNSUPPORTED)
    u64 *d_Gcols = nullptr;      // [n] column v of G as a k-bit word (bit r = G[r][v])
    uchar4 *d_tep = nullptr;     // conventional order-3 TEP table of this k: (i, j, l, weight); order o is the prefix of ntep[o] entries
    int64_t ntep[4] = {0, 0, 0, 0};
    uchar4 *d_tep_fs = nullptr;  // FS-OSD visit order (generate_sequential_teps) of this k: weight classes 1..min(3, k) back to back
    int fs_off[4] = {0, 0, 0, 0}, fs_cnt[4] = {0, 0, 0, 0};   // weight class w: offset / count inside d_tep_fs
    double *d_pb = nullptr;      // PB-OSD of ldpc_osdx_pb.h / ldpc_osdw_pb.h (layout: ldpc_pbx.h): [65] P[Bin(n-k, 1/2) <= b], then [64] (n-k-i)/(i+1) and [64] (k-i)/(i+1)
};

// the host images of the device tables
struct OsdTablesHost {
    std::vector<u64> Gcols;
    std::vector<uchar4> tep, tep_fs;
    std::vector<double> pb;
};

// For a code with 1 <= k <= 64, 1 <= n - k <= 64 and G = [k][n]: fills `host` and the shape, boundaries, offsets and counts
// of `t` (never a device pointer).  Any other code leaves t.k = 0.  LDPC_OK, or the error of tep_table / tep_table_fs.
// Pure host code (ldpc_host.cpp).
int pack_osd_tables(const ldpc_code &c, OsdTables &t, OsdTablesHost &host);

// The tables of the high-rate family (ldpc_osdw.hip): every code with n <= 128 and 1 <= n - k <= 64, hence k up to 127.  A member
// of its own in the context, so that OsdTables::k -- and with it ldpc_osdx_supported -- stays 0 for k > 64.
struct OsdwTables {
    int n = 0, k = 0;            // the shape the tables were built for; k = 0: no tables (ldpc_osdw_* report UNSUPPORTED)
    u64 *d_Gcols = nullptr;      // [n][2] column v of G as two words: bit r of word 0 = G[r][v], bit r of word 1 = G[64 + r][v]
    uchar4 *d_tep = nullptr;     // conventional order-3 TEP table of this k; for k <= 64 it IS OsdTables::d_tep (one device copy)
    bool own_tep = false;        // d_tep, d_tep_fs and d_pb were allocated for this member (k > 64) and are freed with it
    int64_t ntep[4] = {0, 0, 0, 0};
    uchar4 *d_tep_fs = nullptr;  // FS-OSD visit order of this k, weight classes 1..min(3, k) back to back; for k <= 64 it IS OsdTables::d_tep_fs
    int fs_off[4] = {0, 0, 0, 0}, fs_cnt[4] = {0, 0, 0, 0};   // weight class w: offset / count inside d_tep_fs
    double *d_pb = nullptr;      // PB-OSD (ldpc_osdw_pb.h), the layout of OsdTables::d_pb; for k <= 64 it IS OsdTables::d_pb
};

struct OsdwTablesHost {
    std::vector<u64> Gcols;      // [n][2]
    std::vector<uchar4> tep;     // filled only where `base` has no table of this k (k > 64)
    std::vector<uchar4> tep_fs;  // likewise (341 503 entries, 1.37 MB, at k = 127)
    std::vector<double> pb;      // likewise (193 entries)
};

// For a code with n <= 128, 1 <= n - k <= 64, k >= 1 and G = [k][n]: fills `host` and the shape, boundaries, offsets and counts
// of `t` (never a device pointer; t.own_tep tells whether host.tep, host.tep_fs and host.pb were filled).  `base`: the OsdTables already
// packed for the same code.  Any other code leaves t.k = 0.  LDPC_OK, or the error of tep_table / tep_table_fs.  Pure host code
// (ldpc_host.cpp).
int pack_osdw_tables(const ldpc_code &c, const OsdTables &base, OsdwTables &t, OsdwTablesHost &host);

// The tables of the long / low-rate family (ldpc_osdl.hip): every code with n <= 384, 1 <= k <= 192 and 1 <= n - k <= 192.  A
// member of its own in the context, as OsdwTables is; it holds the tables of the conventional scan and of FS-OSD and the PB constants.
// The PB table of this family (float64, m = n - k <= 192): cdfH[193] = P[Bin(m, 1/2) <= b] (zero beyond m), then the ratios of
// consecutive binomial coefficients (m - i) / (i + 1), 192 entries (zero beyond m - 1), and (k - i) / (i + 1), the first 64
// (zero beyond k - 1; the kernel reads the entries i < order <= 3).  The kPbx* layout of the older families (ldpc_pbx.h) is another.
constexpr int kPblCdfH = 0, kPblCoefM = 193, kPblCoefK = 385, kPblTabSize = 449;
struct OsdlTables {
    int n = 0, k = 0;            // the shape the tables were built for; k = 0: no tables (ldpc_osdl_* report UNSUPPORTED)
    u64 *d_Gcols = nullptr;      // [n][W] column v of G as W = ceil(k / 64) words: bit r of word w = G[64 w + r][v]
    uchar4 *d_tep = nullptr;     // conventional order-3 TEP table of this k; where OsdwTables serves the code it IS OsdwTables::d_tep
    bool own_tep = false;        // d_tep and d_tep_fs were allocated for this member and are freed with it
    int64_t ntep[4] = {0, 0, 0, 0};
    uchar4 *d_tep_fs = nullptr;  // FS-OSD visit order of this k, weight classes 1..min(3, k) back to back; where OsdwTables serves the code it IS OsdwTables::d_tep_fs
    int fs_off[4] = {0, 0, 0, 0}, fs_cnt[4] = {0, 0, 0, 0};   // weight class w: offset / count inside d_tep_fs
    double *d_pb = nullptr;      // PB-OSD (ldpc_osdl_pb.h), the kPbl* layout; always this member's own
};

struct OsdlTablesHost {
    std::vector<u64> Gcols;      // [n][W]
    std::vector<uchar4> tep;     // filled only where `base` has no table of this k (1 179 809 entries, 4.7 MB, at k = 192)
    std::vector<uchar4> tep_fs;  // likewise (1 179 808 entries, 4.7 MB, at k = 192)
    std::vector<double> pb;      // [kPblTabSize], for every code the family serves
};

// For a code with n <= 384, 1 <= k <= 192, 1 <= n - k <= 192 and G = [k][n]: fills `host` and the shape, boundaries, offsets and
// counts of `t` (never a device pointer; t.own_tep tells whether host.tep and host.tep_fs were filled).  `base`: the OsdwTables
// already packed for the same code.  Any other code leaves t.k = 0.  LDPC_OK, or the error of tep_table / tep_table_fs.  Pure
// host code (ldpc_host.cpp).
int pack_osdl_tables(const ldpc_code &c, const OsdwTables &base, OsdlTables &t, OsdlTablesHost &host);

// The PB table of the long / low-rate family for 1 <= k <= 192 and 1 <= m = n - k <= 192 (the kPbl* layout above): cdfH by the
// float64 pmf recurrence of pack_pb_table -- q^m by left-to-right square-and-multiply, ratio p / q = 1.  Pure host code.
void pack_osdl_pb_table(int n, int k, std::vector<double> &pb);

// The kernel argument of osd_fs_kernel / osdx_fs_kernel / osdw_fs_kernel / osdl_fs_kernel (FsParams: ldpc_search.h) from the
// caller's parameters and the shape, class offsets and class counts of the context's FS table (OsdTables, OsdwTables or OsdlTables: fs_off / fs_cnt);
// beta_term = (float)((double)fs_beta * (double)(n - k)) (fs_testing.py:138).  Defined in ldpc_osd.hip.
struct FsParams;
FsParams fs_params(const ldpc_osd_params *p, int n, int k, const int (&fs_off)[4], const int (&fs_cnt)[4]);

}  // namespace ldpc
