// The traits of the long / low-rate family for the host paths of ldpc_osd_family.h.  The family's kernels are instantiations
// chosen by the shape, and they live in three translation units, each with its own code object: the front end and the
// conventional scan in ldpc_osdl.hip, FS-OSD and the one-TEP kernel in ldpc_osdl_fs.hip, PB-OSD in ldpc_osdl_pb.hip.  So the five selectors are declared
// here with their kernel types written out and each is defined beside its kernels; ldpc_osdl_fs_decode and ldpc_osdl_pb_decode
// take the front end from ldpc_osdl.hip through front(t), and nothing is instantiated twice.
#pragma once

#include "ldpc_osdl.h"
#include "ldpc_osd_family.h"
#include "ldpc_pbx.h"

namespace ldpc {

struct Osdl {
    using perm_t = uint16_t;
    using front_fn = void (*)(const float *, const int *, const int *, long long, int, int, const u64 *, unsigned short *, u64 *, int *);
    using search_fn = void (*)(const float *, const int *, const int *, long long, int, int, const unsigned short *, const u64 *, const uchar4 *,
                               int, u64 *, float *, int *, int *, const u64 *, u64 *);
    using fs_fn = void (*)(const float *, const int *, const int *, long long, int, int, const unsigned short *, const u64 *, const uchar4 *,
                           FsParams, u64 *, float *, int *, int *, const u64 *, u64 *);
    using tep_eval_fn = void (*)(const float *, const int *, const int *, long long, int, int, const unsigned short *, const u64 *, const u64 *,
                                 u64 *, float *, int *);
    using pb_fn = void (*)(const float *, const int *, const int *, long long, int, int, const unsigned short *, const u64 *, const double *,
                           PbxParams, u64 *, float *, int *, int *, int *, const u64 *, u64 *);
    static const OsdlTables &tables(const ldpc_ctx *ctx) { return ctx->osdl_tables; }
    static constexpr const char *needs = kOsdlNeeds;
    static front_fn front(const OsdlTables &t);         // ldpc_osdl.hip: S = ceil(n / 64) rounded up to 2, 4 or 6 slots, W = ceil(k / 64) row words
    static search_fn search(const OsdlTables &t);       // ldpc_osdl.hip: Wp = ceil((n - k) / 64) words of discrepancy
    static fs_fn fs(const OsdlTables &t);               // ldpc_osdl_fs.hip: Wp
    static tep_eval_fn tep_eval(const OsdlTables &t);   // ldpc_osdl_fs.hip: Wp
    static pb_fn pb(const OsdlTables &t, int order);    // ldpc_osdl_pb.hip: Wp, and the slot tier of the order and k
};

}  // namespace ldpc
