// The limits of the DL-OSD stage that host-only code checks as well (ldpc_dlosd_check.h, which builds without a device
// compiler): what the H-form scans keep in LDS and what the networks' weight blocks in the kernel arguments hold.
#pragma once

namespace ldpc {

constexpr int kHosdMaxBlocks = 1024;   // keys kept in LDS (8 KiB); the reference's paths have 30 blocks
constexpr int kSlideMaxWin = 15;       // window + the block index: at most 16 classifier inputs
constexpr int kDiaMaxL = 64;           // longest trajectory (T + 1) the weight block in the kernel arguments holds

// the weight counts of the sliding-window classifier for a window, and of the bit-wise CNN for trajectories of L rows
constexpr int fcn_weight_count(int win) { return (win + 1) * (win + 1) + 2 * (win + 1); }
constexpr int dia_weight_count(int L) { return 24 + 96 + 24 + 2 * (L - 6) + 1; }

}  // namespace ldpc
