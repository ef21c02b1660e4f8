// net_c4_layout.h — shape constants of the packed Connect4 bf16 net, shared by
// the fused forward that reads the fragments (net_c4.hip) and the device pack
// that writes them on a weight refresh (net_c4_pack.hip).
#pragma once
#include "c4.h"

namespace spai {
namespace c4net {

constexpr int kHid = 64;
constexpr int kKStepsRes = 18;             // 576 / 32
constexpr int kHeadC = 35;                 // 32 policy + 3 value channels
constexpr int kPolIn = 32 * c4::kCells;    // 1344
constexpr int kValIn = 3 * c4::kCells;     // 126
// Head features in LDS: H[s][cell*36 + c] (c < 35: 32 policy + 3 value channels,
// c = 35 is a zero pad), so the head conv's epilogue stores 4 channels of a cell
// as one 8-B word.  The fused linear runs over this cell-major K order (the host
// permutes the linear weights from the reference's c*42 + cell flatten to it).
constexpr int kHC = 36;                    // channels per cell in H
constexpr int kLinFeat = kHC * 42;         // 1512
constexpr int kLinK = 1536;                // padded to 48 k-steps of 32
constexpr int kLinKSteps = kLinK / 32;     // 48
// The fused linear has 8 outputs (7 logits + the value), so an MFMA B fragment
// of 16 columns would be half zeros.  The two K halves are packed into the 16
// columns instead: column n = (output n & 7, K half n >> 3), A row m =
// (position m & 7, K half m >> 3), and the diagonal blocks of D are the two
// halves' partial sums -- 24 k-steps and 24 KiB of weights, not 48.
constexpr int kLinHalves = 2;
constexpr int kLinBSteps = kLinKSteps / kLinHalves;   // B-fragment k-steps (1 KiB each)
constexpr int kMaxBlocks = 20;

}  // namespace c4net
}  // namespace spai
