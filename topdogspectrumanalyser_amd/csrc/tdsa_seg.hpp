// tdsa_seg.hpp - the constants the segment analysers (symbol recovery, tdsa_symsync.hpp; FSK analysis, tdsa_fsk.hpp)
// share: a workgroup per segment, the symbol clock in 32.32 fixed point.  Their kernels' common code is tdsa_seg_block.hpp.
#pragma once
#include <cstdint>

namespace tdsa {

constexpr int kSegThreads = 256;                     // one workgroup per segment
constexpr int kSegMaxSymbols = 4096;                 // K per segment
constexpr int kSegNcoTable = 4096;                   // the rotation's table: the top 12 phase bits
constexpr uint64_t kSegOne = uint64_t(1) << 32;      // one sample in 32.32
constexpr uint64_t kSegMinStep = 4 * kSegOne, kSegMaxStep = 64 * kSegOne;   // samples per symbol

}  // namespace tdsa
