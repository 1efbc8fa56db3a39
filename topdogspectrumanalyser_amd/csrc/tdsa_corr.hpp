// tdsa_corr.hpp - launcher of the correlation search (tdsa_corr.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tdsa {

constexpr int kCorrThreads = 256;
constexpr int kCorrWindowsPerThread = 8;              // R: consecutive windows a thread of the correlate pass keeps in registers (L > kCorrShortRef)
constexpr int kCorrShortWindowsPerThread = 4;         // ... and for a reference of at most
constexpr int kCorrShortRef = 128;                    // ... samples, with packed multiply-adds: the faster of the two there (profiles/corrbench.txt)
constexpr int kCorrTile = kCorrThreads * kCorrWindowsPerThread;   // T = 2048 windows of one stream per workgroup of the correlate pass at R = 8; the unit a call is cut into launches by
constexpr int kCorrBlock = 256;                       // B: windows of a block of the match passes, one per thread; blocks lie on multiples of B
constexpr int kCorrBlocksPerWorkgroup = 8;            // blocks a workgroup of the block-maxima and the count pass walks through
constexpr int kCorrMaxStreams = 256;                  // C, streams of a handle
constexpr int kCorrMinRef = 2;
constexpr int kCorrMaxRef = 1024;                     // L, samples of the reference
constexpr int kCorrMaxDistance = 65536;               // W, min_distance
constexpr int kCorrMaxLaunchTiles = 1024;             // tiles of T windows in a launch, all streams together; a longer call is cut into launches
constexpr long long kCorrMaxRecords = 1ll << 22;      // streams * capacity
constexpr long long kCorrTraceBytes = 1ll << 28;      // the trace of all streams stays within 256 MiB of the ring
constexpr int kCorrRingEntryBytes = 24;               // m, e, c1, c2 of a window
// the budget tests/test_corr_kernel_resources.py pins from the compiler's remarks: no scratch, no spills, and
constexpr int kCorrVgprBudget = 128;                  // ... registers of a thread in every kernel: four waves per SIMD
constexpr int kCorrLdsBudget = 38912;                 // ... bytes of LDS of a workgroup of the correlate pass at R <= 8, the reference staged too: four on a CU
constexpr int kCorrLdsBudgetWide = 81920;             // ... and of its widest variant (R = 16), which tools/corrbench.py times
constexpr int kCorrMatchLdsBudget = 1024;             // ... of a workgroup of the block-maxima, count and emit passes
constexpr int kCorrScanLdsBudget = 2048;              // ... and of the scan pass, which unpacks the history: the uint8 table and four partial sums

// one match, as tdsa_corr_read hands it back (include/tdsa_hip.h)
struct CorrRecord {
  long long index;
  float metric, energy;
  float c1_re, c1_im, c2_re, c2_im;
};
static_assert(sizeof(CorrRecord) == 32, "record layout");

// one stream's summary, as tdsa_corr_read hands it back; the scan pass keeps it
struct CorrSummary {
  unsigned long long n_total, n_windows, n_decided, n_matches, n_lost, n_bad;
  int flushed, reserved;
};
static_assert(sizeof(CorrSummary) == 56, "summary layout");

// One launch: n samples per stream that begin at sample s0 of the stream complete the windows w0 .. w1 - 1, and the
// windows d0 .. d1 - 1 are decided with the right-hand range clipped at w1 - 1.  The ring holds window n of stream c at
// entry n & ring_mask of the stream's ring_mask + 1.
struct CorrLaunch {
  const void* in = nullptr;      // stream c at in + c * in_stride samples of the format
  int fmt = 0;                   // TDSA_IN_I8 / _U8 / _C64
  int C = 1;
  int n = 0;                     // samples per stream of the launch
  size_t in_stride = 0;
  long long s0 = 0, w0 = 0, w1 = 0, d0 = 0, d1 = 0;
  int L = 2, W = 2;
  float threshold = 1.0f, e_ref = 1.0f;
  int capacity = 1;
  int parity = 0;                // which of the two history slots holds the L - 1 samples before s0; flips per launch with samples
  int flush = 0;                 // the launch of tdsa_corr_flush: no samples, the streams end
  int max_launch_tiles = kCorrMaxLaunchTiles;   // lowered by tests only
  int passes = 15;               // bit 0: correlate, 1: block maxima and count, 2: scan, 3: emit; tools/corrbench.py times the shares
  int variant = 0;               // of the correlate pass.  0 as shipped: 4 for L <= kCorrShortRef, else 6.  1 .. 5: R = 4, 8, 16, then R = 4, 8 packed,
                                 // the reference through scalar loads; 6, 7: R = 8, then R = 8 packed, the reference in LDS
  unsigned ring_mask = 0;
  const float2* ref = nullptr;   // [L]
  float2* hist = nullptr;        // [2][C][kCorrMaxRef] the last L - 1 samples of a stream, unpacked, at the front of its row
  float* ring_m = nullptr;       // [C][ring] m
  float* ring_e = nullptr;       // [C][ring] e
  float4* ring_c = nullptr;      // [C][ring] c1, c2
  unsigned* bmax = nullptr;      // [C][blocks] scratch: the largest m of a block, as bits
  int* tile_cnt = nullptr;       // [C][blocks] scratch: matches of a block, then the slot of its first
  unsigned long long* tile_bits = nullptr;   // [C][blocks][4] scratch: which of a block's windows match
  int blocks = 0;                // per stream, what the three scratch arrays have room for
  unsigned n_reach = 0, n_decide = 0;   // set by the launcher: blocks a decision of the launch can reach, blocks with a window to decide
  CorrSummary* sum = nullptr;    // [C]
  CorrRecord* records = nullptr; // [C][capacity]
};

// the kernels of one launch on stream s
hipError_t launch_corr(const CorrLaunch& a, hipStream_t s);

}  // namespace tdsa
