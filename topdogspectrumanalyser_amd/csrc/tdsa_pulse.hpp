// tdsa_pulse.hpp - launcher of the pulse analysis (tdsa_pulse.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace tdsa {

constexpr int kPulseThreads = 256;
constexpr int kPulseSamplesPerThread = 16;            // c: consecutive samples a thread walks, kept in registers
constexpr int kPulseTile = kPulseThreads * kPulseSamplesPerThread;   // T = 4096 samples of one stream per workgroup pass
constexpr int kPulseMaxStreams = 256;                 // C, streams of a handle
constexpr int kPulseMaxLaunchTiles = 16384;           // tiles of a launch, all streams together, one workgroup each; a longer call is cut into launches
constexpr long long kPulseMaxRecords = 1ll << 22;     // streams * capacity
// the budget tests/test_pulse_kernel_resources.py pins from the compiler's remarks: no scratch, no spills, and
constexpr int kPulseVgprBudget = 128;                 // ... registers of a thread in each of the three kernels: four waves per SIMD,
constexpr int kPulseWorkgroupsPerCu = 4;              //     so that many workgroups of 256 threads on a CU
constexpr int kPulseLdsBudget = 4096;                 // ... bytes of LDS of a workgroup, far below what limits residency

// one pulse, as tdsa_pulse_read_pulses hands it back (include/tdsa_hip.h).  The kernels carry every partial run - a
// thread's, a tile's, the handle's open pulse - in the same struct.
struct PulseRecord {
  long long toa, width, peak_index;
  unsigned peak_bits, flags;
  double energy, acc_re, acc_im;
  unsigned long long reserved;
};
static_assert(sizeof(PulseRecord) == 64, "record layout");

// one stream's summary, as tdsa_pulse_read hands it back; the stitch kernel keeps it
struct PulseSummary {
  unsigned long long n_total, n_on, n_pulses, n_short, n_lost, n_nan;
  long long open_toa, open_width;
  int open, reserved;
};
static_assert(sizeof(PulseSummary) == 72, "summary layout");

// What a tile hands up: all that cannot be decided without the state coming in.  Classes: 0 = C or none, 1 = A, 2 = B.
struct PulseTileInfo {
  int first, last;          // class of the tile's first / last sample that is not C (0: the tile holds C samples only)
  int lead;                 // its leading C samples: on if the state coming in is
  int f_closed, has_t;      // F ends inside the tile; T exists
  int kept, n_short;        // pulses wholly inside the tile, behind F: kept, and dropped by min_width
  int n_on, n_nan;          // on samples behind the leading run; NaN powers
  int slot;                 // written by the stitch kernel: the slot of the tile's first interior pulse, at most capacity
  int reserved[2];
  PulseRecord L, F, T;      // the leading run (acc_* with the pair that enters F), the run from the first A sample to
};                          // the first B sample behind it, the run still on at the tile's end if that is not F
static_assert(sizeof(PulseTileInfo) == 48 + 3 * 64, "tile summary layout");

struct PulseLaunch {
  const void* in = nullptr;      // stream c at in + c * in_stride samples of the format
  int fmt = 0;                   // TDSA_IN_I8 / _U8 / _C64
  int C = 1;
  size_t n = 0;                  // samples per stream
  size_t in_stride = 0;
  long long base = 0;            // the index n of the call's first sample: the samples of a stream since the last reset
  float on_level = 1.0f, off_level = 1.0f;
  int min_width = 1;             // below 2^31
  int capacity = 1;
  int parity = 0;                // which of prev's two slots holds the sample before the call's first; flips per launch
  int max_launch_tiles = kPulseMaxLaunchTiles;   // lowered by tests only
  int passes = 7;                // bit k: launch pass k + 1 (tile, stitch, emit); tools/pulsebench.py times the shares
  PulseTileInfo* tiles = nullptr;     // [max_launch_tiles] scratch
  PulseSummary* sum = nullptr;        // [C]
  PulseRecord* open = nullptr;        // [C] the pulse not yet complete
  float2* prev = nullptr;             // [C][2] the stream's last sample, unpacked
  PulseRecord* records = nullptr;     // [C][capacity]
};

// cuts the call into launches of three kernels each on stream s; *launches (if not null) gets their number, by which
// the caller advances its parity
hipError_t launch_pulse(const PulseLaunch& a, hipStream_t s, int* launches);

}  // namespace tdsa
