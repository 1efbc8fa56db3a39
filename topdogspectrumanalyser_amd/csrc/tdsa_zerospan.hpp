// tdsa_zerospan.hpp - launchers of zero span (tdsa_zerospan.hip): the detector ring, the
// trigger search over it and the view pass that reduces a display window to a trace and its statistics.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr long long kZsMinCapacity = 4;
constexpr long long kZsMaxCapacity = 1ll << 28;   // ring-relative indices and chunk lengths fit an int
constexpr int kZsMaxPoints = 16384;
constexpr int kZsMaxBlocks = 1024;                // workgroups of a view launch: one statistics partial each
constexpr int kZsBlockCell = 1024;                // cells of at least this many samples take a workgroup each, shorter ones a wave

// What the launches of one view share with the host, at the start of an allocation of its own.  The first 32 bytes
// are zeroed (one memset node) ahead of the launches: the counters the workgroups add to, and the trigger word.
struct ZsCtrl {
  unsigned long long n_ge;   // samples of the chunk >= level
  int n_rise, n_fall;        // crossings inside the chunk
  int trig;                  // trigger search: max over the hits of i + 1 (i ring-relative); 0 = no hit
  int pad[3];
  long long start;           // written by the view pass: absolute index of the chunk's first sample ...
  int triggered, pad2;       // ... and whether a trigger put it there
};
static_assert(sizeof(ZsCtrl) == 48, "ZsCtrl: 32 zeroed bytes, then the start");
constexpr size_t kZsCtrlZeroed = 32;

// one workgroup's share of the chunk statistics; the host folds them in block order
struct ZsPart {
  float mn, mx;   // np.min / np.max of the workgroup's samples: a NaN stays
  double sum;
};
static_assert(sizeof(ZsPart) == 16, "ZsPart");

constexpr size_t kZsOutOffset = sizeof(ZsCtrl) + size_t(kZsMaxBlocks) * sizeof(ZsPart);   // a multiple of 16

struct ZsPush {
  const void* in = nullptr;   // first sample of this contiguous piece
  float* out = nullptr;       // where it lands in the ring
  long long n = 0;
  int fmt = 0, detector = 0;
  float log_floor = 0.f, offset_db = 0.f;
};

struct ZsTrigger {
  const float* ring = nullptr;
  long long cap = 0;
  long long first = 0;        // absolute index of ring-relative pair ss
  long long ss = 0, n_pairs = 0;
  float level = 0.f;
  int fall = 0;
  ZsCtrl* ctrl = nullptr;
};

struct ZsView {
  const float* ring = nullptr;
  long long cap = 0;
  long long base = 0;         // absolute index of the oldest sample held
  long long free_start = 0;   // the start without a trigger hit
  int use_trig = 0;           // 1: ctrl->trig was filled by a trigger search
  int length = 0;             // samples of the chunk
  float level = 0.f;
  int columns = 0;            // 0: the chunk itself; P otherwise
  int col_detector = 0;
  ZsCtrl* ctrl = nullptr;
  ZsPart* part = nullptr;     // [blocks]
  float* out = nullptr;       // [length], [2][P] (MINMAX) or [P]
  int blocks = 0;             // set by zs_view_blocks
};

// one contiguous piece of a push (the caller splits at the physical wrap): head to a 16-byte store boundary, body, tail
hipError_t launch_zspan_push(const ZsPush& a, hipStream_t s);
hipError_t launch_zspan_trigger(const ZsTrigger& a, hipStream_t s);
int zs_view_blocks(const ZsView& a);
hipError_t launch_zspan_view(const ZsView& a, hipStream_t s);

}  // namespace tdsa
