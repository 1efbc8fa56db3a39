// tdsa_history.hpp - launchers of the 3-D history views (tdsa_history.hip): the push pass into
// the trace ring, the screen reduction, and the ribbon / line-stack / surface passes that turn rows into what the
// displays draw.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr long long kHistMaxCells = 1ll << 28;   // depth * n_bins: ring indices fit an int
constexpr int kHistRibbonRows = 30;
constexpr int kHistHues = 11;
constexpr int kHistNeverPushed = 255;            // colour index of a line no row has reached: RGBA 0
constexpr int kHistPushMaxWgs = 2048;            // workgroups of one push; more rows than 2048 / (column pieces): row chunks

// Rows of a view, newest first.  linear = 0: row r of the view is ring slot (head - 1 - first - r) mod depth;
// linear = 1: `base` is [rows][n] already in view order (the output of the reduction).
struct HistSrc {
  const float* base = nullptr;
  int n = 0, depth = 1, head = 0, first = 0, linear = 0;
};

struct HistPush {
  const float* in = nullptr;        // [n_rows][n] dB rows
  const float* hold_in = nullptr;   // optional max trace [n] (n_rows == 1): the hold follows it instead of the row
  const float* min_in = nullptr;    // optional min trace [n] (n_rows == 1)
  float* ring = nullptr;            // [depth][n]
  float* hold = nullptr;            // [n] heights only; z >= 0, so the maximum is an integer maximum of the bits
  float* min_out = nullptr;         // [n]
  unsigned long long* keys = nullptr;   // [depth] per slot: (orderable maximum << 32) | ~first index, zeroed by the caller
  int n = 0, depth = 1, head = 0, n_rows = 0;
  int skip = 0;                     // rows below this one are older than the ring is deep: they only reach the hold
  int heights = 1, update_hold = 1;
  float bottom = -100.f, range = 100.f, zscale = 8.f;
  int rows_per_wg = 1;
};

struct HistReduce {
  HistSrc src;
  int rows = 0, columns = 0;
  float* vals = nullptr;            // [rows][columns]
  int* bins = nullptr;              // [rows][columns]
};

struct HistRibbonRow {
  float y_front, y_back, hue_scale, alpha;
  double val;
};

struct HistRibbon {
  HistSrc src;
  int rows = 0;
  const float* x = nullptr;         // [n_bins]
  const int* bins = nullptr;        // reduced views: [rows][src.n] bin of each column (x is gathered through it)
  float* verts = nullptr;           // [rows][2 n][3]
  float* colours = nullptr;         // [rows][2 n][4]
  HistRibbonRow row[kHistRibbonRows];
};

struct HistLines {
  HistSrc src;
  int rows = 0;
  int valid = 0;                    // view rows at or beyond this one were never pushed
  int rgba = 0;
  float* z = nullptr;               // [rows][n]
  void* colours = nullptr;          // uint8 [rows][n] or float [rows][n][4]
  float palette[kHistHues][4];
};

struct HistSurface {
  HistSrc src;
  int rows = 0, flat = 0;           // flat: zmax == zmin, 0.5 everywhere
  double zmin = -100.0, span = 100.0;
  float* z = nullptr;               // [rows][n]
  float* colours = nullptr;         // [rows][n][3]
};

hipError_t launch_hist_push(const HistPush& a, hipStream_t s);
hipError_t launch_hist_reduce(const HistReduce& a, hipStream_t s);
hipError_t launch_hist_ribbon(const HistRibbon& a, hipStream_t s);
hipError_t launch_hist_lines(const HistLines& a, hipStream_t s);
hipError_t launch_hist_surface(const HistSurface& a, hipStream_t s);

// (value, first index) of a slot key; an untouched key (0) reads as (0, 0)
inline void hist_key_decode(unsigned long long key, float* value, int* index) {
  if (key == 0) {
    *value = 0.f;
    *index = 0;
    return;
  }
  unsigned hi = unsigned(key >> 32);
  hi = (hi & 0x80000000u) ? hi ^ 0x80000000u : ~hi;
  __builtin_memcpy(value, &hi, 4);
  *index = int(~unsigned(key & 0xffffffffu));
}

}  // namespace tdsa
