// tdsa_sweep.hpp - launchers of the sweep assembler (tdsa_sweep.hip): the step detector that
// folds the dB rows of one tuning step into one trace, and the stitch that lays the steps' kept bins side by side and
// resamples them onto a fixed frequency grid.
#pragma once
#include <hip/hip_runtime.h>

namespace tdsa {

constexpr int kSweepMaxSteps = 4096;                 // the stitch keeps 16 bytes per step in LDS: 64 KiB
constexpr int kSweepMaxNfft = 1 << 20;
constexpr int kSweepMaxGrid = 1 << 24;
constexpr size_t kSweepChunkBytes = size_t(256) << 20;   // default bound of the row scratch of tdsa_sweep_run_dev

struct SweepDetLaunch {
  const float* rows = nullptr;     // step s, frame f, fftshift-ed bin k at rows[s * step_stride + f * nfft + k]
  long long step_stride = 0;       // floats
  int n_steps = 0, frames = 1, nfft = 0;
  int k0 = 0, k1 = 0;              // the kept range [k0, k1) of a row
  int detector = 0;                // TDSA_SWEEP_DET_*
  float* T = nullptr;              // [n_steps][k1 - k0], the first of the steps at T[0]
};
hipError_t launch_sweep_detector(const SweepDetLaunch& a, hipStream_t s);

struct SweepStitchLaunch {
  const double2* tab = nullptr;    // [n_present] (frequency of the first kept bin, centre) of the steps present, ascending
  const int* step_of = nullptr;    // [n_present] their step numbers
  int n_present = 0;
  int K = 0, koff = 0;             // kept bins per step; k0 - nfft / 2: kept bin k of a step lies at centre + (koff + k) bin_hz
  double bin_hz = 0.0;
  const float* T = nullptr;        // [n_steps][K]
  const double* grid = nullptr;    // [n_grid]
  int n_grid = 0;
  double h = 0.0;                  // grid[1] - grid[0] (peak mode)
  int mode = 0;                    // TDSA_SWEEP_INTERP / _PEAK
  double* out = nullptr;           // [n_grid]
};
hipError_t launch_sweep_stitch(const SweepStitchLaunch& a, hipStream_t s);

}  // namespace tdsa
