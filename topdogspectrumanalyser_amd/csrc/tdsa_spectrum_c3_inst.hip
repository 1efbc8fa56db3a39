// tdsa_spectrum_c3_inst.hip - the 16384-point frame kernel with the sliding front end (SLIDE, tdsa_spectrum_kernel.hpp):
// byte formats, dB rows, hop N/2, hold off / max hold.  Instantiations and an object of their own: the ones
// tdsa_spectrum_inst.hip makes keep their names and their instruction streams (tests/test_isa_frozen.py), and a change
// to this front end lands here without touching them.
#include "tdsa_spectrum_kernel.hpp"

namespace tdsa {
hipError_t launch_c3_slide(const SpecParams& p, const LaunchGeom& g, hipStream_t s) {
  return (p.hold_flags & 1) ? launch_one<14, false, 16 | 1>(p, g, s) : launch_one<14, false, 16>(p, g, s);
}
}  // namespace tdsa
