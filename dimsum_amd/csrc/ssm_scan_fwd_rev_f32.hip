// selective-scan forward, f32 I/O: the time-reversed kernels of the bidirectional scan (64-channel and one-lane-per-state: kRev / kAcc).
// A translation unit of its own like ssm_scan_fwd_f32.hip (the scheduled inner blocks make every instantiation slow to compile).
#include "ssm_scan_fwd_kernel.hpp"
#include "ssm_scan_fwd_lanes.hpp"

namespace dimsum {
DIMSUM_INSTANTIATE_FWD_REV(float)
DIMSUM_INSTANTIATE_FWD_LANES_REV(float)
}  // namespace dimsum
