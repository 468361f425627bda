// gate_kernels.hip -- a translation unit with nothing but the gate kernels that request their states early (mfma_fused_body.inc
// EARLY), for tools/check_vmwait.py --gate: seconds to compile instead of the library's minutes.  The same headers, the same
// template arguments as s5fxp_fast.hpp gate_fold_kernel() / cgate_kernel() at KS = 1.
#include "../include/s5fxp.h"
#include "../sparsernns_amd/csrc/s5fxp_kernels.hpp"
#include "../sparsernns_amd/csrc/mfma_fused.hpp"
using namespace s5;
template __global__ void s5::k_cgate_p<1, 3, false, true, true, 32, false, true, true, false, true>(const CGateFoldArgs, GroupOff);
template __global__ void s5::k_cgate_p<1, 3, false, true, true, 32, false, false, true, false, true>(const CGateFoldArgs, GroupOff);
template __global__ void s5::k_cgate_p<1, 3, false, true, true, 32, false, true, true, false, true>(const CGateArgs, GroupOff);
template __global__ void s5::k_cgate_p<1, 3, false, true, true, 32, false, false, true, false, true>(const CGateArgs, GroupOff);
