// rt_dof.hip — the depth-RT_DOF_B instances of the thin-lens kernel (rt_sampled.hpp).  The Makefile compiles this file
// once per bounce depth (rt_dof_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#ifndef RT_DOF_B
#error "compile with -DRT_DOF_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_dof<RT_DOF_B>(const SampledLaunch& L) { return launch_dof_impl<RT_DOF_B>(L); }
}  // namespace rtk
