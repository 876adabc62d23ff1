// rt_converge_window.hip — the depth-RT_CONVERGE_WINDOW_B instances of the windowed converging render's kernel (rt_sampled.hpp).  The
// Makefile compiles this file once per bounce depth (rt_converge_window_b<B>.o), in parallel with the render kernels' units.
#include "rt_sampled.hpp"

#ifndef RT_CONVERGE_WINDOW_B
#error "compile with -DRT_CONVERGE_WINDOW_B=<bounce depth 0..7>"
#endif

namespace rtk {
template <>
hipError_t launch_converge_window<RT_CONVERGE_WINDOW_B>(const SampledLaunch& L) {
    return launch_converge_window_impl<RT_CONVERGE_WINDOW_B>(L);
}
}  // namespace rtk
