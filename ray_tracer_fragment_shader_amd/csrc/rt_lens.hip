// rt_lens.hip — the depth-RT_LENS_B instances of one kind of the lens kernel (rt_sampled.hpp): RT_LENS_KIND 0 depth of
// field, 1 soft shadows (AREA), 2 motion blur (AREA, MOTION).  The Makefile compiles this file once per bounce depth and
// kind (rt_lens_k<kind>_b<B>.o), in parallel with the render kernels' translation units.
#include "rt_sampled.hpp"

#if !defined(RT_LENS_B) || !defined(RT_LENS_KIND)
#error "compile with -DRT_LENS_B=<bounce depth 0..7> -DRT_LENS_KIND=<0 dof, 1 soft, 2 motion>"
#endif

namespace rtk {
template <>
hipError_t launch_lens<RT_LENS_B, (RT_LENS_KIND >= 1), (RT_LENS_KIND >= 2)>(const SampledLaunch& L) {
    return launch_lens_impl<RT_LENS_B, (RT_LENS_KIND >= 1), (RT_LENS_KIND >= 2)>(L);
}
}  // namespace rtk
