// rt_dof.hpp — the thin-lens (depth of field) kernel of rt_render_dof_dev (include/rt_api.h, ABI 10): S x S rays per
// pixel, each from its own point of a square lens around the eye to its own sub-pixel point of the focal plane,
// reduced in the wave.
//
// One launch, no per-view state.  Its instances live in rt_dof.hip, compiled once per bounce depth (rt_dof_b<B>.o),
// so the render kernels' and the refine kernels' translation units are not touched.
#pragma once

#include "rt_render.hpp"

namespace rtk {

constexpr int kDofGridY = 32768;               // tile rows per grid.z slice (grid.y and grid.z stay below 65536)

// One-wave workgroups; a wave owns one 8 x 8 block of the SAMPLE grid — an (8 / S) x (8 / S) tile of output pixels —
// with lane bits 0..2 = x and bits 3..5 = y, as render_body's supersampled instances: lane (x, y) holds sample
// (a, b) = (x mod S, y mod S) of output pixel (8 tx / S + x / S, 8 ty / S + y / S), so the xor butterfly with partners
// 1 .. S/2, then 8 .. 8 S/2, is the contract's fixed pairwise tree (first along a, then along b), and the lanes of a
// wave trace neighbouring pixels (the coherence the scattered refine kernel of rt_adaptive.hpp lacks).
//
// P describes the sample grid (camera rt_camera_supersample, width = S x the output's): the ray's end sp_s is formed
// by exactly the operations of render_body; its start is the lens point
//     e(a, b) = (eye + (A t_a) right) + (A t_b) up',   t_a = (2 a + 1 - S) / S,
// one IEEE operation per parenthesis and component, in this order.  The rays of a wave have different origins, so
// there is no primary cone mask and there are no level masks: they take the generic path of rt_trace_rays_kernel
// (trace<B, false, TRANSP, false> / trace_tree<B>) with hits_ok_from(e) per lane.  A = 0 and S = 1 run this same code.
//
// trace() reduces over the whole wave, so every lane stays active: the sample frame is S times the output, and S
// divides 8, so an S x S block lies wholly inside the sample frame or wholly outside it; lanes outside (and the
// padding tile rows of the last grid.z slice) trace a clamped in-frame sample and store nothing.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_dof_kernel(const DevScene* __restrict__ S, RenderParams P, double aperture,
                                                    int tile_rows, void* o32, void* o8, double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int s = P.ss_log2, S1 = (1 << s) - 1;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    double* slot = reinterpret_cast<double*>(smem) + lane;
    int* mslot = reinterpret_cast<int*>(smem + 3 * 8 * colour_slots(B, TRANSP) * 64) + lane;
    const int x = lane & 7, y = lane >> 3;
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    const int i = tx * 8 + x, lr = ty * 8 + y;
    const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    // Ray end, as render_body forms the primary ray's
    const d3 sp = add(add(ld3(P.look), scl(P.pitch * (double)(ic + P.bottom_x), right)),
                      scl(P.pitch * (double)(j + P.bottom_y), upp));
    // Ray start: t = (2 a + 1 - S) / S, an exact quotient (S is a power of two: the product with 2^-s is the same bits)
    const double inv_s = ldexp(1.0, -s);
    const double ta = (double)(2 * (x & S1) - S1) * inv_s, tb = (double)(2 * (y & S1) - S1) * inv_s;
    const d3 e = add(add(ld3(P.eye), scl(aperture * ta, right)), scl(aperture * tb, upp));
    V.hits_ok = hits_ok_from(S, e);
    uint32_t seg = 0, sh = 0;
    d3 col;
    if constexpr (TREE)
        col = trace_tree<B>(V, e, sp, &seg, &sh);
    else
        col = trace<B, false, TRANSP, false, 64>(V, e, sp, ~0ull, &seg, &sh, slot, mslot);
    for (int m = 1; m <= S1; m <<= 1) {                     // along a; every lane active
        col.x += __shfl_xor(col.x, m);
        col.y += __shfl_xor(col.y, m);
        col.z += __shfl_xor(col.z, m);
        seg += __shfl_xor(seg, m);
        sh += __shfl_xor(sh, m);
    }
    for (int m = 8; m <= 8 * S1; m <<= 1) {                 // along b
        col.x += __shfl_xor(col.x, m);
        col.y += __shfl_xor(col.y, m);
        col.z += __shfl_xor(col.z, m);
        seg += __shfl_xor(seg, m);
        sh += __shfl_xor(sh, m);
    }
    col = scl(ldexp(1.0, -2 * s), col);                     // 1.0 / (S * S), exact
    if ((x & S1) == 0 && (y & S1) == 0 && i < P.width && lr < P.height && !pad) {
        const size_t k = (size_t)(lr >> s) * (size_t)(P.width >> s) + (size_t)(i >> s);
        store_pixel<false>(P, k, col, o32, o8);
        if (o64) { o64[3 * k] = col.x; o64[3 * k + 1] = col.y; o64[3 * k + 2] = col.z; }
        if (orc2) { orc2[2 * k] = seg; orc2[2 * k + 1] = sh; }
    }
}

struct DofLaunch {
    int variant;                               // 0 opaque, 1 FULL (meshes / transparent materials), 2 ray trees
    hipStream_t stream;
    const DevScene* scene;
    RenderParams P;                            // the sample grid's (ss_log2 set)
    double aperture;                           // half-width of the lens
    void* o32;
    void* o8;
    double* o64;
    uint32_t* orc2;
};

// Defined once per depth B in rt_dof_b<B>.o (rt_dof.hip).
template <int B>
hipError_t launch_dof(const DofLaunch& L);
#define RT_DECLARE_DOF(B) \
    template <>           \
    hipError_t launch_dof<B>(const DofLaunch& L);
RT_DECLARE_DOF(0) RT_DECLARE_DOF(1) RT_DECLARE_DOF(2) RT_DECLARE_DOF(3)
RT_DECLARE_DOF(4) RT_DECLARE_DOF(5) RT_DECLARE_DOF(6) RT_DECLARE_DOF(7)
#undef RT_DECLARE_DOF

template <int B>
hipError_t launch_dof_impl(const DofLaunch& L) {
    if constexpr (B > RT_MAX_B) {
        return hipErrorInvalidValue;
    } else {
        const int tiles_x = (L.P.width + 7) / 8, tile_rows = (L.P.height + 7) / 8;
        const dim3 g((unsigned)tiles_x, (unsigned)std::min(tile_rows, kDofGridY),
                     (unsigned)((tile_rows + kDofGridY - 1) / kDofGridY)), w(64);
        if (L.variant == 2)
            hipLaunchKernelGGL((rt_dof_kernel<B, true, true>), g, w, 0, L.stream, L.scene, L.P, L.aperture, tile_rows,
                               L.o32, L.o8, L.o64, L.orc2);
        else if (L.variant == 1)
            hipLaunchKernelGGL((rt_dof_kernel<B, true, false>), g, w, slot_bytes(B, true, 64), L.stream, L.scene, L.P,
                               L.aperture, tile_rows, L.o32, L.o8, L.o64, L.orc2);
        else
            hipLaunchKernelGGL((rt_dof_kernel<B, false, false>), g, w, slot_bytes(B, false, 64), L.stream, L.scene,
                               L.P, L.aperture, tile_rows, L.o32, L.o8, L.o64, L.orc2);
        return hipGetLastError();
    }
}

}  // namespace rtk
