// rt_adaptive.hpp — the refine kernel of adaptive supersampling (rt_render_adaptive_dev, include/rt_api.h): the
// S x S samples of the pixels on a compacted work list, S x S lanes per pixel, reduced in the wave.
//
// rt_render_adaptive_dev runs three passes on one stream: the one-sample base render (the existing render kernels),
// rt_classify_kernel (rt_kernel.hip: the contrast criterion on the base bytes, `refined`, and the work list of
// flagged pixel indices behind a device counter), then this kernel.  Its instances live in rt_adaptive.hip, compiled
// once per bounce depth (rt_adaptive_b<B>.o), so the render kernels' translation units are not touched.
#pragma once

#include "rt_render.hpp"

namespace rtk {

// One-wave workgroups; a fixed grid (the pixel count is only known on the device) walks the list with a grid-stride
// loop.  A wave takes 64 / S^2 listed pixels per step: lane l traces sample (a, b) of the pixel of its group
// l >> 2 log2 S, a = the low log2 S bits of l, b the next log2 S — so the xor butterfly with partners 1 .. S/2, then
// S .. S S/2, is the fixed pairwise tree of the supersampled contract (first along a, then along b), the one
// render_body's SS epilogue applies to its 8 x 8 tile.
//
// P describes the SAMPLE grid (camera rt_camera_supersample, width = S x out_w): the primary ray of sample
// (S i + a, S j + b) is formed by exactly the operations of render_body.  The pixels of a wave are scattered over
// the frame, so there are no per-tile cone or level masks: the rays take the generic path of rt_trace_rays_kernel
// (trace<B, false, TRANSP, false> / trace_tree<B>), with hits_ok_from(eye) as the ray-list kernel computes it.
// Lanes past the end of the list repeat its last pixel and store nothing (trace() reduces over the whole wave).
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_refine_kernel(const DevScene* __restrict__ S, RenderParams P, int out_w,
                                                       const uint32_t* __restrict__ count,
                                                       const uint32_t* __restrict__ list, void* o32, void* o8,
                                                       double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t n = *count;                              // pixels on the list (written by rt_classify_kernel)
    const int s = P.ss_log2, s2 = 2 * s;
    const uint32_t per_wave = 64u >> s2;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const d3 eye = ld3(P.eye);
    V.hits_ok = hits_ok_from(S, eye);
    double* slot = reinterpret_cast<double*>(smem) + lane;
    int* mslot = reinterpret_cast<int*>(smem + 3 * 8 * colour_slots(B, TRANSP) * 64) + lane;
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    const int a = lane & ((1 << s) - 1), b = (lane >> s) & ((1 << s) - 1);
    for (uint64_t g = blockIdx.x; g * per_wave < n; g += gridDim.x) {
        const uint32_t q = (uint32_t)(g * per_wave) + (uint32_t)(lane >> s2);
        const uint32_t pix = list[q < n ? q : n - 1];       // j * out_w + i
        const int j0 = (int)(pix / (uint32_t)out_w), i0 = (int)(pix - (uint32_t)j0 * (uint32_t)out_w);
        const int ic = (i0 << s) + a, j = (j0 << s) + b;
        // Primary ray Line(camera, sp), as render_body forms it
        const d3 sp = add(add(ld3(P.look), scl(P.pitch * (double)(ic + P.bottom_x), right)),
                          scl(P.pitch * (double)(j + P.bottom_y), upp));
        uint32_t seg = 0, sh = 0;
        d3 col;
        if constexpr (TREE)
            col = trace_tree<B>(V, eye, sp, &seg, &sh);
        else
            col = trace<B, false, TRANSP, false, 64>(V, eye, sp, ~0ull, &seg, &sh, slot, mslot);
        for (int m = 1; m < (1 << s2); m <<= 1) {           // every lane active
            col.x += __shfl_xor(col.x, m);
            col.y += __shfl_xor(col.y, m);
            col.z += __shfl_xor(col.z, m);
            seg += __shfl_xor(seg, m);
            sh += __shfl_xor(sh, m);
        }
        col = scl(ldexp(1.0, -s2), col);                    // 1.0 / (S * S), exact
        if ((lane & ((1 << s2) - 1)) == 0 && q < n) {
            const size_t k = pix;
            store_pixel<false>(P, k, col, o32, o8);
            if (o64) { o64[3 * k] = col.x; o64[3 * k + 1] = col.y; o64[3 * k + 2] = col.z; }
            if (orc2) { orc2[2 * k] = seg; orc2[2 * k + 1] = sh; }
        }
    }
}

struct RefineLaunch {
    int variant;                               // 0 opaque, 1 FULL (meshes / transparent materials), 2 ray trees
    unsigned grid;
    hipStream_t stream;
    const DevScene* scene;
    RenderParams P;                            // the sample grid's (ss_log2 set)
    int out_w;
    const uint32_t* count;
    const uint32_t* list;
    void* o32;
    void* o8;
    double* o64;
    uint32_t* orc2;
};

// Defined once per depth B in rt_adaptive_b<B>.o (rt_adaptive.hip).
template <int B>
hipError_t launch_refine(const RefineLaunch& L);
#define RT_DECLARE_REFINE(B) \
    template <>              \
    hipError_t launch_refine<B>(const RefineLaunch& L);
RT_DECLARE_REFINE(0) RT_DECLARE_REFINE(1) RT_DECLARE_REFINE(2) RT_DECLARE_REFINE(3)
RT_DECLARE_REFINE(4) RT_DECLARE_REFINE(5) RT_DECLARE_REFINE(6) RT_DECLARE_REFINE(7)
#undef RT_DECLARE_REFINE

template <int B>
hipError_t launch_refine_impl(const RefineLaunch& L) {
    if constexpr (B > RT_MAX_B) {
        return hipErrorInvalidValue;
    } else {
        const dim3 g(L.grid), w(64);
        if (L.variant == 2)
            hipLaunchKernelGGL((rt_refine_kernel<B, true, true>), g, w, 0, L.stream, L.scene, L.P, L.out_w, L.count,
                               L.list, L.o32, L.o8, L.o64, L.orc2);
        else if (L.variant == 1)
            hipLaunchKernelGGL((rt_refine_kernel<B, true, false>), g, w, slot_bytes(B, true, 64), L.stream, L.scene,
                               L.P, L.out_w, L.count, L.list, L.o32, L.o8, L.o64, L.orc2);
        else
            hipLaunchKernelGGL((rt_refine_kernel<B, false, false>), g, w, slot_bytes(B, false, 64), L.stream, L.scene,
                               L.P, L.out_w, L.count, L.list, L.o32, L.o8, L.o64, L.orc2);
        return hipGetLastError();
    }
}

}  // namespace rtk
