// rt_sampled.hpp — the list-free sampled kernels: S x S rays per output pixel, one per lane, reduced in the wave.
//
//   rt_refine_kernel<B, TRANSP, TREE>  adaptive supersampling (rt_render_adaptive_dev, include/rt_api.h): the samples
//                                      of the pixels on a compacted work list.
//   rt_lens_kernel<B, TRANSP, TREE, AREA, MOTION>  thin-lens rays over the whole frame, in three kinds:
//                                      depth of field (rt_render_dof_dev), AREA: soft shadows (rt_render_soft_dev), each
//                                      ray lit by its own light points, and AREA, MOTION: motion blur
//                                      (rt_render_motion_dev), each sample at its own shutter time.
//   rt_lens_coarse_kernel<B, TRANSP, TREE>, rt_lens_refine_kernel<B, TRANSP, TREE>  the two tracing passes of the
//                                      adaptive lens render (rt_render_lens_adaptive_dev): the motion kind over the
//                                      whole frame with each pixel's sample spread, and over a compacted work list.
//   rt_jitter_kernel<B, TRANSP, TREE>  the jittered render (rt_render_jitter_dev): the motion kind with each sample at
//                                      a hashed sub-position of its stratum in every dimension.
//   rt_shutter_kernel<B, TRANSP, TREE> the shutter render (rt_render_shutter_dev): the jittered kind with the camera
//                                      of each sample's own time, its basis formed per lane.
//   rt_accum_kernel<B, TRANSP, TREE>   progressive accumulation (rt_render_accum_dev): the shutter kind's frames of
//                                      consecutive seeds, summed per pixel in a fixed order by the wave that owns it.
//   rt_converge_kernel<B, TRANSP, TREE> converging accumulation (rt_render_converge_dev): that sum with a sum of
//                                      squares and a pass count per pixel; a pixel stops once its standard error is low.
// All take RenderParams P of the SAMPLE grid (camera rt_camera_supersample, width = S x the output's, ss_log2 set) and
// share the sample-grid contract with render_body's supersampled instances through the helpers of rt_render.hpp:
// screen_point forms a sample's ray end, reduce_samples is the contract's fixed pairwise tree, store_sampled writes
// the reduced pixel.  None has a tile of neighbouring rays from one origin, so there are no cone or level masks:
// the rays take the generic path (trace_generic, as rt_trace_rays_kernel) with hits_ok_from of their start.  trace()
// reduces over the whole wave: every lane stays active, lanes without a sample trace a clamped one and store nothing.
//
// The instances are compiled once per bounce depth, in parallel with the render kernels' translation units:
// rt_adaptive.hip (rt_adaptive_b<B>.o), once per depth and kind rt_lens.hip (rt_lens_k<kind>_b<B>.o), and
// rt_lens_adaptive.hip (rt_lens_adaptive_b<B>.o), rt_jitter.hip (rt_jitter_b<B>.o), rt_shutter.hip
// (rt_shutter_b<B>.o), rt_accum.hip (rt_accum_b<B>.o) and rt_converge.hip (rt_converge_b<B>.o).
#pragma once

#include "rt_jitter.hpp"
#include "rt_render.hpp"

namespace rtk {

// One-wave workgroups; a fixed grid (the pixel count is only known on the device: rt_classify_kernel, rt_sampled.hip,
// writes the list and its length) walks the list with a grid-stride loop.  A wave takes 64 / S^2 listed pixels per
// step: lane l traces sample (a, b) of the pixel of its group l >> 2 log2 S, a = the low log2 S bits of l, b the next
// log2 S: reduce_samples with lane stride S.  Lanes past the end of the list repeat its last pixel.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_refine_kernel(const DevScene* __restrict__ S, RenderParams P, int out_w,
                                                       const uint32_t* __restrict__ count,
                                                       const uint32_t* __restrict__ list, void* o32, void* o8,
                                                       double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t n = *count;                              // pixels on the list
    const int s = P.ss_log2, s2 = 2 * s;
    const uint32_t per_wave = 64u >> s2;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const d3 eye = ld3(P.eye);
    V.hits_ok = hits_ok_from(S, eye);
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    const int a = lane & ((1 << s) - 1), b = (lane >> s) & ((1 << s) - 1);
    for (uint64_t g = blockIdx.x; g * per_wave < n; g += gridDim.x) {
        const uint32_t q = (uint32_t)(g * per_wave) + (uint32_t)(lane >> s2);
        const uint32_t pix = list[q < n ? q : n - 1];       // j * out_w + i
        const int j0 = (int)(pix / (uint32_t)out_w), i0 = (int)(pix - (uint32_t)j0 * (uint32_t)out_w);
        const d3 sp = screen_point(P, (i0 << s) + a, (j0 << s) + b, right, upp);
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64>(V, eye, sp, smem, &seg, &sh);
        reduce_samples(s, 1 << s, col, seg, sh);
        if ((lane & ((1 << s2) - 1)) == 0 && q < n) store_sampled(P, pix, col, seg, sh, o32, o8, o64, orc2);
    }
}

constexpr int kDofGridY = 32768;               // tile rows per grid.z slice (grid.y and grid.z stay below 65536)

// One-wave workgroups; a wave owns one 8 x 8 block of the sample grid — an (8 / S) x (8 / S) tile of output pixels —
// with lane bits 0..2 = x and bits 3..5 = y, as render_body's supersampled instances: lane (x, y) holds sample
// (a, b) = (x mod S, y mod S) of output pixel (8 tx / S + x / S, 8 ty / S + y / S): reduce_samples with lane stride 8,
// and the lanes of a wave trace neighbouring pixels (the coherence the scattered refine kernel lacks).
//
// The ray's end is its sample's screen point; its start is the lens point
//     e(a, b) = (eye + (A t_a) right) + (A t_b) up',   t_a = (2 a + 1 - S) / S,
// one IEEE operation per parenthesis and component, in this order; hits_ok_from(e) per lane.  A = 0 and S = 1 run this
// same code.  The sample frame is S times the output, and S divides 8, so an S x S block lies wholly inside the sample
// frame or wholly outside it; lanes outside (and the padding tile rows of the last grid.z slice) store nothing.
//
// AREA (soft shadows): sample (a, b) also sees every light of the scene displaced to
//     (L.x + (R t_a), L.y, L.z + (R t_b)),
// point (a, b) of a square panel of half-width R = light_size in the world xz-plane, paired with the lens point and the
// sub-pixel point of the same (a, b).  The shift reaches shade() through trace_generic<.., AREA = true> (rt_device.hpp:
// no light-cone records and no masks for the displaced shadow rays).  R = 0, A = 0 and S = 1 run this same code.
//
// MOTION (motion blur, on AREA): sample (a, b) of a pixel also has the time
//     sigma = F u_n,   n = a + S b,   u_n = (2 n + 1 - S^2) / S^2
// (an exact quotient: S^2 is a power of two), F = shutter, at which sphere k is centred at (cl_k + sigma d_k) + pos
// (rt_device.hpp Motion: the displacement d_k and the swept-sphere filter records come from the context's motion
// record M, rt_set_motion).  hits_ok is hits_ok_from with the motion record's flag and limit, which the host proves
// for the swept extents.  F = 0, d = 0, R = 0, A = 0 and S = 1 run this same code.
//
// One __global__ template for the three kinds, with one parameter list (light_size, shutter and M are passed to all
// and read under their flag only: M may be nullptr without MOTION).  The parts of a kind sit under if constexpr, so an
// instance compiles to the code its own kernel had (profiles/lens/isa_compare.md); a shared __device__ body called
// from three kernels did not: the lens kernel's instances came out with another register allocation.
template <int B, bool TRANSP, bool TREE, bool AREA, bool MOTION>
__global__ __launch_bounds__(64) void rt_lens_kernel(const DevScene* __restrict__ S, const DevMotion* __restrict__ M,
                                                     RenderParams P, double aperture, double light_size,
                                                     double shutter, int tile_rows, void* o32, void* o8, double* o64,
                                                     uint32_t* orc2) {
    static_assert(AREA || !MOTION, "the motion instances are area-light instances");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int s = P.ss_log2, S1 = (1 << s) - 1;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int x = lane & 7, y = lane >> 3;
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    const int i = tx * 8 + x, lr = ty * 8 + y;
    const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    const d3 sp = screen_point(P, ic, j, right, upp);
    // Ray start: t = (2 a + 1 - S) / S, an exact quotient (S is a power of two: the product with 2^-s is the same bits)
    const double inv_s = ldexp(1.0, -s);
    const double ta = (double)(2 * (x & S1) - S1) * inv_s, tb = (double)(2 * (y & S1) - S1) * inv_s;
    const d3 e = add(add(ld3(P.eye), scl(aperture * ta, right)), scl(aperture * tb, upp));
    uint32_t seg = 0, sh = 0;
    d3 col;
    if constexpr (MOTION) {
        const int n = (x & S1) + ((y & S1) << s);           // time index a + S b; u_n exact as t is
        const double sigma = shutter * ((double)(2 * n + 1 - (1 << 2 * s)) * ldexp(1.0, -2 * s));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                             LightShift{light_size * ta, light_size * tb}, &mo);
    } else if constexpr (AREA) {
        V.hits_ok = hits_ok_from(S, e);
        col = trace_generic<B, TRANSP, TREE, 64, true>(V, e, sp, smem, &seg, &sh,
                                                       LightShift{light_size * ta, light_size * tb});
    } else {
        V.hits_ok = hits_ok_from(S, e);
        col = trace_generic<B, TRANSP, TREE, 64>(V, e, sp, smem, &seg, &sh);
    }
    reduce_samples(s, 8, col, seg, sh);
    if ((x & S1) == 0 && (y & S1) == 0 && i < P.width && lr < P.height && !pad) {
        const size_t k = (size_t)(lr >> s) * (size_t)(P.width >> s) + (size_t)(i >> s);
        store_sampled(P, k, col, seg, sh, o32, o8, o64, orc2);
    }
}

// ---- The adaptive lens render (rt_render_lens_adaptive_dev, include/rt_api.h): both tracing passes run the motion
// kind (AREA, MOTION) — an unset motion is the zero record the context keeps, R = 0 and A = 0 run the same code — so a
// depth has one instance of each per scene variant. ----

// The lanes' packed colour bytes (r | g << 8 | b << 16), channel by channel the larger one.
__device__ __forceinline__ uint32_t max_bytes3(uint32_t p, uint32_t q) {
    return max(p & 0xffu, q & 0xffu) | max(p & 0xff00u, q & 0xff00u) | max(p & 0xff0000u, q & 0xff0000u);
}

// The coarse pass: rt_lens_kernel<B, TRANSP, TREE, true, true> statement for statement — the same frame, bit for bit —
// plus the pixel's sample spread: before the reduction every lane packs the three RGBA8 bytes of its own sample
// (to_u8: NaN -> 0), an integer max butterfly with reduce_samples' partners at lane stride 8 runs over the bytes and
// over their complements (255 - byte: the minimum), and the block's first lane stores
//     max over channels of (max - min over the S x S samples)
// as one byte at spread[k].  An S x S block lies wholly inside or outside the sample frame (rt_lens_kernel), so a
// clamped lane never enters an in-frame pixel's spread.  S = 1: no partner, spread 0.  A kernel of its own, not a flag
// of rt_lens_kernel: that one's parameter list, hence its instances' code, stays what it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_lens_coarse_kernel(const DevScene* __restrict__ S,
                                                            const DevMotion* __restrict__ M, RenderParams P,
                                                            double aperture, double light_size, double shutter,
                                                            int tile_rows, void* o32, void* o8, double* o64,
                                                            uint32_t* orc2, uint8_t* __restrict__ spread) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int s = P.ss_log2, S1 = (1 << s) - 1;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int x = lane & 7, y = lane >> 3;
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    const int i = tx * 8 + x, lr = ty * 8 + y;
    const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    const d3 sp = screen_point(P, ic, j, right, upp);
    const double inv_s = ldexp(1.0, -s);
    const double ta = (double)(2 * (x & S1) - S1) * inv_s, tb = (double)(2 * (y & S1) - S1) * inv_s;
    const d3 e = add(add(ld3(P.eye), scl(aperture * ta, right)), scl(aperture * tb, upp));
    uint32_t seg = 0, sh = 0;
    const int n = (x & S1) + ((y & S1) << s);
    const double sigma = shutter * ((double)(2 * n + 1 - (1 << 2 * s)) * ldexp(1.0, -2 * s));
    const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];
    V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
    const Motion mo{sigma, M};
    d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                            LightShift{light_size * ta, light_size * tb}, &mo);
    const uint32_t mine = (uint32_t)to_u8(col.x) | ((uint32_t)to_u8(col.y) << 8) | ((uint32_t)to_u8(col.z) << 16);
    uint32_t hi = mine, lo = 0xffffffu - mine;              // lo: the complements, so one max serves both
    for (int m = 1; m <= 8 * S1; m = 2 * m == 1 << s ? 8 : 2 * m) {
        hi = max_bytes3(hi, (uint32_t)__shfl_xor((int)hi, m));
        lo = max_bytes3(lo, (uint32_t)__shfl_xor((int)lo, m));
    }
    reduce_samples(s, 8, col, seg, sh);
    if ((x & S1) == 0 && (y & S1) == 0 && i < P.width && lr < P.height && !pad) {
        const size_t k = (size_t)(lr >> s) * (size_t)(P.width >> s) + (size_t)(i >> s);
        store_sampled(P, k, col, seg, sh, o32, o8, o64, orc2);
        const uint32_t d = hi + lo - 0xffffffu;             // per byte max - min >= 0: no borrow between the bytes
        spread[k] = (uint8_t)max(max(d & 0xffu, (d >> 8) & 0xffu), (d >> 16) & 0xffu);
    }
}

// The refine pass: rt_refine_kernel's walk of the work list with the lens family's rays.  P is the S x S sample grid
// of the refined pixels; lane l traces sample (a, b) of the pixel of its group l >> 2 log2 S exactly as lane
// (x, y) = (a, b) mod S of rt_lens_kernel<.., true, true> does — lens point e(a, b), light shift (R t_a, R t_b), time
// sigma of n = a + S b, hits_ok from the motion record's swept proof per lane — and reduce_samples at lane stride S is
// the same tree, so a listed pixel gets the value and the counters rt_render_motion_dev gives it.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_lens_refine_kernel(const DevScene* __restrict__ S,
                                                            const DevMotion* __restrict__ M, RenderParams P,
                                                            double aperture, double light_size, double shutter,
                                                            int out_w, const uint32_t* __restrict__ count,
                                                            const uint32_t* __restrict__ list, void* o32, void* o8,
                                                            double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const uint32_t n = *count;                              // pixels on the list
    const int s = P.ss_log2, s2 = 2 * s, S1 = (1 << s) - 1;
    const uint32_t per_wave = 64u >> s2;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    const int a = lane & S1, b = (lane >> s) & S1;
    const double inv_s = ldexp(1.0, -s);
    const double ta = (double)(2 * a - S1) * inv_s, tb = (double)(2 * b - S1) * inv_s;
    const d3 e = add(add(ld3(P.eye), scl(aperture * ta, right)), scl(aperture * tb, upp));
    const double sigma = shutter * ((double)(2 * (a + (b << s)) + 1 - (1 << s2)) * ldexp(1.0, -s2));
    const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];
    V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
    const Motion mo{sigma, M};
    const LightShift ls{light_size * ta, light_size * tb};
    for (uint64_t g = blockIdx.x; g * per_wave < n; g += gridDim.x) {
        const uint32_t q = (uint32_t)(g * per_wave) + (uint32_t)(lane >> s2);
        const uint32_t pix = list[q < n ? q : n - 1];       // j * out_w + i
        const int j0 = (int)(pix / (uint32_t)out_w), i0 = (int)(pix - (uint32_t)j0 * (uint32_t)out_w);
        const d3 sp = screen_point(P, (i0 << s) + a, (j0 << s) + b, right, upp);
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh, ls, &mo);
        reduce_samples(s, 1 << s, col, seg, sh);
        if ((lane & ((1 << s2) - 1)) == 0 && q < n) store_sampled(P, pix, col, seg, sh, o32, o8, o64, orc2);
    }
}

// ---- The jittered render (rt_render_jitter_dev, include/rt_api.h): the motion kind with every sample moved, in each
// of its seven dimensions, to one of J sub-positions of its stratum. ----

// What the jittered kernel gets beside the motion kind's arguments: the fine camera's pitch and frame corner
// (pitch / (S J), S J bottom: formed and range-checked by the host), jl = log2 J and the seed.
struct JitterParams {
    double pitch_f;
    int32_t bottom_fx, bottom_fy;
    int32_t jl;
    uint32_t seed;
};

// rt_lens_kernel<B, TRANSP, TREE, true, true>'s wave layout, clamping, hits_ok, trace and reduction, with the lane's
// sample (I, Jr) = (i, lr) of the sample frame drawing seven levels k_0 .. k_6 in 0 .. J - 1 from one hash word
// (rt_jitter.hpp; the key is Jr (S width) + I with the sample frame's own width P.width and the lane's unclamped
// coordinates: a lane outside the frame stores nothing, so its key does not matter).  Every quotient is that of the
// regular grid J times finer, still exact (a power of two):
//     ray end     the fine camera's screen point of fine pixel (J I + k_0, J Jr + k_1),
//     ray start   t_x = (2 (J a + k_2) + 1 - S J) / (S J), t_y from (b, k_3),
//     lights      g_x from (a, k_4), g_z from (b, k_5), the same formula,
//     time        u = (2 (J n + k_6) + 1 - S S J) / (S S J), n = a + S b.
// |t|, |g|, |u| < 1 as on the regular grid, so the motion record's swept proofs hold as they stand.  J = 1: every level
// is 0 and each expression above is the motion kind's, bit for bit.  A kernel of its own, not a flag of rt_lens_kernel:
// that one's parameter list, hence its instances' code, stays what it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_jitter_kernel(const DevScene* __restrict__ S, const DevMotion* __restrict__ M,
                                                       RenderParams P, JitterParams Q, double aperture,
                                                       double light_size, double shutter, int tile_rows, void* o32,
                                                       void* o8, double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int x = lane & 7, y = lane >> 3;
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    const int i = tx * 8 + x, lr = ty * 8 + y;
    const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
    const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed);
    const d3 right = ld3(P.right), upp = ld3(P.upp);
    // screen_point of the fine camera (look, right and up' are P's: the cameras differ in pitch and corner only)
    const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
    const d3 sp = add(add(ld3(P.look), scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                      scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
    const int a = x & S1, b = y & S1, sj = s + jl;
    const double inv_sj = ldexp(1.0, -sj);
    const auto t_of = [&](int c, int k) { return (double)(2 * ((c << jl) + k) + 1 - (1 << sj)) * inv_sj; };
    const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
    const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
    const d3 e = add(add(ld3(P.eye), scl(aperture * ta, right)), scl(aperture * tb, upp));
    const int n = a + (b << s);                             // time index a + S b
    const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                    ldexp(1.0, -(s + sj)));
    const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
    V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
    const Motion mo{sigma, M};
    uint32_t seg = 0, sh = 0;
    d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                            LightShift{light_size * ga, light_size * gb}, &mo);
    reduce_samples(s, 8, col, seg, sh);
    if (a == 0 && b == 0 && i < P.width && lr < P.height && !pad) {
        const size_t k = (size_t)(lr >> s) * (size_t)(P.width >> s) + (size_t)(i >> s);
        store_sampled(P, k, col, seg, sh, o32, o8, o64, orc2);
    }
}

// ---- The shutter render (rt_render_shutter_dev, include/rt_api.h): the jittered render with the camera itself moving
// during the exposure, so that every sample has the camera of its own time. ----

// What the shutter kernel gets beside the jittered kernel's arguments: the camera's up and the half-extents of the
// eye's and the look-at point's move (rt_camera_motion: six doubles; all zero without a motion).
struct ShutterParams {
    double up[3];
    double eye_move[3];
    double look_move[3];
};

// rt_jitter_kernel statement for statement — wave layout, clamping, the key from the true sample-frame width, the
// levels, the swept hits_ok, trace, reduction and store — but for the camera: P's eye and look are those of sigma = 0,
// P's right and up' are not read, and the lane forms
//     eye_s = eye + (sigma * eye_move),   look_s = look + (sigma * look_move)       (one operation per parenthesis),
//     LD = look_s - eye_s,   right_s = normalize(LD x up),   up'_s = normalize(right_s x LD)
// with rt_host.cpp's operation order (rt_camera_basis; cross and cam_normalize of rt_device.hpp: IEEE sqrt and
// division), so sigma moves up ahead of the ray's end.  Under jitter a frame has up to S S J distinct times, so the
// basis cannot be a table of the host's.  A zero move gives eye_s = eye and look_s = look (no component is -0.0) and
// the basis rt_camera_basis gave P, bit for bit: the jittered render's frame.  eye_s, look_s and the basis are dead
// once e and sp are formed — nothing of them is live across the trace.  hits_ok is the motion record's swept proof
// from the lane's own start e, which now differs between the lanes of a wave by the eye's move too.  A kernel of its
// own, not a flag of rt_jitter_kernel: that one's parameter list, hence its instances' code, stays what it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_shutter_kernel(const DevScene* __restrict__ S, const DevMotion* __restrict__ M,
                                                        RenderParams P, JitterParams Q, ShutterParams C,
                                                        double aperture, double light_size, double shutter,
                                                        int tile_rows, void* o32, void* o8, double* o64,
                                                        uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x;
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int x = lane & 7, y = lane >> 3;
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    const int i = tx * 8 + x, lr = ty * 8 + y;
    const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
    const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed);
    const int a = x & S1, b = y & S1, sj = s + jl;
    const int n = a + (b << s);                             // time index a + S b
    const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                    ldexp(1.0, -(s + sj)));
    // the camera of the lane's time
    const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
    const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
    const d3 ld = sub(look, eye);
    const d3 right = cam_normalize(cross(ld, ld3(C.up)));
    const d3 upp = cam_normalize(cross(right, ld));
    // screen_point of the fine camera at that time
    const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
    const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                      scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
    const double inv_sj = ldexp(1.0, -sj);
    const auto t_of = [&](int c, int k) { return (double)(2 * ((c << jl) + k) + 1 - (1 << sj)) * inv_sj; };
    const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
    const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
    const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
    const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
    V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
    const Motion mo{sigma, M};
    uint32_t seg = 0, sh = 0;
    d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                            LightShift{light_size * ga, light_size * gb}, &mo);
    reduce_samples(s, 8, col, seg, sh);
    if (a == 0 && b == 0 && i < P.width && lr < P.height && !pad) {
        const size_t k = (size_t)(lr >> s) * (size_t)(P.width >> s) + (size_t)(i >> s);
        store_sampled(P, k, col, seg, sh, o32, o8, o64, orc2);
    }
}

// ---- Progressive accumulation (rt_render_accum_dev, include/rt_api.h): the frames of consecutive seeds of the shutter
// render summed per pixel in the kernel, in the contract's fixed order. ----

// What the accumulating kernel gets beside the shutter kernel's arguments: the passes of this launch, first ..
// first + count - 1 (first + count <= 2^31), and the first pass of the call the launch belongs to (the host splits a
// call into launches of at most rt_ctx::Knobs::accum_max_passes passes).
struct AccumParams {
    uint32_t first;
    uint32_t count;
    uint32_t call_first;
};

// rt_shutter_kernel's wave layout, clamping and key; then a loop over the launch's passes whose body is that kernel's
// statements from the hash word on, with the seed Q.seed + p (uint32, wrapping) of pass p: word, levels, time, the
// lane's camera and basis, ray, light shift, swept hits_ok, trace and reduce_samples.  After the reduction every lane of
// a pixel's block holds the pass's value v_p and counters; the block's first lane, (a, b) = (0, 0), adds them to the
// pixel's running sum:
//     acc = accum[k] if first > 0, and acc = acc + v_p pass by pass: one IEEE addition per channel, left to right from
//           the LOADED value — never a local partial sum added to it afterwards, which rounds differently;
//     acc = v_0 for pass 0: accum is not read when first = 0 (it may be uninitialised).
// Both branches are on kernel arguments: wave-uniform.  accum is read at most once, before the loop, and written once,
// after it; so are the counters: orc2 holds the sum over the passes of the CALL, so a launch that is not the call's
// first (first > call_first) starts from the words the launch before it left.  The images derive from the mean
// m = acc / (double)(first + count), one IEEE division per channel (not a product with a reciprocal: other bits), by
// store_sampled; the host passes the image pointers to a call's last launch only, and the division runs under them.
// The running sum and the two counters are parked in LDS across the trace, not held in registers: with them (and the
// lane's coordinates) live across the trace the opaque instance needed 107 VGPRs and the transparent one 142, a wave per
// SIMD fewer than the shutter kernel's 84 and 119; parked they need 93 and 126 at depth 1 and keep its 5 and 4 waves.
// A kernel of its own, not a flag of rt_shutter_kernel: that one's parameter list, hence its instances' code, stays what
// it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_accum_kernel(const DevScene* __restrict__ S, const DevMotion* __restrict__ M,
                                                      RenderParams P, JitterParams Q, ShutterParams C, AccumParams N,
                                                      double aperture, double light_size, double shutter,
                                                      int tile_rows, double* accum, void* o32, void* o8, double* o64,
                                                      uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    // The lane's coordinates are formed from its number again wherever they are read — before the loop, in every pass
    // and after the loop — behind an empty asm that hides the number's origin from the optimiser: otherwise the dozen
    // values derived from it stay in registers across the trace beside the running sum, which cost the opaque and the
    // transparent instances a wave per SIMD each (107 and 142 VGPRs against the shutter kernel's 84 and 119).
    struct Lane { int i, lr, a, b, q; bool owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = tx * 8 + x;
        r.lr = ty * 8 + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.owner = r.a == 0 && r.b == 0 && r.i < P.width && r.lr < P.height && !pad;
        r.k = (size_t)(r.lr >> s) * (size_t)(P.width >> s) + (size_t)(r.i >> s);      // read under `owner` only
        return r;
    };
    // The running sums wait in LDS behind trace()'s slots, one slot per output pixel of the tile (accum_park_bytes):
    // three doubles and the two counters, touched by the pixel's first lane alone.
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_rgb + 3 * npix);
    {
        const Lane ln = lane_of();
        if (ln.owner) {
            d3 acc = mk(0.0, 0.0, 0.0);
            uint32_t seg_sum = 0, sh_sum = 0;
            if (N.first > 0) acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
            if (N.first > N.call_first && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            park_rgb[ln.q] = acc.x; park_rgb[npix + ln.q] = acc.y; park_rgb[2 * npix + ln.q] = acc.z;
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
        }
    }
    for (uint32_t t = 0; t < N.count; ++t) {
        const uint32_t p = N.first + t;
        const Lane ln = lane_of();
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + p);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        if (after.owner) {
            const int q = after.q;
            const d3 acc = p == 0 ? col : add(mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]), col);
            park_rgb[q] = acc.x; park_rgb[npix + q] = acc.y; park_rgb[2 * npix + q] = acc.z;
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
        }
    }
    const Lane ln = lane_of();
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]);
        const uint32_t seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
        if (o32 || o8 || o64 || orc2) {
            const double cnt = (double)(N.first + N.count);
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
        }
    }
}

// ---- Converging accumulation (rt_render_converge_dev, include/rt_api.h): rt_accum_kernel's sum with a sum of squares
// and a pass count per pixel, and a pixel that stops receiving passes once its standard error is low. ----

// What the converging kernel gets beside the shutter kernel's arguments: the most passes a pixel receives in this
// launch, the rule's M and E, whether the launch is not the first of its call (then the counters continue from the
// words the launch before it left) and whether it is the last (then it writes the images and counts `active`).
struct ConvergeParams {
    double tolerance;
    uint32_t count;
    uint32_t min_passes;
    uint32_t later;
    uint32_t last;
};

// Rule 3 of the contract: one IEEE operation per operator, in this order (-ffp-contract=off: nothing fuses).  n = 0 is
// never stopped (M >= 2); a NaN d compares false and does not hold the pixel back.
__device__ __forceinline__ bool converge_stopped(d3 acc, d3 sq, uint32_t n, uint32_t min_passes, double tol) {
    if (n == 0x80000000u) return true;
    if (n < min_passes) return false;
    const double dn = (double)n;
    const double lim = (tol * tol) * (dn * (double)(n - 1u));
    const double dx = sq.x - (acc.x * acc.x) / dn, dy = sq.y - (acc.y * acc.y) / dn, dz = sq.z - (acc.z * acc.z) / dn;
    return !(dx > lim) && !(dy > lim) && !(dz > lim);
}

// rt_accum_kernel's wave layout, clamping, key, lane_of and pass body, with every pixel on a pass number of its own: the
// state (acc, sq, n) of a pixel waits in LDS behind trace()'s slots (converge_park_bytes: 60 bytes per output pixel of
// the tile), written by the pixel's first lane alone and, n, read by all S S lanes of the pixel, whose seed is
// Q.seed + n (uint32, wrapping): a per-lane value.  Before every pass the first lane of each pixel evaluates rule 3 on the
// parked state and one __ballot over these lanes gives `live`, the wave's pixels that receive this pass, in a scalar
// pair: live = 0 ends the loop (wave-uniform), so a wave whose pixels had all stopped before the launch traces nothing.
// In a live wave the lanes of a stopped pixel trace the pixel's would-be next pass (a valid ray: seed Q.seed + n) and
// discard it, as pad lanes do; that is sound because a lane's value does not depend on the other lanes' rays —
// trace() reduces over the wave for its loop conditions only, which the refine kernels (rt_refine_kernel,
// rt_lens_refine_kernel) already rely on — and reduce_samples never crosses a pixel's S x S block.  After the reduction
// the first lane of a pixel in `live` does rule 2: acc = v, sq = v * v for n = 0, else acc = acc + v, sq = sq + (v * v),
// one multiplication then one addition (not fused), from the PARKED values; n = n + 1; the pass's counters are added.
// Stores: `accum`, `accum2` and `count` once after the loop, by a wave that ran a pass (the others hold what is
// there); the counters in every launch; the images from m = acc / (double)n in the call's last launch, which also adds
// the wave's pixels that are not stopped to *active: a ballot popcount and one vector atomic per wave.
// LDS: 60 instead of rt_accum_kernel's 32 bytes per pixel is 3840 B per wave at S = 1 (960, 240, 60 B at S = 2, 4, 8);
// profiles/converge/README.md has what that costs in workgroups per CU and why sq is not kept in `accum2`.
// A kernel of its own, not a flag of rt_accum_kernel: that one's parameter list, hence its instances' code, stays what
// it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_converge_kernel(const DevScene* __restrict__ S, const DevMotion* __restrict__ M,
                                                         RenderParams P, JitterParams Q, ShutterParams C,
                                                         ConvergeParams N, double aperture, double light_size,
                                                         double shutter, int tile_rows, double* accum, double* accum2,
                                                         uint32_t* count, uint32_t* active, void* o32, void* o8,
                                                         double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    // (rt_accum_kernel: the lane's coordinates are formed again wherever they are read)
    struct Lane { int i, lr, a, b, q; bool first, owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = tx * 8 + x;
        r.lr = ty * 8 + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.first = r.a == 0 && r.b == 0;
        r.owner = r.first && r.i < P.width && r.lr < P.height && !pad;
        r.k = (size_t)(r.lr >> s) * (size_t)(P.width >> s) + (size_t)(r.i >> s);      // read under `owner` only
        return r;
    };
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    double* park_sq = park_rgb + 3 * npix;
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_sq + 3 * npix);
    uint32_t* park_n = park_rc + 2 * npix;
    const auto parked = [&](const double* p, int q) { return mk(p[q], p[npix + q], p[2 * npix + q]); };
    const auto park = [&](double* p, int q, d3 v) { p[q] = v.x; p[npix + q] = v.y; p[2 * npix + q] = v.z; };
    {
        // every pixel slot of the tile is filled: a slot outside the frame holds n = 0 and is never live
        const Lane ln = lane_of();
        if (ln.first) {
            d3 acc = mk(0.0, 0.0, 0.0), sq = mk(0.0, 0.0, 0.0);
            uint32_t n = 0, seg_sum = 0, sh_sum = 0;
            if (ln.owner) {
                n = count[ln.k];
                if (n > 0) {                                // n = 0: accum and accum2 are not read
                    acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
                    sq = mk(accum2[3 * ln.k], accum2[3 * ln.k + 1], accum2[3 * ln.k + 2]);
                }
                if (N.later && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            }
            park(park_rgb, ln.q, acc);
            park(park_sq, ln.q, sq);
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
            park_n[ln.q] = n;
        }
    }
    bool ran = false;
    for (uint32_t t = 0; t < N.count; ++t) {
        // what the wave's first lanes parked, before the loop or in the pass before, is read by every lane below
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const Lane ln = lane_of();
        const uint32_t n_px = park_n[ln.q];
        const bool go = ln.owner && !converge_stopped(parked(park_rgb, ln.q), parked(park_sq, ln.q), n_px, N.min_passes,
                                                      N.tolerance);
        const uint64_t live = __ballot(go);
        if (live == 0) break;
        ran = true;
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + n_px);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        if (after.owner && ((live >> l) & 1ull)) {          // nothing of a stopped pixel's ray reaches the state
            const int q = after.q;
            const uint32_t np = park_n[q];
            const d3 v2 = mk(col.x * col.x, col.y * col.y, col.z * col.z);
            const d3 acc = np == 0 ? col : add(parked(park_rgb, q), col);
            const d3 sq = np == 0 ? v2 : add(parked(park_sq, q), v2);
            park(park_rgb, q, acc);
            park(park_sq, q, sq);
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
            park_n[q] = np + 1u;
        }
    }
    const Lane ln = lane_of();
    bool open = false;                                      // the pixel is not stopped on its final state
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = parked(park_rgb, q), sq = parked(park_sq, q);
        const uint32_t n = park_n[q], seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        if (ran) {
            accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
            accum2[3 * k] = sq.x; accum2[3 * k + 1] = sq.y; accum2[3 * k + 2] = sq.z;
            count[k] = n;
        }
        if (N.last) {
            const double cnt = (double)n;
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
            open = !converge_stopped(acc, sq, n, N.min_passes, N.tolerance);
        } else if (orc2) {
            orc2[2 * k] = seg_sum; orc2[2 * k + 1] = sh_sum;
        }
    }
    if (N.last && active) {
        const uint64_t still = __ballot(open);
        if (still != 0 && threadIdx.x == 0) atomicAdd(active, (uint32_t)__popcll(still));
    }
}

// ---- Windows of the accumulating and converging renders (rt_render_accum_window_dev, rt_render_converge_window_dev,
// include/rt_api.h): the pixels of one rectangle of the frame, byte for byte what the un-windowed kernels give them. ----

// What a windowed kernel gets beside its parent's arguments, folded by the host: the window's corners in SAMPLE units
// of the frame (S x0, S y0 and S (x0 + width), S (y0 + height): multiples of S) and the buffers' row stride in output
// pixels.  The buffer pointers arrive moved back by y0 * stride + x0 elements, so that a pixel's element number is
// formed from its FRAME coordinates, (lr >> s) * stride + (i >> s), without a subtraction.
struct WindowParams {
    int32_t sx0, sy0;
    int32_t sx1, sy1;
    int32_t stride;
};

// rt_accum_kernel statement for statement, but for lane_of and what hangs on it: the waves tile the window from its own
// origin (the grid is lens_grid over the window's sample extent), the lane's sample (i, lr) is the window's sample
// origin plus the tile's, `owner` and the padding test use the window's far corner, the element number uses the stride.
// S divides sx0, sy0 and 8, so (a, b) = (x, y) mod S is still the lane's sample within its pixel and an S x S block
// lies wholly inside the window or wholly outside it.  The pass body reads the FRAME's P: the key is
// lr * P.width + i of the full sample frame, and a lane past the window traces the frame's own sample there, or the
// frame's clamped one, and stores nothing — a valid ray either way, which is all the body needs of it (a lane's value
// does not depend on the other lanes' rays: rt_converge_kernel).  A kernel of its own, not a flag of rt_accum_kernel:
// that one's parameter list, hence its instances' code, stays what it was.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_accum_window_kernel(const DevScene* __restrict__ S,
                                                             const DevMotion* __restrict__ M, RenderParams P,
                                                             JitterParams Q, ShutterParams C, AccumParams N,
                                                             WindowParams W, double aperture, double light_size,
                                                             double shutter, int tile_rows, double* accum, void* o32,
                                                             void* o8, double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    // (rt_accum_kernel: the lane's coordinates are formed again wherever they are read)
    struct Lane { int i, lr, a, b, q; bool owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = W.sx0 + tx * 8 + x;
        r.lr = W.sy0 + ty * 8 + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.owner = r.a == 0 && r.b == 0 && r.i < W.sx1 && r.lr < W.sy1 && !pad;
        r.k = (size_t)(r.lr >> s) * (size_t)W.stride + (size_t)(r.i >> s);          // read under `owner` only
        return r;
    };
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_rgb + 3 * npix);
    {
        const Lane ln = lane_of();
        if (ln.owner) {
            d3 acc = mk(0.0, 0.0, 0.0);
            uint32_t seg_sum = 0, sh_sum = 0;
            if (N.first > 0) acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
            if (N.first > N.call_first && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            park_rgb[ln.q] = acc.x; park_rgb[npix + ln.q] = acc.y; park_rgb[2 * npix + ln.q] = acc.z;
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
        }
    }
    for (uint32_t t = 0; t < N.count; ++t) {
        const uint32_t p = N.first + t;
        const Lane ln = lane_of();
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + p);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        if (after.owner) {
            const int q = after.q;
            const d3 acc = p == 0 ? col : add(mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]), col);
            park_rgb[q] = acc.x; park_rgb[npix + q] = acc.y; park_rgb[2 * npix + q] = acc.z;
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
        }
    }
    const Lane ln = lane_of();
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]);
        const uint32_t seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
        if (o32 || o8 || o64 || orc2) {
            const double cnt = (double)(N.first + N.count);
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
        }
    }
}

// rt_converge_kernel statement for statement with rt_accum_window_kernel's lane_of: `first` is the lane's place in
// its pixel, `owner` a first lane inside the window.  A pixel slot of the tile outside the window holds n = 0 and is
// never live, so *active counts the window's pixels alone.  A kernel of its own, as above.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_converge_window_kernel(const DevScene* __restrict__ S,
                                                                const DevMotion* __restrict__ M, RenderParams P,
                                                                JitterParams Q, ShutterParams C, ConvergeParams N,
                                                                WindowParams W, double aperture, double light_size,
                                                                double shutter, int tile_rows, double* accum,
                                                                double* accum2, uint32_t* count, uint32_t* active,
                                                                void* o32, void* o8, double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const int tx = blockIdx.x, ty_raw = (int)(blockIdx.z * kDofGridY + blockIdx.y);
    const bool pad = ty_raw >= tile_rows;
    const int ty = pad ? tile_rows - 1 : ty_raw;
    // (rt_accum_kernel: the lane's coordinates are formed again wherever they are read)
    struct Lane { int i, lr, a, b, q; bool first, owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = W.sx0 + tx * 8 + x;
        r.lr = W.sy0 + ty * 8 + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.first = r.a == 0 && r.b == 0;
        r.owner = r.first && r.i < W.sx1 && r.lr < W.sy1 && !pad;
        r.k = (size_t)(r.lr >> s) * (size_t)W.stride + (size_t)(r.i >> s);          // read under `owner` only
        return r;
    };
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    double* park_sq = park_rgb + 3 * npix;
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_sq + 3 * npix);
    uint32_t* park_n = park_rc + 2 * npix;
    const auto parked = [&](const double* p, int q) { return mk(p[q], p[npix + q], p[2 * npix + q]); };
    const auto park = [&](double* p, int q, d3 v) { p[q] = v.x; p[npix + q] = v.y; p[2 * npix + q] = v.z; };
    {
        // every pixel slot of the tile is filled: a slot outside the window holds n = 0 and is never live
        const Lane ln = lane_of();
        if (ln.first) {
            d3 acc = mk(0.0, 0.0, 0.0), sq = mk(0.0, 0.0, 0.0);
            uint32_t n = 0, seg_sum = 0, sh_sum = 0;
            if (ln.owner) {
                n = count[ln.k];
                if (n > 0) {                                // n = 0: accum and accum2 are not read
                    acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
                    sq = mk(accum2[3 * ln.k], accum2[3 * ln.k + 1], accum2[3 * ln.k + 2]);
                }
                if (N.later && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            }
            park(park_rgb, ln.q, acc);
            park(park_sq, ln.q, sq);
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
            park_n[ln.q] = n;
        }
    }
    bool ran = false;
    for (uint32_t t = 0; t < N.count; ++t) {
        // what the wave's first lanes parked, before the loop or in the pass before, is read by every lane below
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const Lane ln = lane_of();
        const uint32_t n_px = park_n[ln.q];
        const bool go = ln.owner && !converge_stopped(parked(park_rgb, ln.q), parked(park_sq, ln.q), n_px, N.min_passes,
                                                      N.tolerance);
        const uint64_t live = __ballot(go);
        if (live == 0) break;
        ran = true;
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + n_px);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        if (after.owner && ((live >> l) & 1ull)) {          // nothing of a stopped pixel's ray reaches the state
            const int q = after.q;
            const uint32_t np = park_n[q];
            const d3 v2 = mk(col.x * col.x, col.y * col.y, col.z * col.z);
            const d3 acc = np == 0 ? col : add(parked(park_rgb, q), col);
            const d3 sq = np == 0 ? v2 : add(parked(park_sq, q), v2);
            park(park_rgb, q, acc);
            park(park_sq, q, sq);
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
            park_n[q] = np + 1u;
        }
    }
    const Lane ln = lane_of();
    bool open = false;                                      // the pixel is not stopped on its final state
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = parked(park_rgb, q), sq = parked(park_sq, q);
        const uint32_t n = park_n[q], seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        if (ran) {
            accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
            accum2[3 * k] = sq.x; accum2[3 * k + 1] = sq.y; accum2[3 * k + 2] = sq.z;
            count[k] = n;
        }
        if (N.last) {
            const double cnt = (double)n;
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
            open = !converge_stopped(acc, sq, n, N.min_passes, N.tolerance);
        } else if (orc2) {
            orc2[2 * k] = seg_sum; orc2[2 * k + 1] = sh_sum;
        }
    }
    if (N.last && active) {
        const uint64_t still = __ballot(open);
        if (still != 0 && threadIdx.x == 0) atomicAdd(active, (uint32_t)__popcll(still));
    }
}

// ---- Lists of windows (rt_render_accum_windows_dev, rt_render_converge_windows_dev, include/rt_api.h): the pixels of any
// set of disjoint windows of the frame in one launch, byte for byte what the un-windowed kernels give them. ----

// What a list kernel gets beside its parent's arguments: the prefix column of the launch's S (n + 1 words: the tiles
// before each window, then the launch's tile count), the entries (rt_layout.hpp DevWindow), the number of windows, the
// launch's tile count and the grid's row length (window_list_grid).
struct WindowListParams {
    const uint32_t* __restrict__ prefix;
    const rt::DevWindow* __restrict__ entries;
    uint32_t n, tiles, grid_x;
};

// What a wave of a list kernel keeps of its window: rt_accum_window_kernel's W.sx0 + 8 tx and W.sy0 + 8 ty already summed
// (the wave's sample origin in the frame), the window's far corner in samples, its stride, and the element number frame
// pixel (0, 0) would have (signed: a packed window far up the frame lies early in the buffers).
struct WindowTile {
    int32_t ox, oy;
    int32_t sx1, sy1;
    int32_t stride;
    int64_t base;
    bool pad;                                  // a wave past the launch's tile count (the fold's last row): stores nothing
};

// The wave's window and its tile within it, from its flat tile number: a binary search of the prefix column (prefix[k]
// <= flat < prefix[k + 1]: no window is empty, so the column rises strictly; at most 12 steps for 4096 windows), one load
// of that entry, one division by the window's tiles per row.  Everything here is formed from the block's number and
// kernel arguments alone, so it is wave-uniform: the loads are scalar loads and the results scalar registers
// (readfirstlane where a division went through the vector unit).  It runs once, before the first trace.
__device__ __forceinline__ WindowTile window_tile_of(const WindowListParams& T, int s) {
    uint32_t flat = blockIdx.y * T.grid_x + blockIdx.x;
    WindowTile r;
    r.pad = flat >= T.tiles;
    if (r.pad) flat = T.tiles - 1;                          // a valid tile to trace; nothing of it is stored
    uint32_t lo = 0, hi = T.n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T.prefix[mid] <= flat) lo = mid;
        else hi = mid;
    }
    const rt::DevWindow e = T.entries[lo];
    const uint32_t t = flat - T.prefix[lo];
    const uint32_t tiles_x = (uint32_t)(((e.width << s) + 7) >> 3);
    const uint32_t ty = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t / tiles_x));
    const uint32_t tx = t - ty * tiles_x;
    r.ox = (e.x0 << s) + (int32_t)(tx * 8u);
    r.oy = (e.y0 << s) + (int32_t)(ty * 8u);
    r.sx1 = (e.x0 + e.width) << s;
    r.sy1 = (e.y0 + e.height) << s;
    r.stride = e.stride;
    r.base = e.base;
    return r;
}

// rt_accum_window_kernel statement for statement, but for where the wave's tile comes from: window_tile_of in place of
// (W, blockIdx), and the element number k = base + (lr >> s) stride + (i >> s) with the list's signed base.  The waves
// of one window tile it from its own origin exactly as the single-window kernel's do, so a lane holds the same sample
// either way.  A kernel of its own, as rt_accum_window_kernel is.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_accum_windows_kernel(const DevScene* __restrict__ S,
                                                              const DevMotion* __restrict__ M, RenderParams P,
                                                              JitterParams Q, ShutterParams C, AccumParams N,
                                                              WindowListParams T, double aperture, double light_size,
                                                              double shutter, double* accum, void* o32, void* o8,
                                                              double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const WindowTile W = window_tile_of(T, s);
    // (rt_accum_kernel: the lane's coordinates are formed again wherever they are read)
    struct Lane { int i, lr, a, b, q; bool owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = W.ox + x;
        r.lr = W.oy + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.owner = r.a == 0 && r.b == 0 && r.i < W.sx1 && r.lr < W.sy1 && !W.pad;
        r.k = (size_t)(W.base + (int64_t)(r.lr >> s) * (int64_t)W.stride + (int64_t)(r.i >> s));   // read under `owner` only
        return r;
    };
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_rgb + 3 * npix);
    {
        const Lane ln = lane_of();
        if (ln.owner) {
            d3 acc = mk(0.0, 0.0, 0.0);
            uint32_t seg_sum = 0, sh_sum = 0;
            if (N.first > 0) acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
            if (N.first > N.call_first && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            park_rgb[ln.q] = acc.x; park_rgb[npix + ln.q] = acc.y; park_rgb[2 * npix + ln.q] = acc.z;
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
        }
    }
    for (uint32_t t = 0; t < N.count; ++t) {
        const uint32_t p = N.first + t;
        const Lane ln = lane_of();
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + p);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        if (after.owner) {
            const int q = after.q;
            const d3 acc = p == 0 ? col : add(mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]), col);
            park_rgb[q] = acc.x; park_rgb[npix + q] = acc.y; park_rgb[2 * npix + q] = acc.z;
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
        }
    }
    const Lane ln = lane_of();
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = mk(park_rgb[q], park_rgb[npix + q], park_rgb[2 * npix + q]);
        const uint32_t seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
        if (o32 || o8 || o64 || orc2) {
            const double cnt = (double)(N.first + N.count);
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
        }
    }
}

// rt_converge_window_kernel statement for statement with rt_accum_windows_kernel's tile lookup and element number.
// *active is added to by every wave of every window, so it counts the list's pixels.
template <int B, bool TRANSP, bool TREE>
__global__ __launch_bounds__(64) void rt_converge_windows_kernel(const DevScene* __restrict__ S,
                                                                 const DevMotion* __restrict__ M, RenderParams P,
                                                                 JitterParams Q, ShutterParams C, ConvergeParams N,
                                                                 WindowListParams T, double aperture, double light_size,
                                                                 double shutter, double* accum, double* accum2,
                                                                 uint32_t* count, uint32_t* active, void* o32, void* o8,
                                                                 double* o64, uint32_t* orc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = P.ss_log2, S1 = (1 << s) - 1, jl = Q.jl, sj = s + jl;
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    const WindowTile W = window_tile_of(T, s);
    // (rt_accum_kernel: the lane's coordinates are formed again wherever they are read)
    struct Lane { int i, lr, a, b, q; bool first, owner; size_t k; };
    const auto lane_of = [&]() {
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        const int x = l & 7, y = l >> 3;
        Lane r;
        r.i = W.ox + x;
        r.lr = W.oy + y;
        r.a = x & S1;
        r.b = y & S1;
        r.q = ((y >> s) << (3 - s)) + (x >> s);          // the pixel's number in the tile
        r.first = r.a == 0 && r.b == 0;
        r.owner = r.first && r.i < W.sx1 && r.lr < W.sy1 && !W.pad;
        r.k = (size_t)(W.base + (int64_t)(r.lr >> s) * (int64_t)W.stride + (int64_t)(r.i >> s));   // read under `owner` only
        return r;
    };
    const int npix = 64 >> (2 * s);
    double* park_rgb = reinterpret_cast<double*>(smem + (TREE ? 0 : slot_bytes(B, TRANSP, 64)));
    double* park_sq = park_rgb + 3 * npix;
    uint32_t* park_rc = reinterpret_cast<uint32_t*>(park_sq + 3 * npix);
    uint32_t* park_n = park_rc + 2 * npix;
    const auto parked = [&](const double* p, int q) { return mk(p[q], p[npix + q], p[2 * npix + q]); };
    const auto park = [&](double* p, int q, d3 v) { p[q] = v.x; p[npix + q] = v.y; p[2 * npix + q] = v.z; };
    {
        // every pixel slot of the tile is filled: a slot outside the window holds n = 0 and is never live
        const Lane ln = lane_of();
        if (ln.first) {
            d3 acc = mk(0.0, 0.0, 0.0), sq = mk(0.0, 0.0, 0.0);
            uint32_t n = 0, seg_sum = 0, sh_sum = 0;
            if (ln.owner) {
                n = count[ln.k];
                if (n > 0) {                                // n = 0: accum and accum2 are not read
                    acc = mk(accum[3 * ln.k], accum[3 * ln.k + 1], accum[3 * ln.k + 2]);
                    sq = mk(accum2[3 * ln.k], accum2[3 * ln.k + 1], accum2[3 * ln.k + 2]);
                }
                if (N.later && orc2) { seg_sum = orc2[2 * ln.k]; sh_sum = orc2[2 * ln.k + 1]; }
            }
            park(park_rgb, ln.q, acc);
            park(park_sq, ln.q, sq);
            park_rc[ln.q] = seg_sum; park_rc[npix + ln.q] = sh_sum;
            park_n[ln.q] = n;
        }
    }
    bool ran = false;
    for (uint32_t t = 0; t < N.count; ++t) {
        // what the wave's first lanes parked, before the loop or in the pass before, is read by every lane below
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const Lane ln = lane_of();
        const uint32_t n_px = park_n[ln.q];
        const bool go = ln.owner && !converge_stopped(parked(park_rgb, ln.q), parked(park_sq, ln.q), n_px, N.min_passes,
                                                      N.tolerance);
        const uint64_t live = __ballot(go);
        if (live == 0) break;
        ran = true;
        const int i = ln.i, lr = ln.lr, a = ln.a, b = ln.b;
        const int ic = i < P.width ? i : P.width - 1, j = lr < P.height ? lr : P.height - 1;
        const uint32_t w = rtj::jitter_word((uint32_t)lr * (uint32_t)P.width + (uint32_t)i, Q.seed + n_px);
        const int n = a + (b << s);                         // time index a + S b
        const double sigma = shutter * ((double)(2 * ((n << jl) + rtj::jitter_level(w, 6, jl)) + 1 - (1 << (s + sj))) *
                                        ldexp(1.0, -(s + sj)));
        // the camera of the lane's time
        const d3 eye = add(ld3(P.eye), scl(sigma, ld3(C.eye_move)));
        const d3 look = add(ld3(P.look), scl(sigma, ld3(C.look_move)));
        const d3 ld = sub(look, eye);
        const d3 right = cam_normalize(cross(ld, ld3(C.up)));
        const d3 upp = cam_normalize(cross(right, ld));
        // screen_point of the fine camera at that time
        const int fi = (ic << jl) + rtj::jitter_level(w, 0, jl), fj = (j << jl) + rtj::jitter_level(w, 1, jl);
        const d3 sp = add(add(look, scl(Q.pitch_f * (double)(fi + Q.bottom_fx), right)),
                          scl(Q.pitch_f * (double)(fj + Q.bottom_fy), upp));
        const double inv_sj = ldexp(1.0, -sj);
        const auto t_of = [&](int c, int kd) { return (double)(2 * ((c << jl) + kd) + 1 - (1 << sj)) * inv_sj; };
        const double ta = t_of(a, rtj::jitter_level(w, 2, jl)), tb = t_of(b, rtj::jitter_level(w, 3, jl));
        const double ga = t_of(a, rtj::jitter_level(w, 4, jl)), gb = t_of(b, rtj::jitter_level(w, 5, jl));
        const d3 e = add(add(eye, scl(aperture * ta, right)), scl(aperture * tb, upp));
        const double ex = e.x - S->bc[0], ey = e.y - S->bc[1], ez = e.z - S->bc[2];   // hits_ok_from, the swept proof
        V.hits_ok = (M->hits_inside != 0) & (ex * ex + ey * ey + ez * ez <= M->hits_lim2);
        const Motion mo{sigma, M};
        uint32_t seg = 0, sh = 0;
        d3 col = trace_generic<B, TRANSP, TREE, 64, true, true>(V, e, sp, smem, &seg, &sh,
                                                                LightShift{light_size * ga, light_size * gb}, &mo);
        reduce_samples(s, 8, col, seg, sh);
        const Lane after = lane_of();
        int l = threadIdx.x;
        asm volatile("" : "+v"(l));
        if (after.owner && ((live >> l) & 1ull)) {          // nothing of a stopped pixel's ray reaches the state
            const int q = after.q;
            const uint32_t np = park_n[q];
            const d3 v2 = mk(col.x * col.x, col.y * col.y, col.z * col.z);
            const d3 acc = np == 0 ? col : add(parked(park_rgb, q), col);
            const d3 sq = np == 0 ? v2 : add(parked(park_sq, q), v2);
            park(park_rgb, q, acc);
            park(park_sq, q, sq);
            park_rc[q] += seg;
            park_rc[npix + q] += sh;
            park_n[q] = np + 1u;
        }
    }
    const Lane ln = lane_of();
    bool open = false;                                      // the pixel is not stopped on its final state
    if (ln.owner) {
        const size_t k = ln.k;
        const int q = ln.q;
        const d3 acc = parked(park_rgb, q), sq = parked(park_sq, q);
        const uint32_t n = park_n[q], seg_sum = park_rc[q], sh_sum = park_rc[npix + q];
        if (ran) {
            accum[3 * k] = acc.x; accum[3 * k + 1] = acc.y; accum[3 * k + 2] = acc.z;
            accum2[3 * k] = sq.x; accum2[3 * k + 1] = sq.y; accum2[3 * k + 2] = sq.z;
            count[k] = n;
        }
        if (N.last) {
            const double cnt = (double)n;
            store_sampled(P, k, mk(acc.x / cnt, acc.y / cnt, acc.z / cnt), seg_sum, sh_sum, o32, o8, o64, orc2);
            open = !converge_stopped(acc, sq, n, N.min_passes, N.tolerance);
        } else if (orc2) {
            orc2[2 * k] = seg_sum; orc2[2 * k + 1] = sh_sum;
        }
    }
    if (N.last && active) {
        const uint64_t still = __ballot(open);
        if (still != 0 && threadIdx.x == 0) atomicAdd(active, (uint32_t)__popcll(still));
    }
}

// A launch of one of the kernels.
struct SampledLaunch {
    int variant;                               // trace_variant()
    hipStream_t stream;
    const DevScene* scene;
    RenderParams P;                            // the sample grid's (ss_log2 set)
    void* o32;
    void* o8;
    double* o64;
    uint32_t* orc2;
    // rt_refine_kernel
    unsigned grid;
    int out_w;
    const uint32_t* count;
    const uint32_t* list;
    // rt_lens_kernel (a kind leaves what it does not read at zero)
    double aperture;                           // half-width of the lens
    double light_size;                         // AREA: half-width of the lights' panels
    double shutter;                            // MOTION: share of the displacements the exposure covers
    const DevMotion* motion;                   // MOTION: the context's motion record (rt_set_motion)
    uint8_t* spread;                           // rt_lens_coarse_kernel: one byte per output pixel
    JitterParams jitter;                       // rt_jitter_kernel, rt_shutter_kernel
    ShutterParams camera;                      // rt_shutter_kernel, rt_accum_kernel
    // rt_accum_kernel: the launch's passes are first_pass .. first_pass + passes - 1 of the call that began at call_first
    uint32_t first_pass, passes, call_first;
    double* accum;                             // the running sums, 3 doubles per output pixel
    // rt_converge_kernel: at most `passes` passes per pixel; `later`: not the call's first launch, `last`: its last
    double* accum2;                            // the sums of squares, 3 doubles per output pixel
    uint32_t* npasses;                         // the pass counts, one word per output pixel
    uint32_t* active;                          // nullable: the pixels not stopped after the call
    uint32_t min_passes;
    double tolerance;
    bool later, last;
    // rt_accum_window_kernel, rt_converge_window_kernel: the window as the kernels take it; accum, accum2, npasses and
    // the four outputs then hold the pointers moved back to frame pixel (0, 0)
    WindowParams window;
    // rt_accum_windows_kernel, rt_converge_windows_kernel: the context's window table as the kernels take it (the
    // buffer pointers are the caller's, unmoved)
    WindowListParams windows;
};

// Defined once per depth B in rt_adaptive_b<B>.o (rt_adaptive.hip), per kind in rt_lens_k<kind>_b<B>.o (rt_lens.hip)
// the adaptive lens render's two in rt_lens_adaptive_b<B>.o (rt_lens_adaptive.hip), the jittered render's in
// rt_jitter_b<B>.o (rt_jitter.hip), the shutter render's in rt_shutter_b<B>.o (rt_shutter.hip) and the accumulating
// render's in rt_accum_b<B>.o (rt_accum.hip); the converging render's in rt_converge_b<B>.o (rt_converge.hip); their
// windowed forms in rt_accum_window_b<B>.o (rt_accum_window.hip) and rt_converge_window_b<B>.o (rt_converge_window.hip);
// the list forms in rt_accum_windows_b<B>.o (rt_accum_windows.hip) and rt_converge_windows_b<B>.o
// (rt_converge_windows.hip).
template <int B>
hipError_t launch_refine(const SampledLaunch& L);
template <int B>
hipError_t launch_lens_coarse(const SampledLaunch& L);
template <int B>
hipError_t launch_lens_refine(const SampledLaunch& L);
template <int B>
hipError_t launch_jitter(const SampledLaunch& L);
template <int B>
hipError_t launch_shutter(const SampledLaunch& L);
template <int B>
hipError_t launch_accum(const SampledLaunch& L);
template <int B>
hipError_t launch_converge(const SampledLaunch& L);
template <int B>
hipError_t launch_accum_window(const SampledLaunch& L);
template <int B>
hipError_t launch_converge_window(const SampledLaunch& L);
template <int B>
hipError_t launch_accum_windows(const SampledLaunch& L);
template <int B>
hipError_t launch_converge_windows(const SampledLaunch& L);
template <int B, bool AREA, bool MOTION>
hipError_t launch_lens(const SampledLaunch& L);
#define RT_DECLARE_SAMPLED(B)                                         \
    template <>                                                       \
    hipError_t launch_refine<B>(const SampledLaunch& L);              \
    template <>                                                       \
    hipError_t launch_lens_coarse<B>(const SampledLaunch& L);         \
    template <>                                                       \
    hipError_t launch_lens_refine<B>(const SampledLaunch& L);         \
    template <>                                                       \
    hipError_t launch_jitter<B>(const SampledLaunch& L);              \
    template <>                                                       \
    hipError_t launch_shutter<B>(const SampledLaunch& L);             \
    template <>                                                       \
    hipError_t launch_accum<B>(const SampledLaunch& L);               \
    template <>                                                       \
    hipError_t launch_converge<B>(const SampledLaunch& L);            \
    template <>                                                       \
    hipError_t launch_accum_window<B>(const SampledLaunch& L);        \
    template <>                                                       \
    hipError_t launch_converge_window<B>(const SampledLaunch& L);     \
    template <>                                                       \
    hipError_t launch_accum_windows<B>(const SampledLaunch& L);       \
    template <>                                                       \
    hipError_t launch_converge_windows<B>(const SampledLaunch& L);    \
    template <>                                                       \
    hipError_t launch_lens<B, false, false>(const SampledLaunch& L);  \
    template <>                                                       \
    hipError_t launch_lens<B, true, false>(const SampledLaunch& L);   \
    template <>                                                       \
    hipError_t launch_lens<B, true, true>(const SampledLaunch& L);
RT_DECLARE_SAMPLED(0) RT_DECLARE_SAMPLED(1) RT_DECLARE_SAMPLED(2) RT_DECLARE_SAMPLED(3)
RT_DECLARE_SAMPLED(4) RT_DECLARE_SAMPLED(5) RT_DECLARE_SAMPLED(6) RT_DECLARE_SAMPLED(7)
#undef RT_DECLARE_SAMPLED

// The scene kind's instance of a kernel template <B, TRANSP, TREE> with one-wave workgroups:
// launch(TRANSP, TREE, lds bytes) (two std::bool_constant) launches it.
template <int B, class Launch>
hipError_t launch_sampled(int variant, Launch&& launch) {
    if constexpr (B > RT_MAX_B) {
        return hipErrorInvalidValue;
    } else {
        if (variant == 2) launch(std::true_type{}, std::true_type{}, (size_t)0);
        else if (variant == 1) launch(std::true_type{}, std::false_type{}, (size_t)slot_bytes(B, true, 64));
        else launch(std::false_type{}, std::false_type{}, (size_t)slot_bytes(B, false, 64));
        return hipGetLastError();
    }
}

template <int B>
hipError_t launch_refine_impl(const SampledLaunch& L) {
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_refine_kernel<B, decltype(transp)::value, decltype(tree)::value>), dim3(L.grid), dim3(64),
                           lds, L.stream, L.scene, L.P, L.out_w, L.count, L.list, L.o32, L.o8, L.o64, L.orc2);
    });
}

// The grid of rt_lens_kernel: one wave per 8 x 8 tile of the sample grid.
inline dim3 lens_grid(const RenderParams& P, int* tile_rows) {
    const int tiles_x = (P.width + 7) / 8;
    *tile_rows = (P.height + 7) / 8;
    return dim3((unsigned)tiles_x, (unsigned)std::min(*tile_rows, kDofGridY),
                (unsigned)((*tile_rows + kDofGridY - 1) / kDofGridY));
}

template <int B, bool AREA, bool MOTION>
hipError_t launch_lens_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_lens_kernel<B, decltype(transp)::value, decltype(tree)::value, AREA, MOTION>), g,
                           dim3(64), lds, L.stream, L.scene, L.motion, L.P, L.aperture, L.light_size, L.shutter,
                           tile_rows, L.o32, L.o8, L.o64, L.orc2);
    });
}

template <int B>
hipError_t launch_lens_coarse_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_lens_coarse_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64), lds,
                           L.stream, L.scene, L.motion, L.P, L.aperture, L.light_size, L.shutter, tile_rows, L.o32, L.o8,
                           L.o64, L.orc2, L.spread);
    });
}

template <int B>
hipError_t launch_lens_refine_impl(const SampledLaunch& L) {
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_lens_refine_kernel<B, decltype(transp)::value, decltype(tree)::value>), dim3(L.grid),
                           dim3(64), lds, L.stream, L.scene, L.motion, L.P, L.aperture, L.light_size, L.shutter, L.out_w,
                           L.count, L.list, L.o32, L.o8, L.o64, L.orc2);
    });
}

template <int B>
hipError_t launch_jitter_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_jitter_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64), lds,
                           L.stream, L.scene, L.motion, L.P, L.jitter, L.aperture, L.light_size, L.shutter, tile_rows,
                           L.o32, L.o8, L.o64, L.orc2);
    });
}

template <int B>
hipError_t launch_shutter_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_shutter_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64), lds,
                           L.stream, L.scene, L.motion, L.P, L.jitter, L.camera, L.aperture, L.light_size, L.shutter,
                           tile_rows, L.o32, L.o8, L.o64, L.orc2);
    });
}

// LDS of rt_accum_kernel's parked sums behind trace()'s slots: 3 doubles and 2 counters per output pixel of a tile.
inline size_t accum_park_bytes(int ss_log2) { return (size_t)(64 >> (2 * ss_log2)) * (3 * 8 + 2 * 4); }

template <int B>
hipError_t launch_accum_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    const AccumParams n{L.first_pass, L.passes, L.call_first};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_accum_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + accum_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera, n, L.aperture, L.light_size, L.shutter,
                           tile_rows, L.accum, L.o32, L.o8, L.o64, L.orc2);
    });
}

// LDS of rt_converge_kernel's parked state behind trace()'s slots: 6 doubles, 2 counters and the pass count per output
// pixel of a tile.
inline size_t converge_park_bytes(int ss_log2) { return (size_t)(64 >> (2 * ss_log2)) * (6 * 8 + 3 * 4); }

template <int B>
hipError_t launch_converge_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = lens_grid(L.P, &tile_rows);
    const ConvergeParams n{L.tolerance, L.passes, L.min_passes, L.later ? 1u : 0u, L.last ? 1u : 0u};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_converge_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + converge_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera,
                           n, L.aperture, L.light_size, L.shutter, tile_rows, L.accum, L.accum2, L.npasses, L.active,
                           L.o32, L.o8, L.o64, L.orc2);
    });
}

// The grid of the windowed kernels: lens_grid over the window's own sample extent.
inline dim3 window_grid(const WindowParams& w, int* tile_rows) {
    RenderParams e{};
    e.width = w.sx1 - w.sx0;
    e.height = w.sy1 - w.sy0;
    return lens_grid(e, tile_rows);
}

template <int B>
hipError_t launch_accum_window_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = window_grid(L.window, &tile_rows);
    const AccumParams n{L.first_pass, L.passes, L.call_first};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_accum_window_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + accum_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera, n,
                           L.window, L.aperture, L.light_size, L.shutter, tile_rows, L.accum, L.o32, L.o8, L.o64,
                           L.orc2);
    });
}

template <int B>
hipError_t launch_converge_window_impl(const SampledLaunch& L) {
    int tile_rows;
    const dim3 g = window_grid(L.window, &tile_rows);
    const ConvergeParams n{L.tolerance, L.passes, L.min_passes, L.later ? 1u : 0u, L.last ? 1u : 0u};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_converge_window_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + converge_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera,
                           n, L.window, L.aperture, L.light_size, L.shutter, tile_rows, L.accum, L.accum2, L.npasses,
                           L.active, L.o32, L.o8, L.o64, L.orc2);
    });
}

// The grid of the list kernels: one wave per tile of the list, `grid_x` (WindowListParams) of them per row of the grid;
// a last row that is not full is padded with waves that store nothing, as lens_grid's last slice is.
inline dim3 window_list_grid(const WindowListParams& t) {
    return dim3(std::min(t.tiles, t.grid_x), (t.tiles + t.grid_x - 1) / t.grid_x, 1u);
}

template <int B>
hipError_t launch_accum_windows_impl(const SampledLaunch& L) {
    const dim3 g = window_list_grid(L.windows);
    const AccumParams n{L.first_pass, L.passes, L.call_first};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_accum_windows_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + accum_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera, n,
                           L.windows, L.aperture, L.light_size, L.shutter, L.accum, L.o32, L.o8, L.o64, L.orc2);
    });
}

template <int B>
hipError_t launch_converge_windows_impl(const SampledLaunch& L) {
    const dim3 g = window_list_grid(L.windows);
    const ConvergeParams n{L.tolerance, L.passes, L.min_passes, L.later ? 1u : 0u, L.last ? 1u : 0u};
    return launch_sampled<B>(L.variant, [&](auto transp, auto tree, size_t lds) {
        hipLaunchKernelGGL((rt_converge_windows_kernel<B, decltype(transp)::value, decltype(tree)::value>), g, dim3(64),
                           lds + converge_park_bytes(L.P.ss_log2), L.stream, L.scene, L.motion, L.P, L.jitter, L.camera,
                           n, L.windows, L.aperture, L.light_size, L.shutter, L.accum, L.accum2, L.npasses, L.active,
                           L.o32, L.o8, L.o64, L.orc2);
    });
}

}  // namespace rtk
