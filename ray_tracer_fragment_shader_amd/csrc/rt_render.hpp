// rt_render.hpp — the per-pixel render kernel and the ray-list kernel (templates), shared by the units of the C ABI
// that launch them (rt_plain.hip, rt_rays.hip, rt_diag.hip; rt_ctx.hpp has the map) and the per-depth instance files
// rt_render_b<B>.hip.  The bounce depth B is a template parameter (the bounce loop is unrolled); each depth's instances
// live in their own translation unit so the eight depths compile in parallel (one file with all of them took > 5
// minutes of one core).
//
//   rt_render_kernel<B, LDS, MINW, TRANSP, CULL, WG, TREE>  one work-item per pixel, FP64, iterative bounce
//                             loop (rt_device.hpp).  Default: one-wave workgroups (WG = 64), each owning an
//                             8 x 8 pixel tile (square tiles keep a wave's rays coherent, so the __any early-out
//                             and the culling masks work for whole waves).  The scene is read through the
//                             scalar cache; the A/B variants with 256-thread workgroups (32 x 8 tiles) copy it
//                             into LDS once per workgroup (LDS = 1) or stage the output tile in LDS for 32-pixel
//                             row stores.  Per-level colours wait in LDS slots; stores go out per wave.
//                             SS = true (the last template parameter; rt_render_ss_dev): the same trace on the
//                             sample grid of a supersampled frame, and an epilogue that sums each pixel's S x S
//                             samples across the wave before the one store per pixel.
//   rt_trace_rays_kernel<B>   rayTraceRay on an arbitrary ray list (parity / fuzz / faithful-screen entry).
//
// Output pixel formats (RenderParams::fmt_f / fmt_8, wave-uniform): the float image is RGBA32F (16 B/px) or
// GRAY32F (4 B/px, the R channel: only for scenes proven achromatic, where R = G = B bit for bit); the byte
// image is RGBA8 (4 B/px), RGB8 (3 B/px) or GRAY8 (1 B/px, achromatic scenes).  The packed formats cut the
// bytes a frame moves over xGMI (rt_render_multi) or PCIe (rt_render_packed).
//
// Reference: /root/reference/Hw4/MySdlApplication.cpp (rayTraceScreen :1251-1324, rayTraceRay :1184-1249,
// intersection code :611-823, :1084-1113).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>

#include "../../include/rt_api.h"
#include "rt_device.hpp"

#ifndef RT_WAVE_TRACE
#define RT_WAVE_TRACE 0
#endif
#ifndef RT_ABLATE
#define RT_ABLATE 0                            // instruction-count ablation builds (tools/ablate.sh): 1 prologue, 2 no stores
#endif
#ifndef RT_WG_FAST
#define RT_WG_FAST 64                          // workgroup of the default render kernels: 64 (8 x 8) or 128 (16 x 8)
#endif
// The culling variant (>= kConeMin spheres): 7 waves per SIMD (72 VGPRs, 94 SGPRs with 30 spilled to VGPR lanes,
// 12 B/lane of scratch), which its LDS allows since the last level's colour stays in registers (colour_slots:
// 4.5 KB per workgroup at depth 3).  c5 -2.6% serial, -3.9% with 3 frames in flight against the same code at 6
// waves (77 VGPRs, no scratch; in-process A/B).
#ifndef RT_MINW_CULL
#define RT_MINW_CULL 7
#endif
// (depth 2 spills 12 B/lane at 7 waves even with the store position recomputed: 6 waves there, 75 VGPRs, no scratch)
__host__ __device__ constexpr int cull_min_waves(int B) { return B == 2 && RT_MINW_CULL > 6 ? 6 : RT_MINW_CULL; }
// Launch-bound waves per SIMD of the bounded fast instances of depth B (the culling ones': cull_min_waves): 6 up to
// depth 2 (<= 80 VGPRs, no spills since the bounce loop stopped carrying the previous ray through the light loop), 5
// from depth 3 (<= 96 VGPRs; 6 would spill 8 B/lane).  The bound is a floor: the depth 1 and 2 kernels come out at 63 / 67 VGPRs under it (8 / 7 waves by VGPRs; the c2 kernel
// accumulates its colour in LDS, shade ACC) and their SGPR cap (rt_render_kernel_sg, 96) gives them 7 waves per
// SIMD on the hardware; r03's bound of 7 made the compiler trade SGPR spills (v_writelane) for the same VGPRs and
// ran c2 +2.3% slower (same-box A/B).
__host__ __device__ constexpr int fast_min_waves(int B) { return B <= 2 ? 6 : 5; }
// RT_MAX_B < 7 (experiment builds only, tools/variants.sh): deeper kernels are not instantiated.
#ifndef RT_MAX_B
#define RT_MAX_B 7
#endif
// The most mask slots per tile the cache holds (B ray masks + (B + 1) nl shadow masks); beyond it the masks are computed.
constexpr int kLevelMaskSlotsMax = 24;

namespace rtk {

using namespace rt;

constexpr int kTileW = 32;   // workgroup tile of the 256-thread variants: 32 columns ...
constexpr int kTileH = 8;    // ... x 8 rows = 256 pixels
static_assert(kThreads == kSlotStride, "one LDS colour slot column per work-item");
constexpr int kGridY = 32768;                  // grid.y per grid.z slice

// Pixel formats of the kernel's two images (include/rt_api.h RT_PIXEL_*).
constexpr int kFmtF_RGBA = 0, kFmtF_GRAY = 1;                // float image
constexpr int kFmt8_RGBA = 0, kFmt8_RGB = 1, kFmt8_GRAY = 2;  // byte image

// LDS bytes of trace()'s per-level slots for depth B: 3 doubles per colour slot (colour_slots: one per level,
// plus one for the parked continuation when the colour accumulates in LDS) and the material id per level when
// TRANSP, per work-item of a `wg`-thread workgroup.
__host__ __device__ constexpr int slot_bytes(int B, bool transp, int wg = kSlotStride, bool cull = false) {
    return (colour_slots(B, transp, cull) * 3 * 8 + (transp ? (B + 1) * 4 : 0)) * wg;
}
static_assert(slot_bytes(3, false, 64, true) == 4608 && slot_bytes(3, true, 64, true) == slot_bytes(3, true, 64) &&
                  slot_bytes(3, true, 64) == 7168 && slot_bytes(0, false) == 6144,
              "the launches' LDS: 3 B doubles per work-item for opaque culling, 3 (B + 1) and B + 1 ints for transparent");

// Slot of dispatch position L (linear workgroup id) in the dispatch table of n positions: grouped by L mod 8, the XCD
// the round-robin dispatcher sends workgroup L to (up to a per-launch rotation), so each XCD reads a contiguous run
// of the table and no L2 line is fetched by more than one XCD.
__host__ __device__ __forceinline__ size_t cone_slot(size_t L, size_t n) { return (L & 7) * ((n + 7) >> 3) + (L >> 3); }
__host__ __device__ __forceinline__ size_t cone_slots(size_t n) { return ((n + 7) >> 3) << 3; }

// One dispatch position of a calibrated view (rt_plain.hip rt_disp_kernel): the tile its workgroup traces
// (ty << 16 | tx), that tile's primary cone mask and its sky verdict (0: trace; r >= 1: no primary ray of the r tiles
// tx .. tx + r - 1 of that tile row hits anything — r = 1 in the plain table, up to the run maximum in the run-compacted
// one, rt_run_disp_kernel; both valid when RenderParams::cone_use).  The table is indexed by cone_slot(position): one
// 16-byte scalar load per wave brings all three.
// The top bit of `sky` (run lengths are at most 65,535) is the tile's class: set for a tracing tile of a fast-kernel view
// that is sphere-free (rt_cone.hpp tile_sphere_free: neither its cone mask nor any of its level masks keeps a sphere),
// which the fast kernels then trace without the sphere code (render_body).  Never set in a sky record.
struct alignas(16) DispRec {
    uint32_t cone_lo, cone_hi;
    uint32_t tile;
    uint32_t sky;
};
// Bit 30 (kDispFlat) marks a sphere-free tile that is also flat (rt_device.hpp trace_flat; decided by rt_plain.hip
// rt_flat_kernel at calibration): set only together with the top bit, in the records of the same instances' views.
// (Both constants, kDispSphereFree and kDispFlat, and the word's construction are in rt_cone.hpp: disp_sky_word, which the
// host evaluates too.)
// Which fast one-wave opaque instances read the class bit (render_body) — and so which views' records may carry it
// (rt_plain.hip render_build_dispatch; an instance that does not read it would take the bit for a run length): the RGBA
// instances of every depth and the packed ones up to depth 1.  Not the packed instances beyond depth 1: the second trace
// cost the SGPR-capped achromatic packed depth-2 kernel 6 SGPR spills and a 65th VGPR, so its code stays as it was.  Not
// the supersampled ones: their views keep the plain table and were left alone.
__host__ __device__ constexpr bool class_instance(bool packed, bool ss, int B) { return !ss && !(packed && B >= 2); }

struct RenderParams {
    double eye[3];
    double look[3];
    double right[3];
    double upp[3];
    double pitch;
    int32_t bottom_x, bottom_y;
    int32_t width, height;
    int32_t local_rows;                        // over all frames
    int32_t frame_rows;                        // local rows per frame
    int32_t frames;
    int32_t band_height, n_ranks, rank;
    int32_t lds_bytes;
    int32_t np;
    int32_t nl;
    int32_t wg_staging;                        // 1: stage the 32 x 8 tile in LDS behind a workgroup barrier
    int32_t fmt_f;                             // kFmtF_*: float image format
    int32_t fmt_8;                             // kFmt8_*: byte image format
    float look32[3], right32[3], upp32[3], eye32[3], pitch32;   // FP32 camera for primary_cone_mask
    float cone_slack;                          // its error bound (render_params)
    const DispRec* disp;                       // dispatch table (nullptr: identity order; the kernel reads its argument)
    uint32_t* tile_cost;                       // calibration render: each tile's wave time (100 MHz), by tile
    int32_t tile_rows_n;                       // tile rows of this launch
    int32_t tiles_x;                           // tiles per tile row (= grid.x)
    uint64_t* wtrace;                          // RT_WAVE_TRACE builds: per-wave {start, end, HW_ID}
    int32_t cone_use;                          // 1: disp's cone masks are this view's (cached primary cone masks)
    int32_t sky;                               // 1: sky tiles take the early-out (RT_SKY_TILES; in cone_use's padding)
    uint64_t* cone_out;                        // calibration render: each tile's mask, by tile, then each tile's sky
                                               // verdict (tile_rows_n * tiles_x further on), or nullptr
    int32_t ns;                                // stride of the scene's per-sphere arrays (DevScene::n_stride)
    // Per-tile level masks (rt_device.hpp LevelMasks; culling kernels, one-wave tiles): lmask_stride slots per tile,
    // written by the calibration render (lmask_out) and read by later renders of exactly that view (lmask_in)
    uint64_t* lmask_out;
    const uint64_t* lmask_in;
    int32_t lmask_stride;
    // Supersampled instances (render_body SS): log2 of the samples per axis S.  The other fields then describe the
    // sample grid (width = S x the output's, local_rows = S x its rows); the epilogue sums each pixel's S x S
    // samples in the wave and stores the output pixel.  (In the struct's tail padding: no other field moves.)
    int32_t ss_log2;
};

// The dispatch table's geometry, scalar arguments right after the table, so that gfx950's kernarg preload
// (-mllvm -amdgpu-kernarg-preload-count=4, Makefile KERNARG_PRELOAD) can hand both to the wave in SGPRs and its
// first memory access is its dispatch record.  Measured (r05, tools/ab_libs.py, 9 rounds): preloading 4 or 6
// dwords within +-0.8% of none at c2 / c3 / c5 (and the preloaded registers cost 20 more SGPR spills), so off.
struct DispGeom {
    int32_t tiles_x;                           // dispatch positions per grid row (= grid.x: the tiles per tile row, or
                                               // the run-compacted table's own width)
    int32_t n;                                 // dispatch positions with a record (tile rows x tiles per row, or the
                                               // run-compacted table's count)
};

// The render kernels' arguments, in order: the kernel-argument segment lays them out as this struct (each at its
// natural alignment), which late_outputs() relies on.  (The kernels take them as separate parameters: one
// by-value struct parameter measured +11 VGPRs in the culling kernel.)
struct RenderArgs {
    const DispRec* disp;                       // dispatch table (nullptr: identity order)
    int32_t tiles_x, n_disp;                   // its DispGeom (scalars: aggregates are not preloaded)
    const DevScene* scene;
    RenderParams P;
    void* o32;                                 // float image (RGBA32F / GRAY32F) or nullptr
    void* o8;                                  // byte image (RGBA8 / RGB8 / GRAY8) or nullptr
    double* o64;                               // RGB64F parity image or nullptr
    uint32_t* orc;                             // per-pixel ray counters or nullptr
};

// The output pointers, read from the kernel-argument segment where the stores need them: scalar loads behind an
// opaque copy of the segment pointer, so the compiler cannot hoist them to the kernel's start and hold 8 SGPRs
// through the whole trace (the SGPR budget of a seventh wave per SIMD).
struct RenderOuts {
    void* o32;
    void* o8;
    double* o64;
    uint32_t* orc;
};
__device__ __forceinline__ RenderOuts late_outputs() {
    typedef const __attribute__((address_space(4))) char* kptr;
    typedef void* const __attribute__((address_space(4)))* kpp;
    kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    RenderOuts o;
    o.o32 = *(kpp)(ka + offsetof(RenderArgs, o32));
    o.o8 = *(kpp)(ka + offsetof(RenderArgs, o8));
    o.o64 = (double*)*(kpp)(ka + offsetof(RenderArgs, o64));
    o.orc = (uint32_t*)*(kpp)(ka + offsetof(RenderArgs, orc));
    return o;
}

}  // namespace rtk

// The level-mask arrays of the render (RenderParams::lmask_in / lmask_out, rt_device.hpp LevelMasks), read from the
// kernel-argument segment where a mask is needed (behind an opaque copy of the segment pointer, as late_outputs).
namespace rt {
using rtk::RenderArgs;
using rtk::RenderParams;
__device__ __forceinline__ const uint64_t* level_masks_in() {
    typedef const __attribute__((address_space(4))) char* kptr;
    typedef const uint64_t* const __attribute__((address_space(4)))* kpp;
    kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(kpp)(ka + offsetof(RenderArgs, P) + offsetof(RenderParams, lmask_in));
}
__device__ __forceinline__ uint64_t* level_masks_out() {
    typedef const __attribute__((address_space(4))) char* kptr;
    typedef uint64_t* const __attribute__((address_space(4)))* kpp;
    kptr ka = (kptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(kpp)(ka + offsetof(RenderArgs, P) + offsetof(RenderParams, lmask_out));
}
}  // namespace rt

namespace rtk {

// Image row (within its frame) of local row lr; local rows are frame-major (rt_rows.frames).
__device__ __forceinline__ int global_row_of(const RenderParams& P, int lr) {
    if (P.frames > 1) lr %= P.frame_rows;
    if (P.n_ranks <= 1) return lr;
    int band = lr / P.band_height, within = lr - band * P.band_height;
    return (band * P.n_ranks + P.rank) * P.band_height + within;
}

// Copy the scene record into LDS, 16 B per work-item per step.
__device__ __forceinline__ void stage_scene(char* dst, const DevScene* __restrict__ src, int bytes) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (int k = threadIdx.x; k < (bytes >> 4); k += kThreads) d[k] = s[k];
}

// floor(clamp(c, 0, 1) * 255 + 0.5) (RGBA8 definition).  fmax/fmin (v_max/v_min_f64) clamp
// exactly like the comparisons; NaN becomes 0 (the conversion of a NaN is 0 on the device as well).
__device__ __forceinline__ unsigned char to_u8(double c) {
    double v = fmin(fmax(c, 0.0), 1.0);
    return (unsigned char)(int)floor(v * 255.0 + 0.5);
}

// Store pixel k of the two images in their formats.  PACKED = false: RGBA32F / RGBA8 only (the benchmark
// kernels: the runtime format branches cost c3 8% through the whole kernel's register allocation, same-box
// A/B); PACKED = true: fmt_f / fmt_8 are kernel arguments (scalar branches).
// (store_pixel_fmt: the formats as values, for code without the RenderParams at hand)
template <bool PACKED>
__device__ __forceinline__ void store_pixel_fmt(int fmt_f, int fmt_8, size_t k, d3 col, void* __restrict__ out32,
                                                void* __restrict__ out8) {
    if (out32) {
        if (PACKED && fmt_f == kFmtF_GRAY) {
            reinterpret_cast<float*>(out32)[k] = (float)col.x;
        } else {
            float* o = reinterpret_cast<float*>(out32) + 4 * k;   // (non-temporal: the frame is not read back here)
            __builtin_nontemporal_store((float)col.x, o);
            __builtin_nontemporal_store((float)col.y, o + 1);
            __builtin_nontemporal_store((float)col.z, o + 2);
            __builtin_nontemporal_store(1.0f, o + 3);
        }
    }
    if (out8) {
        if (PACKED && fmt_8 == kFmt8_GRAY) {
            reinterpret_cast<uint8_t*>(out8)[k] = to_u8(col.x);
        } else if (PACKED && fmt_8 == kFmt8_RGB) {
            uint8_t* o = reinterpret_cast<uint8_t*>(out8) + 3 * k;
            o[0] = to_u8(col.x);
            o[1] = to_u8(col.y);
            o[2] = to_u8(col.z);
        } else {
            const uint32_t px = (uint32_t)to_u8(col.x) | ((uint32_t)to_u8(col.y) << 8) |
                                ((uint32_t)to_u8(col.z) << 16) | (255u << 24);
            __builtin_nontemporal_store(px, reinterpret_cast<uint32_t*>(out8) + k);
        }
    }
}

template <bool PACKED>
__device__ __forceinline__ void store_pixel(const RenderParams& P, size_t k, d3 col, void* __restrict__ out32,
                                            void* __restrict__ out8) {
    store_pixel_fmt<PACKED>(P.fmt_f, P.fmt_8, k, col, out32, out8);
}

// The stores of a run of sky tiles (render_body's run branch; one-wave 8 x 8 tiles): the miss constants — colour 0, one
// ray segment, no shadow ray — of tiles tx .. tx + run - 1 of tile row ty into every output that is present, in its
// format, under the epilogue's per-pixel width and local-row checks.  One store step per tile of the run.  ROWS: a
// group of eight tiles that lies wholly in the run goes out row by row — step y of the group stores row y, 64
// consecutive pixels per store instruction (1 KB of RGBA32F, 256 B of RGBA8: whole lines) instead of eight 8-pixel
// segments — and the remainder tile by tile; the same bytes.  The run length and the loop are scalar.
template <bool PACKED, bool ROWS>
__device__ __forceinline__ void store_sky_run(const RenderOuts O, int width, int local_rows, int fmt_f, int fmt_8, int tx,
                                              int ty, int run, int lane) {
    for (int t = 0; t < run; ++t) {
        const bool rows = ROWS && (t | 7) < run;
        const int i_r = rows ? (tx + (t & ~7)) * 8 + lane : (tx + t) * 8 + (lane & 7);
        const int lr_r = ty * kTileH + (rows ? (t & 7) : (lane >> 3));
        if (i_r < width && lr_r < local_rows) {
            const size_t k = (size_t)lr_r * width + i_r;
            store_pixel_fmt<PACKED>(fmt_f, fmt_8, k, mk(0.0, 0.0, 0.0), O.o32, O.o8);
            if (O.o64) { O.o64[3 * k] = 0.0; O.o64[3 * k + 1] = 0.0; O.o64[3 * k + 2] = 0.0; }
            if (O.orc) O.orc[k] = 1u;
        }
    }
}
// ... as a function of its own, for the culling kernels: inlined into them, in either form, the run branch moved the
// register allocation of their tracing path (7-wave instances of depth 1 and 3: 12 B/lane of scratch with the row form;
// achromatic depth-2 instances: 71 -> 73 VGPRs, 7 -> 6 waves, even tile by tile).  Called, it is a few arguments and a
// return.  The kernel reads the output pointers and hands them over: the kernel-argument segment pointer is the kernel's
// alone (in a called function the builtin behind late_outputs() compiles to a null pointer).  Arguments travel in vector
// registers, so the wave-uniform ones are made scalars again.
template <bool PACKED, bool ROWS>
__device__ __attribute__((noinline)) void store_sky_run_call(const RenderOuts O, int width, int local_rows, int fmt_f,
                                                             int fmt_8, int tx, int ty, int run, int lane) {
    const auto uni = [](int v) { return __builtin_amdgcn_readfirstlane(v); };
    store_sky_run<PACKED, ROWS>(O, uni(width), uni(local_rows), uni(fmt_f), uni(fmt_8), uni(tx), uni(ty), uni(run), lane);
}

// ---- The sample-grid contract of include/rt_api.h (rt_render_ss_dev), spelled once for render_body's supersampled
// instances and the two list-free sampled kernels of rt_sampled.hpp (rt_refine_kernel, rt_lens_kernel). ----

// Screen point of pixel (ic, j) of the frame P describes (for a sampled render: the sample grid),
//     sp = (look + (pitch (ic + bottom_x)) right) + (pitch (j + bottom_y)) up',
// one IEEE operation per parenthesis and component, in this order (-ffp-contract=off): the end of the primary ray
// Line(camera, sp), SURVEY.md Appendix B (basis: rayTraceScreen :1270-1279).
__device__ __forceinline__ d3 screen_point(const RenderParams& P, int ic, int j, d3 right, d3 upp) {
    return add(add(ld3(P.look), scl(P.pitch * (double)(ic + P.bottom_x), right)),
               scl(P.pitch * (double)(j + P.bottom_y), upp));
}

// The S x S samples of a pixel, S = 2^s, one per lane: sample (a, b) sits a lanes and b * stride lanes past the
// pixel's first lane (stride 8 in an 8 x 8 tile of the sample grid, S where a pixel's samples are consecutive lanes).
// Colour and the two ray counters are summed per channel, the colour in FP64, as the fixed pairwise tree of
// include/rt_api.h: an xor butterfly with partners 1, 2, .. S/2 (along a), then stride, 2 stride, .. stride S/2
// (along b), every lane of the wave active; then the exact scale 1 / S^2 (a power of two).  IEEE addition is
// commutative bit for bit for non-NaN operands, so every lane of a pixel's block ends with the same bits, the
// contract's; a NaN's sign and payload may differ by lane: unspecified.
__device__ __forceinline__ void reduce_samples(int s, int stride, d3& col, uint32_t& seg, uint32_t& sh) {
    const auto step = [&](int m) {
        col.x += __shfl_xor(col.x, m);
        col.y += __shfl_xor(col.y, m);
        col.z += __shfl_xor(col.z, m);
        seg += __shfl_xor(seg, m);
        sh += __shfl_xor(sh, m);
    };
    // (one loop, whose step from S/2 goes on at stride: with stride = S it folds to plain doubling up to S^2 / 2)
    const int S = 1 << s;
    for (int m = 1; m <= stride * (S - 1); m = 2 * m == S ? stride : 2 * m) step(m);
    col = scl(ldexp(1.0, -2 * s), col);
}

// Store output pixel k of a sampled render: RGBA32F / RGBA8, RGB64F, and the counters as two words per pixel
// (summed over S^2 ray trees the packed 16 + 16-bit word of the plain render would overflow).
__device__ __forceinline__ void store_sampled(const RenderParams& P, size_t k, d3 col, uint32_t seg, uint32_t sh,
                                              void* o32, void* o8, double* o64, uint32_t* orc2) {
    store_pixel<false>(P, k, col, o32, o8);
    if (o64) { o64[3 * k] = col.x; o64[3 * k + 1] = col.y; o64[3 * k + 2] = col.z; }
    if (orc2) { orc2[2 * k] = seg; orc2[2 * k + 1] = sh; }
}

// rayTraceRay on Line(p0, p1) through the generic path: no per-tile cone or level masks, V.hits_ok as the caller set
// it.  lds: the workgroup's trace() slots (slot_bytes(B, TRANSP, WG); unused by ray trees).  AREA, ls: shade()'s (the
// lane's lights, MOTION, mo: its sphere centres).  (rt_trace_rays_kernel spells the call itself: its depth-3 FULL code differed.)
template <int B, bool TRANSP, bool TREE, int WG, bool AREA = false, bool MOTION = false>
__device__ __forceinline__ d3 trace_generic(const SceneView& V, d3 p0, d3 p1, char* lds, uint32_t* seg, uint32_t* sh,
                                            LightShift ls = LightShift{0.0, 0.0}, const Motion* mo = nullptr) {
    if constexpr (TREE) return trace_tree<B, AREA, MOTION>(V, p0, p1, seg, sh, ls, mo);
    else {
        double* slot = reinterpret_cast<double*>(lds) + threadIdx.x;
        int* mslot = reinterpret_cast<int*>(lds + 3 * 8 * colour_slots(B, TRANSP) * WG) + threadIdx.x;
        return trace<B, false, TRANSP, false, WG, false, AREA, MOTION>(V, p0, p1, ~0ull, seg, sh, slot, mslot, {-1}, ls, mo);
    }
}

template <int B, int LDS, int MINW, bool TRANSP, bool CULL, int WG = kThreads, bool TREE = false,
          bool PACKED = false, bool FIX64 = false, bool ACHRO = false, bool SS = false>
__device__ __forceinline__ void render_body(const DevScene* __restrict__ gscene, RenderParams P,
                                            const DispRec* __restrict__ disp, DispGeom geom) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
#if RT_WAVE_TRACE
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    const uint64_t t_cal = __builtin_amdgcn_s_memrealtime();   // used by calibration renders (P.tile_cost)
    // LDS: [header | DevSphere[np] | DevSpherePrim[np]] (LDS = 1), the per-level colour slots of trace()
    // (slot_bytes), then the output staging tile (12 KB, RT_WG_STAGING only).
    // The scene record is broadcast into LDS once per workgroup; the FP32 filter images stay in global
    // memory and are read with wave-uniform indices (scalar loads, SGPR operands).
    int off = 0;
    const DevScene* S = gscene;
    if (LDS) {
        stage_scene(smem, gscene, P.lds_bytes);
        S = reinterpret_cast<const DevScene*>(smem);
        off = P.lds_bytes;
    }
    double* slot = reinterpret_cast<double*>(smem + off) + tid;
    int* mslot = reinterpret_cast<int*>(smem + off + 3 * 8 * colour_slots(B, TRANSP, CULL) * WG) + tid;
    off += slot_bytes(B, TRANSP, WG, CULL);
    float4* st32 = reinterpret_cast<float4*>(smem + off);                              // [8][32] 4 KB
    double* st64 = reinterpret_cast<double*>(smem + off + 4096);                        // [8][32][3] 6 KB
    uint32_t* strc = reinterpret_cast<uint32_t*>(smem + off + 4096 + 6144);             // [8][32] 1 KB
    uchar4* st8 = reinterpret_cast<uchar4*>(smem + off + 4096 + 6144 + 1024);           // [8][32] 1 KB
    if (LDS) __syncthreads();
    // the fast kernels (scenes with np < kConeMin) see the fixed array stride as a constant
    constexpr bool kFixed = !LDS && !TRANSP && !CULL && !TREE && WG == RT_WG_FAST && RT_WG_FAST != kThreads;
    // (FIX64: the culling instance for scenes whose arrays have the stride kCullStride, see rt_layout.hpp)
    const SceneView V = view_of(S, gscene, P.np, kFixed ? kFastStride : FIX64 ? kCullStride : P.ns, P.nl);

    const int wave = tid >> 6, lane = tid & 63;
    // The 32 x 8 tile (WG = 256) is cut into 4 wave blocks of 8 x 8 pixels (square blocks keep a wave's
    // rays coherent; 16 x 4 and 32 x 2 blocks measured no faster, and 32 x 2 slower at c5); WG = 64: one
    // wave, one 8 x 8 tile.
    constexpr int bw = 8, bh = 8, TW = WG / 8;
    const int bx0 = wave * bw, by0 = 0;
    const int cx = bx0 + (lane & 7);               // column inside the tile
    const int cy = lane >> 3;                      // row inside the tile
    const int bxd = blockIdx.x;                     // 2-D grid: tiles_x x tiles_y
    const int gy = (int)(blockIdx.z * kGridY + blockIdx.y);    // tile rows beyond kGridY go to grid.z
    // The tile of this dispatch position and (cached views) its primary cone mask: one 16-byte record of the
    // dispatch table (a const __restrict__ kernel argument: a scalar load issued beside the other argument loads),
    // or the identity order.  Padding positions of the last grid.z slice trace a clamped tile and store nothing (no
    // early return: a branch here kept the compiler from issuing the scene loads until the tile had arrived).
    int tx = bxd, ty_raw = gy;
    uint64_t cone_cached = 0;
    uint32_t sky_cached = 0;
    if (disp) {
        const size_t n = (size_t)geom.n, Lp = (size_t)gy * geom.tiles_x + bxd;
        const DispRec rec = disp[cone_slot(Lp < n ? Lp : n - 1, n)];   // (padding positions: in bounds, unused)
        asm volatile("" ::"s"(rec.cone_lo), "s"(rec.cone_hi), "s"(rec.tile), "s"(rec.sky));
        cone_cached = (uint64_t)rec.cone_lo | ((uint64_t)rec.cone_hi << 32);
        sky_cached = rec.sky;
        tx = (int)(rec.tile & 0xffffu);
        ty_raw = Lp < n ? (int)(rec.tile >> 16) : P.tile_rows_n;
    }
    const bool pad = (unsigned)ty_raw >= (unsigned)P.tile_rows_n;
    const int ty = pad ? P.tile_rows_n - 1 : ty_raw;
    // the stores' tile row: past every local row for padding positions (their bounds check fails), so no flag
    // needs to live through the trace
    const int ty_st = pad ? (1 << 27) : ty_raw;
    const int i = tx * TW + cx;
    const int lr = ty * kTileH + cy;
    const bool valid = i < P.width && lr < P.local_rows && !pad;
    (void)valid;                                   // (the direct stores recompute it from i_e, lr_e)
#if RT_WAVE_TRACE >= 2
    asm volatile("" ::"s"(ty));
    const uint64_t t_ty = __builtin_amdgcn_s_memrealtime();   // the tile row has arrived
#endif

    // Per-wave sphere culling (all lanes active here).  The block's rows must be contiguous image rows.
    uint64_t cone = ~0ull;
    // Sky tile (wave-uniform): no primary ray of the wave hits anything — the board provably missed (a proof like the
    // cone mask's: rt_cone.hpp board_edge_record) and no sphere left in the cone mask, which covers every sphere of a
    // scene of up to 64.  Opaque, mesh-free instances with one-wave tiles (the conditions of trace()'s lazy_u).
    constexpr bool kSkyInst = !TRANSP && !TREE && !LDS && WG == 64;
    // Sphere-free tiles (DispRec, kDispSphereFree): the fast one-wave opaque instances read the class bit of a cached
    // view's record; the records of every other instance's views never have it set, and their code is as it was.
    constexpr bool kClassInst = kSkyInst && !CULL && class_instance(PACKED, SS, B);
    const uint32_t sky_len = kClassInst ? sky_cached & ~kDispClassBits : sky_cached;
    bool sky = false;
    RT_COUNT(V.S, kCntWaves, 1);
    if (P.np >= kPrimaryConeMin && P.cone_use) {
        // the mask and the verdict this view's calibration render computed for this tile, in its dispatch record
        // (rt_disp_kernel): no cone phase
        cone = cone_cached;
        sky = kSkyInst && sky_len != 0;
    } else if (P.np >= kPrimaryConeMin) {
        // Within one frame global_row_of is increasing, so jb - ja == 7 means 8 consecutive rows.
        const int lr0 = ty * kTileH + by0, ja = global_row_of(P, lr0), jb = global_row_of(P, lr0 + bh - 1);
        const bool one_frame = P.frames <= 1 || lr0 / P.frame_rows == (lr0 + bh - 1) / P.frame_rows;
        const float hx = 0.5f * (float)(bw - 1), hy = 0.5f * (float)(bh - 1);
        bool board_miss = false;
        if (one_frame && jb - ja == bh - 1)
            cone = primary_cone_mask(V, P.look32, P.right32, P.upp32, P.eye32, P.pitch32,
                                     (float)(tx * TW + bx0 + P.bottom_x) + hx, (float)(ja + P.bottom_y) + hy,
                                     sqrtf(hx * hx + hy * hy), P.cone_slack, lane, &board_miss);
        RT_COUNT(V.S, kCntConeKept, __popcll(cone & sphere_bits(V.np)));
        sky = kSkyInst && P.sky && P.np <= 64 && board_miss && (cone & sphere_bits(V.np)) == 0;
        if (P.cone_out && tid == 0 && !pad) {                // lane 0, vector stores
            const size_t t = (size_t)ty * P.tiles_x + tx;
            P.cone_out[t] = cone;
            P.cone_out[(size_t)P.tile_rows_n * P.tiles_x + t] = sky;
        }
    }
#if RT_WAVE_TRACE >= 2
    asm volatile("" ::"s"(cone));
    const uint64_t t_cone = __builtin_amdgcn_s_memrealtime();   // the primary cone mask is known
#endif

    // Every lane traces (trace() reduces over the wave): lanes outside the frame trace a clamped pixel
    // and store nothing.
    // A sky wave skips the screen points, the board test and trace(), and stores what trace() returns for 64 misses:
    // colour 0, one ray segment, no shadow ray.  The epilogue below is the same for both.
    // (The verdict is made a scalar again — it went through per-lane values on its way — so that the branch is a
    // scalar one and no exec mask is held through trace().)
    sky = __builtin_amdgcn_readfirstlane((int)sky) != 0;
    // A cached view's sky record holds a run length (rt_cone.hpp sky_run_at; 1 in the plain table): the wave stores
    // the miss constants of tiles tx .. tx + run - 1 of its tile row — what the sky epilogue below stores, pixel by
    // pixel, under the same width and local-row checks — and retires: one prologue per run instead of one per tile.
    // A branch of its own ahead of the screen points, so that the tracing path below is compiled as it was; the run
    // length and the loop stay scalar (store_sky_run).  (The supersampled epilogue reduces over the wave: those views
    // keep the plain table.  Padding positions read the last record: ty_st puts their rows past every local row.)
    // The branch leaves before the P.tile_cost store below, and a cached render of the plain table (run = 1) takes it
    // too: a render that times its tiles never has cone_use set (render_plan_view: the cached branch never calibrates).
    // One that did would have to store its time here, or it would order the view by stale costs of the sky tiles.
#if RT_WAVE_TRACE
    // The wave's trace record, by dispatch position (a tile; in the run-compacted table a tile or a run — how many
    // there are: rt_diag_disp_count): 4 words per position, and (level 2) 3 more behind 4 words for every tile of the
    // frame, whatever the grid's shape: the buffer holds 7 words per tile, and positions never outnumber tiles.
    // Padding positions leave no record.
    const auto wave_trace = [&](uint64_t mid, uint64_t traced) {
        const size_t tiles = (size_t)P.tile_rows_n * P.tiles_x, n = disp ? (size_t)geom.n : tiles;
        const size_t w = (size_t)gy * (disp ? geom.tiles_x : P.tiles_x) + bxd;
        if (!P.wtrace || tid != 0 || w >= n || n > tiles) return;
        P.wtrace[4 * w] = t_start;
        P.wtrace[4 * w + 1] = __builtin_amdgcn_s_memrealtime();
        P.wtrace[4 * w + 3] = mid;
#if RT_WAVE_TRACE >= 2
        P.wtrace[4 * tiles + 3 * w] = t_ty;
        P.wtrace[4 * tiles + 3 * w + 1] = t_cone;
        P.wtrace[4 * tiles + 3 * w + 2] = traced;
#else
        (void)traced;
#endif
        // (HW_ID, the XCC id in bits 32 .. 35, and the position's tile — a run's first — as tx | ty << 14 from bit 36,
        // so that tools/wave_trace.py can split the waves by their tile's class)
        P.wtrace[4 * w + 2] = (uint64_t)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11)) |
                              ((uint64_t)(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11)) & 0xFu) << 32) |
                              ((uint64_t)((uint32_t)(tx & 0x3fff) | ((uint32_t)(ty & 0x3fff) << 14)) << 36);
    };
#endif
    if constexpr (kSkyInst && !SS) {
        if (sky && P.cone_use) {
            const int run = __builtin_amdgcn_readfirstlane((int)sky_len);
#if RT_WAVE_TRACE
            const uint64_t t_run = __builtin_amdgcn_s_memrealtime();   // the run is known; its stores next
#endif
            if constexpr (CULL)
                store_sky_run_call<PACKED, true>(late_outputs(), P.width, P.local_rows, P.fmt_f, P.fmt_8, tx,
                                                                   ty_st, run, lane);
            else
                store_sky_run<PACKED, true>(late_outputs(), P.width, P.local_rows, P.fmt_f, P.fmt_8, tx,
                                                              ty_st, run, lane);
#if RT_WAVE_TRACE
            wave_trace(t_run, t_run);
#endif
            return;
        }
    }
    uint32_t seg = 1, sh = 0;
    d3 col = mk(0.0, 0.0, 0.0);
#if RT_WAVE_TRACE
    uint64_t t_mid = __builtin_amdgcn_s_memrealtime();      // (a sky wave: its verdict is known)
#endif
    if (!sky) {
        const d3 eye = ld3(P.eye);
        const int ic = i < P.width ? i : P.width - 1, lrc = lr < P.local_rows ? lr : P.local_rows - 1;
        const int j = global_row_of(P, lrc);
        const d3 right = ld3(P.right), upp = ld3(P.upp);
        const d3 sp = screen_point(P, ic, j, right, upp);    // primary ray Line(camera, sp)
#if RT_WAVE_TRACE
        t_mid = __builtin_amdgcn_s_memrealtime();           // prologue done: the primary ray is formed
#endif
#if RT_ABLATE == 1
        // (instruction-count ablation builds only, tools/ablate.sh: the prologue alone — no trace, no stores)
        asm volatile("" ::"v"(sp.x), "v"(sp.y), "v"(sp.z), "s"(cone));
        return;
#endif
        LevelMasks lm{-1};
        if (!TRANSP && !TREE && P.lmask_stride > 0 && !pad)
            lm.tile = (ty * P.tiles_x + tx) * P.lmask_stride;
        if constexpr (TREE) {
            col = trace_tree<B>(V, eye, sp, &seg, &sh);
        } else if constexpr (kClassInst) {
            // A sphere-free tile of a cached view (its record's class bit, decided at calibration like the sky verdict;
            // read once, made a scalar, consumed by this branch — nothing of it lives through a trace): the same trace
            // compiled without the sphere loops and without the level-mask reads (trace NOSPH).  The prologue above and
            // the stores below are shared.
            // A flat tile (kDispFlat, set only beside the class bit): all 64 primary rays hit the board and nothing else
            // can happen to them — the straight-line path, trace_flat, which has the proof.
            const uint32_t cls = P.cone_use ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(sky_cached >> 30)) : 0u;
            if (cls == 3u)
                col = trace_flat<B, ACHRO>(V, eye, sp, &seg, &sh);
            else if (cls != 0u)
                col = trace<B, true, false, false, WG, ACHRO, false, false, true>(V, eye, sp, 0, &seg, &sh, slot, mslot);
            else
                col = trace<B, true, TRANSP, CULL, WG, ACHRO>(V, eye, sp, cone, &seg, &sh, slot, mslot, lm);
        } else {
            col = trace<B, true, TRANSP, CULL, WG, ACHRO>(V, eye, sp, cone, &seg, &sh, slot, mslot, lm);
        }
    }
#if RT_WAVE_TRACE >= 2
    asm volatile("" ::"v"(col.x), "v"(col.y), "v"(col.z));
    const uint64_t t_trace = __builtin_amdgcn_s_memrealtime();   // trace() done, the stores next
#endif
#if RT_ABLATE == 2
    asm volatile("" ::"v"(col.x), "v"(col.y), "v"(col.z), "v"(seg), "v"(sh));   // (ablation: trace, no stores)
    return;
#endif

    if (WG != kThreads || !P.wg_staging) {
        // Direct stores: each wave writes its 8 x 8 block as 8 row segments (128 B of RGBA32F each) and
        // retires without waiting at a workgroup barrier for slower waves of the tile.
        // The culling kernels recompute the pixel position for the stores from an opaque copy of the thread index
        // instead of keeping it live through trace(): in their 7-wave instances that is what keeps it out of scratch
        // (12 B/lane spilled at the prologue and reloaded for the stores otherwise).  The fast kernels keep it live.
        int tid_e = tid;
        if constexpr (CULL) asm volatile("" : "+v"(tid_e));
        const int lane_e = tid_e & 63;
        const int i_e = tx * TW + (tid_e >> 6) * bw + (lane_e & 7), lr_e = ty_st * kTileH + (lane_e >> 3);
        if constexpr (SS) {
            // Supersampled instance: lane (x, y) of the 8 x 8 tile holds sample (x mod S, y mod S) of output pixel
            // (tile_x * 8 / S + x / S, tile_row * 8 / S + y / S): reduce_samples with lane stride 8.
            static_assert(WG == 64 && !PACKED && !LDS, "supersampling: one-wave RGBA direct-store instances only");
            const int s = P.ss_log2, S1 = (1 << s) - 1;
            reduce_samples(s, 8, col, seg, sh);
            // P.width and P.local_rows are the sample frame's: S x the output's width and local rows, and S divides
            // 8, so an S x S block lies either wholly inside the sample frame or wholly outside it: the block of an
            // in-frame pixel never holds a clamped out-of-frame sample, and the test on the block's first lane is
            // the test on W and the output's local rows.  (Padding dispatch positions: lr_e is past every row.)
            if (((lane_e & 7) & S1) == 0 && ((lane_e >> 3) & S1) == 0 && i_e < P.width && lr_e < P.local_rows) {
                const RenderOuts O = late_outputs();
                const size_t k = (size_t)(lr_e >> s) * (size_t)(P.width >> s) + (size_t)(i_e >> s);
                store_sampled(P, k, col, seg, sh, O.o32, O.o8, O.o64, O.orc);
            }
        } else
        if (i_e < P.width && lr_e < P.local_rows) {
            const RenderOuts O = late_outputs();
            const size_t k = (size_t)lr_e * P.width + i_e;
            store_pixel<PACKED>(P, k, col, O.o32, O.o8);
            if (O.o64) { O.o64[3 * k] = col.x; O.o64[3 * k + 1] = col.y; O.o64[3 * k + 2] = col.z; }
            if (O.orc) O.orc[k] = seg | (sh << 16);
        }
        if (P.tile_cost && tid == 0 && ty_st < P.tile_rows_n)
            P.tile_cost[(size_t)ty_st * P.tiles_x + tx] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_cal);
#if RT_WAVE_TRACE
#if RT_WAVE_TRACE >= 2
        wave_trace(t_mid, t_trace);
#else
        wave_trace(t_mid, 0);
#endif
#endif
        return;
    }
    // Stage through LDS, then store whole tile rows (RGBA formats only: the host routes packed formats to the
    // direct-store variants).
    const RenderOuts O = late_outputs();
    void* const out32 = O.o32;
    void* const out8 = O.o8;
    double* const out64 = O.o64;
    uint32_t* const outrc = O.orc;
    const int ts = cy * kTileW + cx;
    if (out32) st32[ts] = make_float4((float)col.x, (float)col.y, (float)col.z, 1.0f);
    if (out64) { st64[3 * ts] = col.x; st64[3 * ts + 1] = col.y; st64[3 * ts + 2] = col.z; }
    if (outrc) strc[ts] = seg | (sh << 16);
    if (out8) st8[ts] = make_uchar4(to_u8(col.x), to_u8(col.y), to_u8(col.z), 255);
    __syncthreads();
    const int oy = tid >> 5, ox = tid & 31;
    const int gi = tx * kTileW + ox, glr = ty * kTileH + oy;
    if (gi < P.width && glr < P.local_rows && !pad) {                     // (A/B variant: pad kept)
        const size_t k = (size_t)glr * P.width + gi;
        if (out32) reinterpret_cast<float4*>(out32)[k] = st32[tid];
        if (out64) {
            out64[3 * k] = st64[3 * tid];
            out64[3 * k + 1] = st64[3 * tid + 1];
            out64[3 * k + 2] = st64[3 * tid + 2];
        }
        if (outrc) outrc[k] = strc[tid];
        if (out8) reinterpret_cast<uchar4*>(out8)[k] = st8[tid];
    }
    if (P.tile_cost && tid == 0 && !pad)
        P.tile_cost[(size_t)ty * P.tiles_x + tx] = (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_cal);
}

// (out32 .. outrc are read by late_outputs() from the argument segment, not through the parameters.)
// The parameter list must match RenderArgs field for field: kernarg_offsets_match below checks it at compile time.
template <int B, int LDS, int MINW, bool TRANSP, bool CULL, int WG = kThreads, bool TREE = false,
          bool PACKED = false, bool FIX64 = false, bool ACHRO = false, bool SS = false>
__global__ __launch_bounds__(WG, MINW) void rt_render_kernel(const DispRec* __restrict__ disp, int32_t tiles_x, int32_t n_disp,
                                                             const DevScene* __restrict__ gscene, RenderParams P,
                                                             void* out32, void* out8, double* out64, uint32_t* outrc) {
    render_body<B, LDS, MINW, TRANSP, CULL, WG, TREE, PACKED, FIX64, ACHRO, SS>(gscene, P, disp, DispGeom{tiles_x, n_disp});
}

// The same kernel with its SGPRs capped at RT_FAST_SGPRS (amdgpu_num_sgpr: a constant, hence a kernel of its
// own).  The hardware fits 7 one-wave workgroups per SIMD only up to 96 SGPRs per wave (the compiler's
// TotalSGPRs, VCC and friends included) and 8 only up to 78 (tools/mb_slots.cpp: 71 VGPRs with 96 SGPRs -> 7
// waves, 98 -> 6; 63 VGPRs with 78 -> 8, 86 -> 7) — the compiler's occupancy estimate assumes a larger SGPR file.
// r03: the cap cost 19 SGPR spills (+1.1%), so it was off.  r04: with the output pointers read at the stores
// (late_outputs), the fixed array stride of the fast kernels and the bounding-sphere delta formed where it is
// tested, the uncapped c2 kernel needs 98 SGPRs / 62 VGPRs and the capped one 94 / 63 with 2 spills: 7 waves per
// SIMD, c2 -1.7% and c3 -2.5% against the uncapped build (same-box in-process A/B, tools/ab_libs.py); a cap of 80
// (8 waves, 14 spills) ran +0.8%.
#ifndef RT_FAST_SGPRS
#define RT_FAST_SGPRS 96
#endif
// (the same parameter list as rt_render_kernel: RenderArgs, checked below)
template <int B, int MINW, bool CULL, bool PACKED, bool ACHRO = false>
__global__ __launch_bounds__(RT_WG_FAST, MINW) __attribute__((amdgpu_num_sgpr(RT_FAST_SGPRS)))
void rt_render_kernel_sg(const DispRec* __restrict__ disp, int32_t tiles_x, int32_t n_disp,
                         const DevScene* __restrict__ gscene, RenderParams P, void* out32, void* out8, double* out64,
                         uint32_t* outrc) {
    render_body<B, 0, MINW, false, CULL, RT_WG_FAST, false, PACKED, false, ACHRO>(gscene, P, disp, DispGeom{tiles_x, n_disp});
}

// late_outputs() reads the output pointers at offsetof(RenderArgs, ...) of the kernel-argument segment, which lays the
// kernels' parameters out in order, each at its natural alignment.  The offsets of both kernels' actual parameter
// lists are computed here from their types and compared with RenderArgs: adding, reordering or re-typing a parameter
// (or a RenderParams change that moves the pointers) fails to compile instead of storing through a wrong pointer.
template <typename... A>
struct KernargLayout {
    static constexpr size_t offset(size_t i) {
        constexpr size_t sz[] = {sizeof(A)...}, al[] = {alignof(A)...};
        size_t off = 0;
        for (size_t k = 0;; ++k) {
            off = (off + al[k] - 1) / al[k] * al[k];
            if (k == i) return off;
            off += sz[k];
        }
    }
};
template <typename... A>
constexpr bool kernarg_offsets_match(void (*)(A...)) {
    using K = KernargLayout<A...>;
    return sizeof...(A) == 9 && K::offset(0) == offsetof(RenderArgs, disp) &&
           K::offset(1) == offsetof(RenderArgs, tiles_x) && K::offset(2) == offsetof(RenderArgs, n_disp) &&
           K::offset(3) == offsetof(RenderArgs, scene) && K::offset(4) == offsetof(RenderArgs, P) &&
           K::offset(5) == offsetof(RenderArgs, o32) && K::offset(6) == offsetof(RenderArgs, o8) &&
           K::offset(7) == offsetof(RenderArgs, o64) && K::offset(8) == offsetof(RenderArgs, orc);
}
// (The kernels are named inside decltype, an unevaluated operand: their types are all the check needs, so no
// translation unit instantiates or emits a kernel for it.)
static_assert(kernarg_offsets_match(decltype(&rt_render_kernel<1, 0, 1, false, false>){}),
              "rt_render_kernel's parameters must lay out as RenderArgs (late_outputs)");
static_assert(kernarg_offsets_match(decltype(&rt_render_kernel_sg<1, 1, false, false>){}),
              "rt_render_kernel_sg's parameters must lay out as RenderArgs (late_outputs)");

// rayTraceRay on a list of rays Line(starts[k], ends[k]).  Rays from arbitrary starts: whether their hit
// points may skip the bounding-sphere cull is decided per ray (hits_ok_from).
// Screen mode (spix != nullptr, rt_render_screen's chunks): every ray starts at starts[0..2] (the camera) and ends at
// its pixel's screen point + 0.5 * its jitter value (MSA:1296), formed here instead of by a launch of its own.
template <int B, bool TRANSP, bool TREE = false, int WG = kThreads>
__global__ __launch_bounds__(WG) void rt_trace_rays_kernel(const DevScene* __restrict__ S,
                                                                 const double* __restrict__ starts,
                                                                 const double* __restrict__ ends, int n,
                                                                 double* __restrict__ rgb,
                                                                 uint32_t* __restrict__ rc,
                                                                 const ScreenPix* __restrict__ spix, int sm,
                                                                 const int32_t* __restrict__ sfirst,
                                                                 const double* __restrict__ sjit, int scene_lds,
                                                                 uint32_t* __restrict__ sdone, uint32_t sseq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // Every lane traces (trace() reduces over the wave); lanes past n repeat ray n - 1 and store nothing.
    const int k = blockIdx.x * WG + threadIdx.x, kk = k < n ? k : n - 1;
    uint32_t seg = 0, sh = 0;
    // scene_lds > 0 (small launches: rt_render_screen's chunks): the whole scene record is copied into LDS first —
    // one burst of loads instead of a cold-cache round trip per record on the rays' dependent chain.  (The slots
    // behind it stay 8-byte aligned: scene_lds is a multiple of 8.)
    int off = 0;
    if (scene_lds > 0) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(S);
        uint32_t* dst = reinterpret_cast<uint32_t*>(smem);
        for (int q = threadIdx.x; q < (scene_lds >> 2); q += WG) dst[q] = src[q];
        __syncthreads();
        S = reinterpret_cast<const DevScene*>(smem);
        off = scene_lds;
    }
    SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    d3 p0, p1;
    if (spix) {
        p0 = ld3(starts);
        int q = sfirst[blockIdx.x];                         // the pixel of the workgroup's first ray (WG = kScreenBlock)
        while (q + 1 < sm && spix[q + 1].off <= kk) ++q;
        const ScreenPix& X = spix[q];
        const double* J = sjit + 3 * (size_t)(X.base + (kk - X.off));
        p1 = d3{X.sp[0] + 0.5 * J[0], X.sp[1] + 0.5 * J[1], X.sp[2] + 0.5 * J[2]};
    } else {
        p0 = ld3(starts + 3 * kk);
        p1 = ld3(ends + 3 * kk);
    }
    V.hits_ok = hits_ok_from(S, p0);
    double* slot = reinterpret_cast<double*>(smem + off) + threadIdx.x;
    int* mslot = reinterpret_cast<int*>(smem + off + 3 * 8 * colour_slots(B, TRANSP) * WG) + threadIdx.x;
    d3 c;
    if constexpr (TREE)
        c = trace_tree<B>(V, p0, p1, &seg, &sh);
    else
        c = trace<B, false, TRANSP, false, WG>(V, p0, p1, ~0ull, &seg, &sh, slot, mslot);
    if (k < n) {
        if (rgb) { rgb[3 * k] = c.x; rgb[3 * k + 1] = c.y; rgb[3 * k + 2] = c.z; }
        if (rc) rc[k] = seg | (sh << 16);
    }
    if (sdone) {                                        // screen chunks: this workgroup's colours are out
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(sdone + blockIdx.x, sseq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The screen-mode arguments of a trace launch (all null: a plain ray list).
struct ScreenArgs {
    const ScreenPix* pix = nullptr;
    int m = 0;
    const int32_t* first = nullptr;
    const double* jit = nullptr;
    int scene_lds = 0;                 // bytes of the scene record copied into LDS (multiple of 4; 0: none)
    uint32_t* done = nullptr;          // per-workgroup completion words (rt_trace_screen_dev)
    uint32_t seq = 0;
};

// The SGPR-capped fast kernel (rt_render_kernel_sg) for the depths whose fast kernels fit 7 waves by VGPRs (c2: 63,
// c3: 67).
#ifndef RT_SG_MAX_B
#define RT_SG_MAX_B 2
#endif
// The achromatic (one-channel, rt_device.hpp shade ACHRO) instances: the benchmark depths' fast and culling kernels.
#ifndef RT_ACHRO_MAX_B
#define RT_ACHRO_MAX_B 3
#endif
// The supersampled instances (SS = 1; one-wave tiles).  0: not built (experiment builds; rt_render_ss_dev then fails).
#ifndef RT_SS
#define RT_SS (RT_WG_FAST == 64)
#endif

// ---- Which instance of the render kernels a frame runs: the key, the selector (here), the list (below) ----

// An instance's key: the kernel template and exactly its template arguments after the depth B.  (The SGPR-capped
// template takes MINW, CULL, PACKED and ACHRO; its body fixes the other fields, RenderRow checks which values.)
enum RenderTemplate { kKernel = 0, kKernelSg = 1 };   // rt_render_kernel, rt_render_kernel_sg
struct RenderKey {
    int kernel;                                // RenderTemplate
    int LDS, MINW;
    bool TRANSP, CULL;
    int WG;
    bool TREE, PACKED, FIX64, ACHRO, SS;
};
constexpr bool operator==(const RenderKey& a, const RenderKey& b) {
    return a.kernel == b.kernel && a.LDS == b.LDS && a.MINW == b.MINW && a.TRANSP == b.TRANSP && a.CULL == b.CULL &&
           a.WG == b.WG && a.TREE == b.TREE && a.PACKED == b.PACKED && a.FIX64 == b.FIX64 && a.ACHRO == b.ACHRO &&
           a.SS == b.SS;
}

// What render_route() decides on: the scene kind (rt_ctx / DevScene) and the context's A/B knobs (RT_SCENE_IN_LDS,
// RT_WG_STAGING, RT_MIN_WAVES — >= 5 keeps the launch bounds of depth <= 3 —, RT_ACHRO_OFF), beside depth and mode.
struct RouteScene { bool tree, transparent; int n_padded, n_stride; bool achromatic; int lds_bytes; };
struct RouteKnobs { bool use_lds, wg_staging; int min_waves; bool achro_off; };
enum RenderMode { kModePlain = 0, kModePacked = 1, kModeSS = 2 };   // RGBA images; GRAY / RGB images; supersampled
struct RenderRoute {
    RenderKey key;
    int lds;                                   // dynamic LDS bytes of the launch
    int tile_w;                                // tile width in pixels: 32 for the 256-thread instances, else RT_WG_FAST / 8
};

// The instance a frame of scene s runs at `depth` in `mode` under the knobs k — or, level_mask, the launch that
// follows a fast scene's calibration render to write its level masks (a culling instance at the scene's own stride).
// Pure, and the one place this is decided (render_dev_impl, rt_diag_kernel_*, rt_diag_render_route); DESIGN.md §5g
// has the rules as a table, tests/test_route.py pins them.
inline RenderRoute render_route(const RouteScene& s, const RouteKnobs& k, int depth, int mode, bool level_mask) {
    const bool plain = mode == kModePlain, ss = mode == kModeSS;
    // bounded (MINW > 1): depth <= 3; plain frames and the level-mask launch only with RT_MIN_WAVES >= 5
    const bool bounded = depth <= 3 && (k.min_waves >= 5 || !(plain || level_mask));
    const bool achro = s.achromatic && !s.transparent && !s.tree && !k.achro_off && !ss &&
                       depth <= RT_ACHRO_MAX_B && bounded;
    const bool frame = !level_mask, knobs = plain && frame;   // (packed and supersampled frames take no A/B knob)
    RenderKey K{kKernel, 0, 1, false, false, 64, false, mode == kModePacked && frame, false, false, ss && frame};
    int lds = 0;
    if (s.tree && frame) {
        K.TRANSP = K.TREE = true;
    } else if (s.transparent && frame) {
        K.TRANSP = true;
        lds = slot_bytes(depth, true, 64);
    } else if (knobs && k.use_lds) {
        K.LDS = 1;
        K.WG = kThreads;
        lds = s.lds_bytes + slot_bytes(depth, false);
    } else if (knobs && k.wg_staging) {         // (the tile's four staged output images behind the slots)
        K.WG = kThreads;
        K.MINW = bounded ? fast_min_waves(depth) : 1;
        lds = 4096 + 6144 + 1024 + 1024 + slot_bytes(depth, false);
    } else {                                    // culling from kConeMin spheres (rt_device.hpp CULL), else fast
        K.CULL = level_mask || s.n_padded >= kConeMin;
        K.WG = RT_WG_FAST;
        K.MINW = !bounded ? 1 : K.CULL ? cull_min_waves(depth) : fast_min_waves(depth);
        K.FIX64 = K.CULL && s.n_stride == kCullStride;
        K.ACHRO = achro;
        if (!K.CULL && !ss && bounded && depth <= RT_SG_MAX_B && RT_FAST_SGPRS > 0) K.kernel = kKernelSg;   // the SGPR cap
        lds = slot_bytes(depth, false, RT_WG_FAST, K.CULL);
    }
    return RenderRoute{K, lds, K.WG == kThreads ? kTileW : RT_WG_FAST / 8};
}

struct RenderLaunch {
    RenderKey key;                             // the instance (render_route)
    dim3 grid;
    int32_t disp_w, disp_n;                    // the dispatch table's DispGeom: positions per grid row, positions in all
    size_t lds;
    hipStream_t stream;
    const DevScene* scene;
    RenderParams P;
    void* o32;
    void* o8;
    double* o64;
    uint32_t* orc;
};

// Defined once per depth B in rt_render_b<B>.hip.
template <int B>
hipError_t launch_render(const RenderLaunch& L);
template <int B>
hipError_t launch_trace_rays(int variant /* 0 opaque, 1 FULL, 2 tree */, dim3 grid, hipStream_t st,
                             const DevScene* s, const double* a, const double* b, int n, double* rgb, uint32_t* rc,
                             const ScreenArgs& sa);
template <int B>
const void* render_kernel_ptr(const RenderKey& k);   // the depth-B instance with key k, or nullptr: there is none

#define RT_DECLARE_DEPTH(B)                                                                                   \
    template <>                                                                                                \
    hipError_t launch_render<B>(const RenderLaunch& L);                                                        \
    template <>                                                                                                \
    hipError_t launch_trace_rays<B>(int, dim3, hipStream_t, const DevScene*, const double*, const double*, int,   \
                                    double*, uint32_t*, const ScreenArgs&);                                    \
    template <>                                                                                                \
    const void* render_kernel_ptr<B>(const RenderKey&);
RT_DECLARE_DEPTH(0) RT_DECLARE_DEPTH(1) RT_DECLARE_DEPTH(2) RT_DECLARE_DEPTH(3)
RT_DECLARE_DEPTH(4) RT_DECLARE_DEPTH(5) RT_DECLARE_DEPTH(6) RT_DECLARE_DEPTH(7)
#undef RT_DECLARE_DEPTH

// f(std::integral_constant<int, B>) for the bounce depth B = depth of a checked render (0 .. 7: rt_api.h RT_MAX_DEPTH),
// the one place a runtime depth becomes a template argument.
template <class F>
auto with_depth(int depth, F&& f) {
    switch (depth) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        default: return f(std::integral_constant<int, 7>{});
    }
}

// The `variant` of the generic-path launches (launch_trace_rays and rt_sampled.hpp's) for a scene kind.
inline int trace_variant(bool tree, bool transparent) { return tree ? 2 : transparent ? 1 : 0; }

// ---- The per-depth instance files' bodies ----

// The two kernel templates share one parameter list (RenderArgs), so one pointer type holds any instance.
using RenderKernelFn = void (*)(const DispRec*, int32_t, int32_t, const DevScene*, RenderParams, void*, void*, double*,
                                uint32_t*);

// One row of a depth's instance list: whether this build has the instance (ON) and its key.  The key's fields are the
// very template arguments kernel<B>() instantiates, so what is matched and what is launched cannot disagree.
template <bool ON, int KERNEL, int LDS, int MINW, bool TRANSP, bool CULL, int WG, bool TREE = false, bool PACKED = false,
          bool FIX64 = false, bool ACHRO = false, bool SS = false>
struct RenderRow {
    static constexpr bool on = ON;
    static constexpr RenderKey key{KERNEL, LDS, MINW, TRANSP, CULL, WG, TREE, PACKED, FIX64, ACHRO, SS};
    static_assert(KERNEL == kKernel || (LDS == 0 && !TRANSP && WG == RT_WG_FAST && !TREE && !FIX64 && !SS),
                  "the SGPR-capped kernel's body fixes these fields");
    template <int B>
    static RenderKernelFn kernel() {
        if constexpr (!ON) return nullptr;
        else if constexpr (KERNEL == kKernelSg) return rt_render_kernel_sg<B, MINW, CULL, PACKED, ACHRO>;
        else return rt_render_kernel<B, LDS, MINW, TRANSP, CULL, WG, TREE, PACKED, FIX64, ACHRO, SS>;
    }
};
template <class... Rows>
struct RenderRows {};

// The render-kernel instances of depth B: every kernel an instance file emits, one row each.  render_route() returns
// rows of this list only (tests/test_route.py walks its inputs).  Rows marked * are compiled but never chosen at some
// depths — the bounded rows beyond depth 3 (any-waves there) and the uncapped twin of an SGPR-capped row up to depth
// RT_SG_MAX_B: the instance files have always emitted them, and this list keeps the set of kernels as it was.
template <int B>
struct RenderInstances {
    static constexpr bool kAll = B <= RT_MAX_B;                               // (experiment builds stop earlier)
    static constexpr bool kSg = kAll && B <= RT_SG_MAX_B && RT_FAST_SGPRS > 0;
    static constexpr bool kAc = kAll && B <= RT_ACHRO_MAX_B;
    static constexpr bool kSs = kAll && RT_SS;
    static constexpr int F = RT_WG_FAST, T = kThreads;
    static constexpr int MW = fast_min_waves(B), MC = cull_min_waves(B);     // bounded: plain and achromatic rows
    static constexpr int PW = B <= 3 ? MW : 1, PC = B <= 3 ? MC : 1;          // packed and supersampled rows
    using rows = RenderRows<
        //        ON    template   LDS MINW TRANSP CULL WG TREE PACKED FIX64 ACHRO SS
        RenderRow<kSg,  kKernelSg,  0,  MW,  0,    0,   F>,                             // fast, bounded, SGPR cap
        RenderRow<kAll, kKernel,    0,  MW,  0,    0,   F>,                             // fast, bounded *
        RenderRow<kAll, kKernel,    0,  1,   0,    0,   F>,                             // fast, any waves
        RenderRow<kAll, kKernel,    0,  MC,  0,    1,   F,  0,   0,     1>,             // culling, bounded, stride 64 *
        RenderRow<kAll, kKernel,    0,  MC,  0,    1,   F>,                             // culling, bounded *
        RenderRow<kAll, kKernel,    0,  1,   0,    1,   F,  0,   0,     1>,             // culling, any waves, stride 64
        RenderRow<kAll, kKernel,    0,  1,   0,    1,   F>,                             // culling, any waves
        RenderRow<kAll, kKernel,    0,  1,   1,    0,   64>,                            // transparent
        RenderRow<kAll, kKernel,    0,  1,   1,    0,   64, 1>,                         // ray tree
        RenderRow<kAll, kKernel,    1,  1,   0,    0,   T>,                             // A/B: scene in LDS
        RenderRow<kAll, kKernel,    0,  MW,  0,    0,   T>,                             // A/B: staged stores, bounded *
        RenderRow<kAll, kKernel,    0,  1,   0,    0,   T>,                             // A/B: staged stores, any waves
        // achromatic (one channel)
        RenderRow<kSg && kAc, kKernelSg, 0,  MW,  0,    0,   F,  0,   0,     0,    1>,       // fast, SGPR cap
        RenderRow<kAc,  kKernel,    0,  MW,  0,    0,   F,  0,   0,     0,    1>,       // fast *
        RenderRow<kAc,  kKernel,    0,  MC,  0,    1,   F,  0,   0,     1,    1>,       // culling, stride 64
        RenderRow<kAc,  kKernel,    0,  MC,  0,    1,   F,  0,   0,     0,    1>,       // culling
        // packed pixel formats (runtime format branches at the stores)
        RenderRow<kSg,  kKernelSg,  0,  MW,  0,    0,   F,  0,   1>,                    // fast, SGPR cap
        RenderRow<kAll, kKernel,    0,  PW,  0,    0,   F,  0,   1>,                    // fast *
        RenderRow<kAll, kKernel,    0,  PC,  0,    1,   F,  0,   1,     1>,             // culling, stride 64
        RenderRow<kAll, kKernel,    0,  PC,  0,    1,   F,  0,   1>,                    // culling
        RenderRow<kAll, kKernel,    0,  1,   1,    0,   64, 0,   1>,                    // transparent
        RenderRow<kAll, kKernel,    0,  1,   1,    0,   64, 1,   1>,                    // ray tree
        RenderRow<kSg && kAc, kKernelSg, 0,  MW,  0,    0,   F,  0,   1,     0,    1>,       // achromatic fast, SGPR cap
        RenderRow<kAc,  kKernel,    0,  MW,  0,    0,   F,  0,   1,     0,    1>,       // achromatic fast *
        RenderRow<kAc,  kKernel,    0,  MC,  0,    1,   F,  0,   1,     1,    1>,       // achromatic culling, stride 64
        RenderRow<kAc,  kKernel,    0,  MC,  0,    1,   F,  0,   1,     0,    1>,       // achromatic culling
        // supersampled (three channels, RGBA stores, no SGPR cap)
        RenderRow<kSs,  kKernel,    0,  PW,  0,    0,   F,  0,   0,     0,    0,    1>, // fast
        RenderRow<kSs,  kKernel,    0,  PC,  0,    1,   F,  0,   0,     1,    0,    1>, // culling, stride 64
        RenderRow<kSs,  kKernel,    0,  PC,  0,    1,   F,  0,   0,     0,    0,    1>, // culling
        RenderRow<kSs,  kKernel,    0,  1,   1,    0,   64, 0,   0,     0,    0,    1>, // transparent
        RenderRow<kSs,  kKernel,    0,  1,   1,    0,   64, 1,   0,     0,    0,    1>  // ray tree
        >;
};

// The kernel of the row whose key equals k, or nullptr.
template <int B, class... Rows>
RenderKernelFn find_render_kernel(RenderRows<Rows...>, const RenderKey& k) {
    RenderKernelFn f = nullptr;
    (void)((Rows::on && Rows::key == k && ((f = Rows::template kernel<B>()), true)) || ...);
    return f;
}

template <int B>
const void* render_kernel_ptr_impl(const RenderKey& k) {
    return (const void*)find_render_kernel<B>(typename RenderInstances<B>::rows{}, k);
}

template <int B>
hipError_t launch_render_impl(const RenderLaunch& L) {
    const RenderKernelFn kern = find_render_kernel<B>(typename RenderInstances<B>::rows{}, L.key);
    if (!kern) return hipErrorInvalidValue;
    if (L.lds > 65536) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, L.grid, dim3(L.key.WG), L.lds, L.stream, L.P.disp, L.disp_w, L.disp_n,
                       L.scene, L.P, L.o32, L.o8, L.o64, L.orc);
    return hipGetLastError();
}

template <int B>
hipError_t launch_trace_rays_impl(int variant, dim3 grid, hipStream_t st, const DevScene* s, const double* a,
                                  const double* b, int n, double* rgb, uint32_t* rc, const ScreenArgs& sa) {
    if constexpr (B > RT_MAX_B) {
        return hipErrorInvalidValue;
    } else {
        const size_t lds = (size_t)sa.scene_lds;
        if (sa.pix) {                                   // screen chunks: kScreenBlock-thread workgroups
            constexpr int W = kScreenBlock;
            const dim3 g((unsigned)((n + W - 1) / W));
            if (variant == 2)
                hipLaunchKernelGGL((rt_trace_rays_kernel<B, true, true, W>), g, dim3(W), lds, st, s, a, b, n, rgb, rc,
                                   sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
            else if (variant == 1)
                hipLaunchKernelGGL((rt_trace_rays_kernel<B, true, false, W>), g, dim3(W), lds + slot_bytes(B, true, W),
                                   st, s, a, b, n, rgb, rc, sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
            else
                hipLaunchKernelGGL((rt_trace_rays_kernel<B, false, false, W>), g, dim3(W), lds + slot_bytes(B, false, W),
                                   st, s, a, b, n, rgb, rc, sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
            return hipGetLastError();
        }
        if (variant == 2)
            hipLaunchKernelGGL((rt_trace_rays_kernel<B, true, true>), grid, dim3(kThreads), lds, st, s, a, b, n, rgb, rc,
                               sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
        else if (variant == 1)
            hipLaunchKernelGGL((rt_trace_rays_kernel<B, true, false>), grid, dim3(kThreads), lds + slot_bytes(B, true),
                               st, s, a, b, n, rgb, rc, sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
        else
            hipLaunchKernelGGL((rt_trace_rays_kernel<B, false, false>), grid, dim3(kThreads), lds + slot_bytes(B, false),
                               st, s, a, b, n, rgb, rc, sa.pix, sa.m, sa.first, sa.jit, sa.scene_lds, sa.done, sa.seq);
        return hipGetLastError();
    }
}

}  // namespace rtk

// One line per instance file: the depth-B definitions of the three declarations above.
#define RT_RENDER_INSTANCES(B)                                                                                  \
    namespace rtk {                                                                                            \
    template <>                                                                                                \
    hipError_t launch_render<B>(const RenderLaunch& L) { return launch_render_impl<B>(L); }                    \
    template <>                                                                                                \
    hipError_t launch_trace_rays<B>(int v, dim3 g, hipStream_t st, const DevScene* s, const double* a,         \
                                    const double* b, int n, double* rgb, uint32_t* rc, const ScreenArgs& sa) { \
        return launch_trace_rays_impl<B>(v, g, st, s, a, b, n, rgb, rc, sa);                                   \
    }                                                                                                          \
    template <>                                                                                                \
    const void* render_kernel_ptr<B>(const RenderKey& k) { return render_kernel_ptr_impl<B>(k); }              \
    }
