// rt_sampled.hip — the device entry points of the sampled renders of rt_sampled.hpp: adaptive supersampling
// (base render, rt_classify_kernel, the refine launch), the lens family's one launch, the jittered render's, the
// shutter render's, the accumulating render's launches and the adaptive lens render's three passes.
#include <algorithm>
#include <cmath>
#include <string>

#include "rt_ctx.hpp"
#include "rt_sampled.hpp"

using namespace rt;

namespace {

using namespace rtk;

// Adaptive supersampling, pass 2 (rt_render_adaptive_dev): the criterion on the W x H base frame and the work list.
// Pixel k = j W + i is refined iff some in-frame 4-neighbour differs from it by more than T in some colour byte of
// the base RGBA8 image (T = -1: any in-frame neighbour).  Sets refined[k] (when given) and appends the flagged
// pixels to `list` behind *count (zeroed on the stream by the caller).  A workgroup of kClassifyThreads work-items
// takes kClassifyPer runs of kClassifyThreads consecutive pixels; every wave ballots each of its runs and counts the
// bits, the waves' counts meet in LDS, and ONE atomic add per workgroup reserves its stretch of the list: returning
// atomics on one word complete at about 88 per us on this chip, and one per wave of 64 pixels (7500 of them in a
// 1920 x 1080 c2 frame) made this pass 86 us long.  Each flagged lane stores at the workgroup's base + the flagged
// pixels of earlier waves and runs + the flagged lanes below it.  The list's order depends on the workgroups'
// arrival; no output does.
// SPREAD (rt_render_lens_adaptive_dev): base8 is the coarse lens frame, and a pixel is also refined when its samples'
// spread byte (rt_lens_coarse_kernel) is above T — for T = -1 every pixel, a lone one included.  spread is not read
// without the flag.
constexpr int kClassifyThreads = 1024, kClassifyPer = 8;
template <bool SPREAD>
__global__ __launch_bounds__(kClassifyThreads) void rt_classify_kernel(const uint32_t* __restrict__ base8,
                                                                       const uint8_t* __restrict__ spread, int W, int H,
                                                                       int T, uint8_t* __restrict__ refined,
                                                                       uint32_t* __restrict__ count,
                                                                       uint32_t* __restrict__ list) {
    __shared__ uint32_t wave_first[kClassifyThreads / 64];
    __shared__ uint32_t block_first;
    const size_t n = (size_t)W * (size_t)H;
    const size_t k0 = (size_t)blockIdx.x * (kClassifyThreads * kClassifyPer) + threadIdx.x;
    uint32_t flags = 0;                                     // bit r: this lane's pixel of run r is refined
    // The loads of all runs first, without branches (a neighbour outside the frame, and a pixel past the frame's end,
    // is replaced by an in-frame address and masked below): the 5 kClassifyPer loads of a lane are in flight together,
    // where one dependent round trip per run made the pass latency-bound.
    uint32_t px[kClassifyPer][5], edge[kClassifyPer], spr[kClassifyPer];
#pragma unroll
    for (int r = 0; r < kClassifyPer; ++r) {
        const size_t k = k0 + (size_t)r * kClassifyThreads, kc = k < n ? k : n - 1;   // (n <= 2^31: kc fits 32 bits)
        const uint32_t j = (uint32_t)kc / (uint32_t)W, i = (uint32_t)kc - j * (uint32_t)W;
        const uint32_t l = i > 0, rr = i + 1 < (uint32_t)W, d = j > 0, u = j + 1 < (uint32_t)H;
        edge[r] = k < n ? (l | (rr << 1) | (d << 2) | (u << 3)) : 0u;
        px[r][0] = base8[kc];
        px[r][1] = base8[kc - l];
        px[r][2] = base8[kc + rr];
        px[r][3] = base8[kc - (d ? (size_t)W : 0)];
        px[r][4] = base8[kc + (u ? (size_t)W : 0)];
        if constexpr (SPREAD) spr[r] = spread[kc];
    }
#pragma unroll
    for (int r = 0; r < kClassifyPer; ++r) {
        const size_t k = k0 + (size_t)r * kClassifyThreads;
        bool flag = false;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            int worst = -1;
            for (int c = 0; c < 24; c += 8) {
                const int df = (int)((px[r][0] >> c) & 0xffu) - (int)((px[r][nb + 1] >> c) & 0xffu);
                worst = max(worst, df < 0 ? -df : df);
            }
            flag |= ((edge[r] >> nb) & 1u) && worst > T;
        }
        if constexpr (SPREAD) flag |= k < n && (int)spr[r] > T;
        if (k < n && refined) refined[k] = flag ? 1 : 0;
        flags |= (flag ? 1u : 0u) << r;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t ballot[kClassifyPer];                          // every lane of the workgroup is here
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < kClassifyPer; ++r) {
        ballot[r] = __ballot((flags >> r) & 1u);
        mine += (uint32_t)__popcll(ballot[r]);
    }
    if (lane == 0) wave_first[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kClassifyThreads / 64; ++w) {
            const uint32_t c = wave_first[w];
            wave_first[w] = sum;
            sum += c;
        }
        block_first = sum ? atomicAdd(count, sum) : 0u;
    }
    __syncthreads();
    uint32_t at = block_first + wave_first[wave];
#pragma unroll
    for (int r = 0; r < kClassifyPer; ++r) {
        if ((flags >> r) & 1u)
            list[at + (uint32_t)__popcll(ballot[r] & ((1ull << lane) - 1ull))] = (uint32_t)(k0 + (size_t)r * kClassifyThreads);
        at += (uint32_t)__popcll(ballot[r]);
    }
}

}  // namespace

// ---- adaptive supersampling (include/rt_api.h, ABI 9) -------------------------------------------------------------
// Workgroups of the refine launch: a fixed grid of one-wave workgroups (the list's length is only known on the
// device) that covers the device's wave slots a few times over; the grid-stride loop takes the rest.
constexpr unsigned kRefineGrid = 8192;

// Three passes on `stream`: the one-sample base render (rt_render_ss_dev with S = 1: rt_render_dev's instances, or
// the two-word-counter ones when counters are asked for) straight into the caller's outputs, rt_classify_kernel on
// its RGBA8 bytes, rt_refine_kernel over the work list.  No shortcut for any threshold.
extern "C" int rt_render_adaptive_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                                      int threshold, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                      uint32_t* raycount2, uint8_t* refined, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    if (threshold < -1 || threshold > 255)
        return rt_fail(RT_EINVAL, "rt_render_adaptive_dev: threshold must lie in -1 .. 255");
    SampledLaunch L{};                                      // P: the sample grid's, the refine kernel's ray set-up
    int s, rc = sample_grid_front(c, cam, W, H, depth, samples, &s, &L.P);
    if (rc) return rc;
    const size_t npx = (size_t)W * (size_t)H;
    const AdaptiveLayout lay = rt_adaptive_layout(npx);
    if (!workspace || workspace_bytes < lay.bytes || (uintptr_t)workspace % 16 != 0)
        return rt_fail(RT_EINVAL, "rt_render_adaptive_dev: null, misaligned or too small workspace "
                                  "(rt_adaptive_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    uint32_t* count = reinterpret_cast<uint32_t*>(ws);
    uint32_t* list = reinterpret_cast<uint32_t*>(ws + lay.list);
    uint8_t* base8 = rgba8 ? rgba8 : ws + lay.base8;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
    rc = rt_render_ss_dev(c, cam, W, H, depth, 1, nullptr, rgba32f, base8, rgb64f, raycount2, st);
    if (rc) return rc;
    constexpr size_t kClassifyBlock = (size_t)kClassifyThreads * kClassifyPer;
    hipLaunchKernelGGL(rt_classify_kernel<false>, dim3((unsigned)((npx + kClassifyBlock - 1) / kClassifyBlock)),
                       dim3(kClassifyThreads), 0, st, reinterpret_cast<const uint32_t*>(base8),
                       (const uint8_t*)nullptr, W, H, threshold, refined, count, list);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_classify_kernel: ") + hipGetErrorString(e));
    // S = 1: a refined pixel's only sample is the base sample itself, already in place
    if (s == 0 || (!rgba32f && !rgba8 && !rgb64f && !raycount2)) return RT_OK;
    L.variant = trace_variant(c->scene.tree, c->scene.transparent);
    const size_t per_wave = (size_t)64 >> (2 * s);
    L.grid = (unsigned)std::min<size_t>((npx + per_wave - 1) / per_wave, kRefineGrid);
    L.stream = st;
    L.scene = c->scene.d_scene;
    L.out_w = W;
    L.count = count;
    L.list = list;
    L.o32 = rgba32f;
    L.o8 = rgba8;
    L.o64 = rgb64f;
    L.orc2 = raycount2;
    e = with_depth(depth, [&](auto B) { return launch_refine<decltype(B)::value>(L); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_refine_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

// ---- the lens family: depth of field, soft shadows, motion blur (include/rt_api.h, ABI 10) -------------------------
// rt_render_motion_dev with shutter 0 is rt_render_soft_dev, and that with light_size 0 is rt_render_dof_dev: one
// kernel (rt_lens_kernel<.., AREA, MOTION>, rt_sampled.hpp) in three kinds behind the three pairs of entry points.

// The arguments a kind reads, in the order aperture, light_size, shutter.
int lens_arg_checks(LensKind kind, const char* who, double aperture, double light_size, double shutter) {
    if (!(aperture >= 0.0) || !std::isfinite(aperture))
        return rt_fail(RT_EINVAL, std::string(who) + ": aperture must be finite and >= 0");
    if (kind >= kLensSoft && (!(light_size >= 0.0) || !std::isfinite(light_size)))
        return rt_fail(RT_EINVAL, std::string(who) + ": light_size must be finite and >= 0");
    if (kind >= kLensMotion && !(shutter >= 0.0 && shutter <= 1.0))
        return rt_fail(RT_EINVAL, std::string(who) + ": shutter must be in [0, 1]");
    return RT_OK;
}

// One launch of the kind's rt_lens_kernel on `stream`: S x S lens samples per pixel through the generic trace path;
// soft: sample (a, b) lit by point (a, b) of every light's square panel; motion: sample (a, b) also at its own shutter
// time.  The light shift and the displaced centres are formed in the kernel, from light_size and from the context's
// motion record: the scene record is read, never written or re-uploaded.  Nothing per view: no rt_prepare_kernel, no
// calibration, no dispatch table, and no field of the context is written, so the context's cone and level masks and
// its tile order stay what the last rt_render_dev left.  No shortcut for shutter 0, an unset motion, light_size 0,
// aperture 0 or samples 1.  `who` is the entry point, the prefix of its messages.
int lens_render_dev(LensKind kind, const char* who, rt_ctx* c, const rt_camera* cam, int W, int H, int depth,
                    int samples, double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                    double* rgb64f, uint32_t* raycount2, void* stream) {
    int s, rc = lens_arg_checks(kind, who, aperture, light_size, shutter);
    if (rc) return rc;
    SampledLaunch L{};                                      // P: the sample grid's, the kernel's ray set-up
    rc = sample_grid_front(c, cam, W, H, depth, samples, &s, &L.P);
    if (rc) return rc;
    if (kind == kLensMotion && !c->scene.d_motion) return rt_fail(RT_EINVAL, std::string(who) + ": no scene set");
    L.variant = trace_variant(c->scene.tree, c->scene.transparent);
    L.stream = (hipStream_t)stream;
    L.scene = c->scene.d_scene;
    L.aperture = aperture;
    L.light_size = light_size;                              // 0 from the kinds without it
    L.shutter = shutter;
    if (kind == kLensMotion) L.motion = c->scene.d_motion;
    L.o32 = rgba32f;
    L.o8 = rgba8;
    L.o64 = rgb64f;
    L.orc2 = raycount2;
    if (!rgba32f && !rgba8 && !rgb64f && !raycount2) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    const hipError_t e = with_depth(depth, [&](auto B) {
        constexpr int b = decltype(B)::value;
        return kind == kLensMotion ? launch_lens<b, true, true>(L)
               : kind == kLensSoft ? launch_lens<b, true, false>(L)
                                   : launch_lens<b, false, false>(L);
    });
    // the names the kinds' kernels had as kernels of their own: the messages keep them
    static const char* const kKernel[] = {"rt_dof_kernel: ", "rt_soft_kernel: ", "rt_motion_kernel: "};
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string(kKernel[kind]) + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_render_dof_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                                 double aperture, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                 uint32_t* raycount2, void* stream) {
    return lens_render_dev(kLensDof, "rt_render_dof_dev", c, cam, W, H, depth, samples, aperture, 0.0, 0.0, rgba32f,
                           rgba8, rgb64f, raycount2, stream);
}

extern "C" int rt_render_soft_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                                  double aperture, double light_size, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                  uint32_t* raycount2, void* stream) {
    return lens_render_dev(kLensSoft, "rt_render_soft_dev", c, cam, W, H, depth, samples, aperture, light_size, 0.0,
                           rgba32f, rgba8, rgb64f, raycount2, stream);
}

extern "C" int rt_render_motion_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                                    double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                                    double* rgb64f, uint32_t* raycount2, void* stream) {
    return lens_render_dev(kLensMotion, "rt_render_motion_dev", c, cam, W, H, depth, samples, aperture, light_size,
                           shutter, rgba32f, rgba8, rgb64f, raycount2, stream);
}

// ---- the jittered render (include/rt_api.h) -------------------------------------------------------------------------
int jitter_arg_checks(const char* who, int jitter) {
    if (rtj::jitter_log2_of(jitter) < 0) return rt_fail(RT_EINVAL, std::string(who) + ": jitter must be 1, 2, 4, 8 or 16");
    return RT_OK;
}

// The jittered render's checks and its launch record: lens_render_dev's motion kind with the fine camera (pitch / (S J),
// S J bottom, whose whole S J width x S J height frame must index in int32) and the seed beside it.
static int jitter_launch(const char* who, rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                         int jitter, uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f,
                         uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream, SampledLaunch* out) {
    int s, rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter);
    if (rc || (rc = jitter_arg_checks(who, jitter))) return rc;
    SampledLaunch& L = *out;                                // P: the sample grid's, the kernel's ray set-up
    rc = sample_grid_front(c, cam, W, H, depth, samples, &s, &L.P);
    if (rc) return rc;
    if (!c->scene.d_motion) return rt_fail(RT_EINVAL, std::string(who) + ": no scene set");
    const long long sj = (long long)samples * jitter;
    const long long bx = sj * cam->bottom_x, by = sj * cam->bottom_y, fw = sj * W, fh = sj * H;
    if (fw > INT32_MAX || fh > INT32_MAX || bx < INT32_MIN || by < INT32_MIN || bx + fw - 1 > INT32_MAX ||
        by + fh - 1 > INT32_MAX)
        return rt_fail(RT_EINVAL, std::string(who) + ": samples * jitter * (bottom_x / bottom_y, width / height) "
                                                     "overflows int32");
    L.jitter.pitch_f = cam->pitch / (double)sj;             // exact: a power of two
    L.jitter.bottom_fx = (int32_t)bx;
    L.jitter.bottom_fy = (int32_t)by;
    L.jitter.jl = rtj::jitter_log2_of(jitter);
    L.jitter.seed = seed;
    L.variant = trace_variant(c->scene.tree, c->scene.transparent);
    L.stream = (hipStream_t)stream;
    L.scene = c->scene.d_scene;
    L.motion = c->scene.d_motion;
    L.aperture = aperture;
    L.light_size = light_size;
    L.shutter = shutter;
    L.o32 = rgba32f;
    L.o8 = rgba8;
    L.o64 = rgb64f;
    L.orc2 = raycount2;
    return RT_OK;
}

// One launch of rt_jitter_kernel on `stream`.  Nothing per view, no field of the context written, no shortcut for
// jitter 1 or any argument of 0.
int jitter_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples, int jitter,
                      uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                      double* rgb64f, uint32_t* raycount2, void* stream) {
    SampledLaunch L{};
    const int rc = jitter_launch(who, c, cam, W, H, depth, samples, jitter, seed, aperture, light_size, shutter, rgba32f,
                                 rgba8, rgb64f, raycount2, stream, &L);
    if (rc) return rc;
    if (!rgba32f && !rgba8 && !rgb64f && !raycount2) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    const hipError_t e = with_depth(depth, [&](auto B) { return launch_jitter<decltype(B)::value>(L); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_jitter_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_render_jitter_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples, int jitter,
                                    uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f,
                                    uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream) {
    return jitter_render_dev("rt_render_jitter_dev", c, cam, W, H, depth, samples, jitter, seed, aperture, light_size,
                             shutter, rgba32f, rgba8, rgb64f, raycount2, stream);
}

// ---- the shutter render: a moving camera (include/rt_api.h) ----------------------------------------------------------
// One launch of rt_shutter_kernel on `stream`: the jittered render's checks and launch record, then the camera motion's
// own checks: finite half-extents, and a finite basis at the two ends and the middle of the exposure (a view direction
// parallel to up there is rejected; in between it is the caller's).  The six half-extents and the camera's up travel in
// the kernel arguments; motion = nullptr is the zero motion.  Nothing per view, no field of the context written, no
// shortcut for a zero motion, shutter 0, jitter 1 or any argument of 0.
// The shutter render's checks and its launch record: jitter_launch, then the camera motion's own checks and fields.
static int shutter_launch(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                          int depth, int samples, int jitter, uint32_t seed, double aperture, double light_size,
                          double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                          void* stream, SampledLaunch* out) {
    SampledLaunch& L = *out;
    const int rc = jitter_launch(who, c, cam, W, H, depth, samples, jitter, seed, aperture, light_size, shutter, rgba32f,
                                 rgba8, rgb64f, raycount2, stream, &L);
    if (rc) return rc;
    const rt_camera_motion none{};
    const rt_camera_motion& m = motion ? *motion : none;
    for (int q = 0; q < 3; ++q)
        if (!std::isfinite(m.eye[q]) || !std::isfinite(m.look_at[q]))
            return rt_fail(RT_EINVAL, std::string(who) + ": non-finite displacement (motion)");
    for (const double sigma : {-shutter, 0.0, shutter}) {
        rt_camera at;
        double right[3], upp[3];
        if (rt_camera_at(cam, &m, sigma, &at)) return RT_EINVAL;
        rt_camera_basis(&at, right, upp);
        for (int q = 0; q < 3; ++q)
            if (!std::isfinite(right[q]) || !std::isfinite(upp[q]))
                return rt_fail(RT_EINVAL, std::string(who) + ": the camera's view direction is parallel to up within "
                                                             "the exposure (cam, motion)");
    }
    for (int q = 0; q < 3; ++q) {
        L.camera.up[q] = cam->up[q];
        L.camera.eye_move[q] = m.eye[q];
        L.camera.look_move[q] = m.look_at[q];
    }
    return RT_OK;
}

int shutter_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                       int depth, int samples, int jitter, uint32_t seed, double aperture, double light_size,
                       double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                       void* stream) {
    SampledLaunch L{};
    const int rc = shutter_launch(who, c, cam, motion, W, H, depth, samples, jitter, seed, aperture, light_size, shutter,
                                  rgba32f, rgba8, rgb64f, raycount2, stream, &L);
    if (rc) return rc;
    if (!rgba32f && !rgba8 && !rgb64f && !raycount2) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    const hipError_t e = with_depth(depth, [&](auto B) { return launch_shutter<decltype(B)::value>(L); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_shutter_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_render_shutter_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                     int depth, int samples, int jitter, uint32_t seed, double aperture,
                                     double light_size, double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                     uint32_t* raycount2, void* stream) {
    return shutter_render_dev("rt_render_shutter_dev", c, cam, motion, W, H, depth, samples, jitter, seed, aperture,
                              light_size, shutter, rgba32f, rgba8, rgb64f, raycount2, stream);
}

// ---- windows of the accumulating and converging renders (include/rt_api.h) -------------------------------------------
// The checks on a window of the W x H frame (W, H are checked by the render's own front).
int window_arg_checks(const char* who, const rt_window* win, int W, int H) {
    if (!win) return rt_fail(RT_EINVAL, std::string(who) + ": null window");
    if (win->x0 < 0 || win->y0 < 0) return rt_fail(RT_EINVAL, std::string(who) + ": negative window origin (window)");
    if (win->width < 1 || win->height < 1)
        return rt_fail(RT_EINVAL, std::string(who) + ": window width and height must be at least 1 (window)");
    if ((long long)win->x0 + win->width > W || (long long)win->y0 + win->height > H)
        return rt_fail(RT_EINVAL, std::string(who) + ": the window leaves the frame (window)");
    if (win->stride < win->width)
        return rt_fail(RT_EINVAL, std::string(who) + ": the window's stride is below its width (window)");
    return RT_OK;
}

// What the windowed kernels take (rt_sampled.hpp WindowParams): the window's corners in sample units and every buffer
// pointer of the launch record moved back by y0 * stride + x0 of its own elements, to where frame pixel (0, 0) would lie.
// The moved pointers are only ever indexed with the elements of the window's pixels (integer arithmetic: no pointer
// outside its buffer is formed in C++).
static void window_fold(const rt_window& w, int samples, SampledLaunch* L) {
    L->window = WindowParams{samples * w.x0, samples * w.y0, samples * (w.x0 + w.width), samples * (w.y0 + w.height),
                             w.stride};
    const uintptr_t off = (uintptr_t)w.y0 * (uintptr_t)w.stride + (uintptr_t)w.x0;
    const auto back = [&](auto* p, size_t bytes) {
        return p ? reinterpret_cast<decltype(p)>((uintptr_t)p - off * bytes) : p;
    };
    L->accum = back(L->accum, 24);
    L->accum2 = back(L->accum2, 24);
    L->npasses = back(L->npasses, 4);
    L->o32 = back(L->o32, 16);
    L->o8 = back(L->o8, 4);
    L->o64 = back(L->o64, 24);
    L->orc2 = back(L->orc2, 8);
}

// The context's list of windows as the list kernels take it (rt_sampled.hpp WindowListParams), after the checks of the
// list renders: a list must be set and must be of the W x H frame.
static int window_list_params(const char* who, const rt_ctx* c, int W, int H, int s, WindowListParams* out) {
    if (!c->windows.set) return rt_fail(RT_EINVAL, std::string(who) + ": no list of windows set (window)");
    if (W != c->windows.width || H != c->windows.height)
        return rt_fail(RT_EINVAL, std::string(who) + ": width, height are not the frame of the list of windows (window)");
    const int n = (int)c->windows.list.size();
    out->prefix = reinterpret_cast<const uint32_t*>(c->windows.d_table) + (size_t)s * (size_t)(n + 1);
    out->entries = reinterpret_cast<const rt::DevWindow*>(c->windows.d_table + rt::window_entries_at(n));
    out->n = (uint32_t)n;
    out->tiles = c->windows.tiles[s];
    // the grid's row length: the knob's, raised where the list's tiles would otherwise need more than 65535 rows
    out->grid_x = std::max((uint32_t)c->knobs.window_grid_x, (out->tiles + 65534u) / 65535u);
    return RT_OK;
}

// ---- progressive accumulation (include/rt_api.h) -----------------------------------------------------------------------
// Passes first_pass .. first_pass + passes - 1 of the shutter render (seed + p each) added to `accum` in the contract's
// order by rt_accum_kernel: the shutter render's checks and launch record, the call's own checks, then launches of at most
// L = Knobs::accum_max_passes passes each on `stream`.  A launch reads `accum` unless it begins at pass 0 and writes it, so
// the sum a later launch continues is the one the launch before it stored: one addition per pass from the loaded value
// either way, and the split is invisible in the bytes.  Every launch adds its passes' counters to raycount2 (the call's
// first launch starts them at zero); only the last one gets the image pointers, so the mean is formed once, from the
// whole sum.  Nothing per view, no field of the context written, no allocation, no shortcut for any argument; with no
// output at all the sum is still advanced.
int accum_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                     int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes, double aperture,
                     double light_size, double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                     uint32_t* raycount2, void* stream, const rt_window* win, bool list) {
    SampledLaunch L{};
    int rc = shutter_launch(who, c, cam, motion, W, H, depth, samples, jitter, seed, aperture, light_size, shutter,
                            rgba32f, rgba8, rgb64f, raycount2, stream, &L);
    if (rc || (win && (rc = window_arg_checks(who, win, W, H)))) return rc;
    if (list && (rc = window_list_params(who, c, W, H, L.P.ss_log2, &L.windows))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (passes < 1 || passes > kAccumCallPasses)
        return rt_fail(RT_EINVAL, std::string(who) + ": passes must lie in 1 .. 65536");
    if ((uint64_t)first_pass + (uint64_t)passes > (1ull << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": first_pass + passes must not exceed 2^31");
    RT_HIP(hipSetDevice(c->device));
    L.accum = accum;
    L.call_first = first_pass;
    if (win) {
        window_fold(*win, samples, &L);
        rgba32f = (float*)L.o32;
        rgba8 = (uint8_t*)L.o8;
        rgb64f = L.o64;
    }
    const uint32_t end = first_pass + (uint32_t)passes, step = (uint32_t)c->knobs.accum_max_passes;
    for (uint32_t p = first_pass; p < end; p += step) {
        L.first_pass = p;
        L.passes = std::min(step, end - p);
        const bool last = p + L.passes == end;
        L.o32 = last ? rgba32f : nullptr;
        L.o8 = last ? rgba8 : nullptr;
        L.o64 = last ? rgb64f : nullptr;
        const hipError_t e = with_depth(depth, [&](auto B) {
            return list  ? launch_accum_windows<decltype(B)::value>(L)
                   : win ? launch_accum_window<decltype(B)::value>(L)
                         : launch_accum<decltype(B)::value>(L);
        });
        if (e != hipSuccess)
            return rt_fail(RT_EHIP, std::string(list  ? "rt_accum_windows_kernel: "
                                                : win ? "rt_accum_window_kernel: "
                                                      : "rt_accum_kernel: ") + hipGetErrorString(e));
    }
    return RT_OK;
}

extern "C" int rt_render_accum_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                   int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes,
                                   double aperture, double light_size, double shutter, double* accum, float* rgba32f,
                                   uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream) {
    return accum_render_dev("rt_render_accum_dev", c, cam, motion, W, H, depth, samples, jitter, seed, first_pass, passes,
                            aperture, light_size, shutter, accum, rgba32f, rgba8, rgb64f, raycount2, stream);
}

// ---- converging accumulation (include/rt_api.h) ------------------------------------------------------------------------
// Up to `passes` passes per pixel, each pixel on the pass number of its own `count`, by rt_converge_kernel: the shutter
// render's checks and launch record, the call's own checks, the reset of `active` (a memset on `stream`: a node of the
// call under capture), then launches of at most L = Knobs::accum_max_passes passes each.  A launch loads the state and
// stores it, so a later launch continues every pixel where the launch before it left it, stopped pixels included (the
// rule is evaluated before every pass from the state alone): the split is invisible in the bytes.  Every launch adds its
// passes' counters to raycount2 (the call's first launch starts them at zero); only the last one gets the image
// pointers and `active`.  Nothing per view, no field of the context written, no allocation, no shortcut for any
// argument; with no output at all the state is still advanced.
int converge_arg_checks(const char* who, int passes, uint32_t min_passes, double tolerance) {
    if (passes < 1 || passes > kAccumCallPasses)
        return rt_fail(RT_EINVAL, std::string(who) + ": passes must lie in 1 .. 65536");
    if (min_passes < 2 || min_passes > (1u << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": min_passes must lie in 2 .. 2^31");
    if (!(tolerance >= 0.0) || !std::isfinite(tolerance))
        return rt_fail(RT_EINVAL, std::string(who) + ": tolerance must be finite and not negative");
    return RT_OK;
}

int converge_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                        int depth, int samples, int jitter, uint32_t seed, int passes, uint32_t min_passes,
                        double tolerance, double aperture, double light_size, double shutter, double* accum,
                        double* accum2, uint32_t* count, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                        uint32_t* raycount2, uint32_t* active, void* stream, const rt_window* win, bool list) {
    SampledLaunch L{};
    int rc = shutter_launch(who, c, cam, motion, W, H, depth, samples, jitter, seed, aperture, light_size, shutter,
                            rgba32f, rgba8, rgb64f, raycount2, stream, &L);
    if (rc || (win && (rc = window_arg_checks(who, win, W, H)))) return rc;
    if (list && (rc = window_list_params(who, c, W, H, L.P.ss_log2, &L.windows))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (!accum2) return rt_fail(RT_EINVAL, std::string(who) + ": null accum2");
    if (!count) return rt_fail(RT_EINVAL, std::string(who) + ": null count");
    if ((rc = converge_arg_checks(who, passes, min_passes, tolerance))) return rc;
    RT_HIP(hipSetDevice(c->device));
    if (active) RT_HIP(hipMemsetAsync(active, 0, sizeof(uint32_t), L.stream));
    L.accum = accum;
    L.accum2 = accum2;
    L.npasses = count;
    L.min_passes = min_passes;
    L.tolerance = tolerance;
    if (win) {
        window_fold(*win, samples, &L);
        rgba32f = (float*)L.o32;
        rgba8 = (uint8_t*)L.o8;
        rgb64f = L.o64;
    }
    const uint32_t end = (uint32_t)passes, step = (uint32_t)c->knobs.accum_max_passes;
    for (uint32_t p = 0; p < end; p += step) {
        L.passes = std::min(step, end - p);
        L.later = p > 0;
        L.last = p + L.passes == end;
        L.o32 = L.last ? rgba32f : nullptr;
        L.o8 = L.last ? rgba8 : nullptr;
        L.o64 = L.last ? rgb64f : nullptr;
        L.active = L.last ? active : nullptr;
        const hipError_t e = with_depth(depth, [&](auto B) {
            return list  ? launch_converge_windows<decltype(B)::value>(L)
                   : win ? launch_converge_window<decltype(B)::value>(L)
                         : launch_converge<decltype(B)::value>(L);
        });
        if (e != hipSuccess)
            return rt_fail(RT_EHIP, std::string(list  ? "rt_converge_windows_kernel: "
                                                : win ? "rt_converge_window_kernel: "
                                                      : "rt_converge_kernel: ") + hipGetErrorString(e));
    }
    return RT_OK;
}

extern "C" int rt_render_converge_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                      int depth, int samples, int jitter, uint32_t seed, int passes,
                                      uint32_t min_passes, double tolerance, double aperture, double light_size,
                                      double shutter, double* accum, double* accum2, uint32_t* count, float* rgba32f,
                                      uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, uint32_t* active,
                                      void* stream) {
    return converge_render_dev("rt_render_converge_dev", c, cam, motion, W, H, depth, samples, jitter, seed, passes,
                               min_passes, tolerance, aperture, light_size, shutter, accum, accum2, count, rgba32f, rgba8,
                               rgb64f, raycount2, active, stream);
}

// The windowed entry points: the same host code with the window's checks, folding and kernels.
extern "C" int rt_render_accum_window_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                          const rt_window* win, int depth, int samples, int jitter, uint32_t seed,
                                          uint32_t first_pass, int passes, double aperture, double light_size,
                                          double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                          uint32_t* raycount2, void* stream) {
    const char* who = "rt_render_accum_window_dev";
    if (const int rc = window_arg_checks(who, win, W, H)) return rc;    // first: no context is needed to reject a window
    return accum_render_dev(who, c, cam, motion, W, H, depth, samples, jitter, seed, first_pass, passes, aperture,
                            light_size, shutter, accum, rgba32f, rgba8, rgb64f, raycount2, stream, win);
}

extern "C" int rt_render_converge_window_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W,
                                             int H, const rt_window* win, int depth, int samples, int jitter,
                                             uint32_t seed, int passes, uint32_t min_passes, double tolerance,
                                             double aperture, double light_size, double shutter, double* accum,
                                             double* accum2, uint32_t* count, float* rgba32f, uint8_t* rgba8,
                                             double* rgb64f, uint32_t* raycount2, uint32_t* active, void* stream) {
    const char* who = "rt_render_converge_window_dev";
    if (const int rc = window_arg_checks(who, win, W, H)) return rc;    // first: no context is needed to reject a window
    return converge_render_dev(who, c, cam, motion, W, H, depth, samples, jitter, seed, passes, min_passes, tolerance,
                               aperture, light_size, shutter, accum, accum2, count, rgba32f, rgba8, rgb64f, raycount2,
                               active, stream, win);
}

// The list entry points: the same host code with the context's list of windows and the list kernels.
extern "C" int rt_render_accum_windows_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                           int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass,
                                           int passes, double aperture, double light_size, double shutter,
                                           double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                           uint32_t* raycount2, void* stream) {
    return accum_render_dev("rt_render_accum_windows_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                            first_pass, passes, aperture, light_size, shutter, accum, rgba32f, rgba8, rgb64f, raycount2,
                            stream, nullptr, true);
}

extern "C" int rt_render_converge_windows_dev(rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W,
                                              int H, int depth, int samples, int jitter, uint32_t seed, int passes,
                                              uint32_t min_passes, double tolerance, double aperture, double light_size,
                                              double shutter, double* accum, double* accum2, uint32_t* count,
                                              float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                                              uint32_t* active, void* stream) {
    return converge_render_dev("rt_render_converge_windows_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                               passes, min_passes, tolerance, aperture, light_size, shutter, accum, accum2, count,
                               rgba32f, rgba8, rgb64f, raycount2, active, stream, nullptr, true);
}

// ---- the adaptive lens render (include/rt_api.h) --------------------------------------------------------------------
// Three passes on `stream`, all of the motion kind: rt_lens_coarse_kernel on the samples_lo grid straight into the
// caller's outputs (the RGBA8 image into the workspace when the caller has none) with each pixel's spread byte,
// rt_classify_kernel<true> on those bytes, rt_lens_refine_kernel on the samples_hi grid over the work list.  No
// shortcut for any threshold, for equal sample counts or for an argument of 0; nothing per view, no field of the
// context written (lens_render_dev).
extern "C" int rt_render_lens_adaptive_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples_lo,
                                           int samples_hi, int threshold, double aperture, double light_size,
                                           double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                           uint32_t* raycount2, uint8_t* refined, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    const char* who = "rt_render_lens_adaptive_dev";
    if (ss_log2_of(samples_lo) < 0) return rt_fail(RT_EINVAL, std::string(who) + ": samples_lo must be 1, 2, 4 or 8");
    if (ss_log2_of(samples_hi) < 0) return rt_fail(RT_EINVAL, std::string(who) + ": samples_hi must be 1, 2, 4 or 8");
    if (samples_lo > samples_hi) return rt_fail(RT_EINVAL, std::string(who) + ": samples_lo must not exceed samples_hi");
    if (threshold < -1 || threshold > 255)
        return rt_fail(RT_EINVAL, std::string(who) + ": threshold must lie in -1 .. 255");
    int s_lo, s_hi, rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter);
    if (rc) return rc;
    SampledLaunch lo{}, hi{};                               // P: each sample grid's ray set-up
    if ((rc = sample_grid_front(c, cam, W, H, depth, samples_lo, &s_lo, &lo.P))) return rc;
    if ((rc = sample_grid_front(c, cam, W, H, depth, samples_hi, &s_hi, &hi.P))) return rc;
    if (!c->scene.d_motion) return rt_fail(RT_EINVAL, std::string(who) + ": no scene set");
    const size_t npx = (size_t)W * (size_t)H;
    const LensAdaptiveLayout lay = rt_lens_adaptive_layout(npx);
    if (!workspace || workspace_bytes < lay.bytes || (uintptr_t)workspace % 16 != 0)
        return rt_fail(RT_EINVAL, std::string(who) + ": null, misaligned or too small workspace "
                                                     "(rt_lens_adaptive_workspace_bytes)");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* ws = reinterpret_cast<uint8_t*>(workspace);
    uint32_t* count = reinterpret_cast<uint32_t*>(ws);
    uint32_t* list = reinterpret_cast<uint32_t*>(ws + lay.list);
    uint8_t* base8 = rgba8 ? rgba8 : ws + lay.base8;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipMemsetAsync(count, 0, sizeof(uint32_t), st));
    lo.variant = hi.variant = trace_variant(c->scene.tree, c->scene.transparent);
    lo.stream = hi.stream = st;
    lo.scene = hi.scene = c->scene.d_scene;
    lo.motion = hi.motion = c->scene.d_motion;
    lo.aperture = hi.aperture = aperture;
    lo.light_size = hi.light_size = light_size;
    lo.shutter = hi.shutter = shutter;
    lo.o32 = hi.o32 = rgba32f;
    lo.o8 = base8;
    hi.o8 = rgba8;
    lo.o64 = hi.o64 = rgb64f;
    lo.orc2 = hi.orc2 = raycount2;
    lo.spread = ws + lay.spread;
    hipError_t e = with_depth(depth, [&](auto B) { return launch_lens_coarse<decltype(B)::value>(lo); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_lens_coarse_kernel: ") + hipGetErrorString(e));
    constexpr size_t kClassifyBlock = (size_t)kClassifyThreads * kClassifyPer;
    hipLaunchKernelGGL(rt_classify_kernel<true>, dim3((unsigned)((npx + kClassifyBlock - 1) / kClassifyBlock)),
                       dim3(kClassifyThreads), 0, st, reinterpret_cast<const uint32_t*>(base8),
                       (const uint8_t*)lo.spread, W, H, threshold, refined, count, list);
    e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_classify_kernel: ") + hipGetErrorString(e));
    const size_t per_wave = (size_t)64 >> (2 * s_hi);
    hi.grid = (unsigned)std::min<size_t>((npx + per_wave - 1) / per_wave, kRefineGrid);
    hi.out_w = W;
    hi.count = count;
    hi.list = list;
    e = with_depth(depth, [&](auto B) { return launch_lens_refine<decltype(B)::value>(hi); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_lens_refine_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}
