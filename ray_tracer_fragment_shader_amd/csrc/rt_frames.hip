// rt_frames.hip — the calls that render into host memory (include/rt_api.h): rt_render and its sampled siblings
// through the context's grow-only device buffers, and the packed and asynchronous frames with their copy paths
// (copy kernel, hipMemcpyAsync, SDMA engine).  The renders themselves are the _dev calls of the other units.
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>

#include "../../include/rt_diag.h"
#include "rt_ctx.hpp"

using namespace rt;

namespace {

using namespace rtk;

// Device -> pinned host frame (rt_host_alloc memory, mapped into the device's address space): a copy kernel
// whose 16-byte stores cross PCIe straight into the host buffer.  On the render stream it needs no cross-stream
// hand-off; on the copy stream it overlaps the next frame's render (the table at copy_to_host has the measurements).
__global__ __launch_bounds__(kThreads) void rt_copy_out_kernel(const uint8_t* __restrict__ src,
                                                               uint8_t* __restrict__ dst, size_t n) {
    const size_t n16 = n >> 4;
    const size_t step = (size_t)gridDim.x * kThreads;
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n16; k += step) d[k] = s[k];
    if (blockIdx.x == 0 && threadIdx.x < (n & 15)) dst[(n16 << 4) + threadIdx.x] = src[(n16 << 4) + threadIdx.x];
}

// rt_render's ray statistics: sums of the per-pixel counters (primary+reflect segments, shadow rays) into
// sums[0], sums[1] (zeroed by the caller), so only 16 bytes cross PCIe instead of 4 bytes per pixel.
__global__ __launch_bounds__(kThreads) void rt_raysum_kernel(const uint32_t* __restrict__ rc, size_t n,
                                                             unsigned long long* __restrict__ sums) {
    unsigned long long seg = 0, sh = 0;
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kThreads) {
        const uint32_t v = rc[k];
        seg += v & 0xffffu;
        sh += v >> 16;
    }
    for (int o = 32; o > 0; o >>= 1) {
        seg += __shfl_down(seg, o);
        sh += __shfl_down(sh, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(sums, seg);
        atomicAdd(sums + 1, sh);
    }
}

// ... of a supersampled render's two-word counters (rt_render_ss_dev: rc2[2 k] segments, rc2[2 k + 1] shadow rays).
__global__ __launch_bounds__(kThreads) void rt_raysum2_kernel(const uint32_t* __restrict__ rc2, size_t n,
                                                              unsigned long long* __restrict__ sums) {
    unsigned long long seg = 0, sh = 0;
    const uint2* v2 = reinterpret_cast<const uint2*>(rc2);
    for (size_t k = (size_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (size_t)gridDim.x * kThreads) {
        const uint2 v = v2[k];
        seg += v.x;
        sh += v.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        seg += __shfl_down(seg, o);
        sh += __shfl_down(sh, o);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(sums, seg);
        atomicAdd(sums + 1, sh);
    }
}

}  // namespace

// Grow-only device buffer k of the context (rt_render's outputs).
static int ctx_buffer(rt_ctx* c, int k, size_t bytes, void** out) {
    if (bytes > c->frames.out_cap[k]) {
        // the buffer may still be read by a copy (or written by a render) queued on the context's streams
        RT_HIP(hipStreamSynchronize(c->frames.rs));
        RT_HIP(hipStreamSynchronize(c->frames.cs));
        if (c->frames.d_out[k]) (void)hipFree(c->frames.d_out[k]);
        c->frames.d_out[k] = nullptr;
        c->frames.out_cap[k] = 0;
        if (hipMalloc(&c->frames.d_out[k], bytes) != hipSuccess)
            return rt_fail(RT_ENOMEM, "rt_render: hipMalloc of output buffers failed");
        c->frames.out_cap[k] = bytes;
    }
    *out = c->frames.d_out[k];
    return RT_OK;
}

// Ray statistics of a render with per-pixel counters d_rc (npx pixels) into *stats (the stream must be done).
static int read_stats(rt_ctx* c, size_t npx, const unsigned long long* d_sums, rt_stats* stats) {
    unsigned long long sums[2] = {0, 0};
    if (npx) RT_HIP(hipMemcpy(sums, d_sums, sizeof(sums), hipMemcpyDeviceToHost));
    stats->primary_rays = npx;
    stats->reflect_rays = sums[0] - npx;
    stats->shadow_rays = sums[1];
    float ms = 0.f;
    if (npx) RT_HIP(hipEventElapsedTime(&ms, c->frames.ev0, c->frames.ev1));
    stats->kernel_ms = ms;
    return RT_OK;
}

// rt_host_alloc's pinned allocations (host base -> size, device mapping): host frames that land in one are
// copied by rt_copy_out_kernel, everything else by hipMemcpyAsync (pageable memory is staged by HIP).
static std::mutex g_pinned_mu;
static std::map<uintptr_t, std::pair<size_t, uintptr_t>> g_pinned;

static void* pinned_device_ptr(const void* host, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    const uintptr_t h = (uintptr_t)host;
    auto it = g_pinned.upper_bound(h);
    if (it == g_pinned.begin()) return nullptr;
    --it;
    if (h + bytes > it->first + it->second.first) return nullptr;
    return (void*)(it->second.second + (h - it->first));
}

// The device address of any page-locked host buffer (rt_host_alloc's, or one the caller pinned elsewhere, e.g. a
// torch pin_memory() tensor): the runtime's pointer attributes; nullptr for pageable memory.
static void* host_device_ptr(const void* host, size_t bytes) {
    if (void* d = pinned_device_ptr(host, bytes)) return d;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host) != hipSuccess) {
        (void)hipGetLastError();                                     // pageable: not an error of this call
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}

// Where the packed host frames' device-to-host copy runs (r04, tools/copy_ab.py and tools/copy_trace.py on MI355X,
// c2 GRAY8, 2.07 MB into pinned memory; us per frame, medians of 5 interleaved rounds x 60 frames):
//                                              synchronous   pipelined (wait f-1)   (wait f-2)
//   copy kernel behind the render (rs)             84-85         74-75               74-75
//   copy kernel on the copy stream (cs), 16 WGs    100           74                  66
//                                     4 / 8 WGs    122 / 108     111 / 77            111 / 64
//   hipMemcpyAsync on the copy stream              106-107       59 / 95 / 290       59 / 95 / 290
// The runtime executes that hipMemcpyAsync as its own blit kernel (__amd_rocclr_copyBuffer in the kernel trace, no
// SDMA transfer in the memory-copy trace, whatever GPU_FORCE_BLIT_COPY_SIZE / ROC_ENABLE_LARGE_BAR /
// HSA_ENABLE_SDMA / GPU_BLIT_ENGINE_TYPE say), and its pipelined rate settles in one of three states per process
// (59, 95 or 290 us) — so the product uses its own copy kernel for both calls: behind the render on `rs` for
// rt_render_packed, on `cs` with 16 workgroups (a copy beside the next render takes CUs from it: fewer
// workgroups leave it more) after a cross-stream event for rt_render_packed_async.
// r05: the HSA runtime does reach the SDMA engines (hsa_amd_memory_async_copy_on_engine; tools/mb_sdma.cpp: engines
// 0-3 move the frame at 44.5 GB/s, 46 us, and take nothing from a kernel running beside them), and a copy queued
// with a dependency signal that the render stream fires starts without the host (copy_mode 3, rt_ctx::Sdma).
// tools/copy_ab.py, same box, 60 frames x 5 rounds:   synchronous   pipelined (wait f-1)   (wait f-2)
//   copy kernel behind the render (rs)                    79.3          69.9                  70.2
//   copy kernel on the copy stream (cs), 16 WGs           95.2          85.3                  85.7
//   SDMA engine behind the render                         81.6          49.6                  49.5
// So rt_render_packed_async defaults to the SDMA engine for page-locked buffers (the copy stream for others or
// when no engine is free) and rt_render_packed to the copy kernel behind the render.  RT_COPY_MODE (1: rs, 0: cs,
// 2: the kernel stores straight into the pinned buffer — 290 us: single-byte stores over PCIe, 3: SDMA),
// RT_COPY_KERNEL (0: hipMemcpyAsync) and RT_COPY_BLOCKS override (A/B; -1 / 0: the defaults above).
constexpr unsigned kCopyStreamBlocks = 16;     // copy kernel beside a render: workgroups (the table above)

// A copy kernel into rt_host_alloc memory (else hipMemcpyAsync); max_blocks: its workgroups (0: one per 4 KB, up to
// 1024).  RT_COPY_KERNEL / RT_COPY_BLOCKS override.
static int copy_to_host(rt_ctx* c, void* host, const void* dev, size_t bytes, hipStream_t st, unsigned max_blocks = 0) {
    if (!bytes) return RT_OK;
    void* dmap = host_device_ptr(host, bytes);
    const bool kernel = c->knobs.copy_kernel != 0;
    if (dmap && kernel && ((uintptr_t)dmap | (uintptr_t)dev) % 16 == 0) {
        unsigned blocks = (unsigned)std::min<size_t>((bytes / 16 + kThreads - 1) / kThreads + 1, 1024);
        if (c->knobs.copy_blocks > 0) max_blocks = (unsigned)c->knobs.copy_blocks;
        if (max_blocks > 0) blocks = std::min(blocks, max_blocks);
        hipLaunchKernelGGL(rt_copy_out_kernel, dim3(blocks), dim3(kThreads), 0, st, (const uint8_t*)dev,
                           (uint8_t*)dmap, bytes);
        RT_HIP(hipGetLastError());
        return RT_OK;
    }
    RT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
    return RT_OK;
}

// Sum a render's per-pixel ray counters into d_sums[0..1]: `words` = 1 for the packed 16 + 16-bit word of the plain
// renders, 2 for the two words per pixel of the sampled ones.
static int queue_raysum(rt_ctx* c, size_t npx, int words, uint32_t* d_rc, unsigned long long* d_sums) {
    RT_HIP(hipMemsetAsync(d_sums, 0, 2 * sizeof(unsigned long long), c->frames.rs));
    hipLaunchKernelGGL(words == 2 ? rt_raysum2_kernel : rt_raysum_kernel,
                       dim3((unsigned)std::min<size_t>((npx + kThreads - 1) / kThreads, 1024)), dim3(kThreads), 0, c->frames.rs,
                       (const uint32_t*)d_rc, npx, d_sums);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// One more context buffer of a host render (rt_render_adaptive's two): `bytes` of buffer k (0: not wanted), copied back
// to `host` when that is given.  dev: filled in by host_render.
struct ExtraBuf {
    int k;
    size_t bytes;
    void* host;
    void* dev;
};

// The host side of rt_render and its sampled siblings, after their argument checks: the context's device buffers for
// the outputs asked for (npx pixels, rc_words counter words each) and for `extra`; the render queued by render(d)
// (d[0..3]: RGBA32F, RGBA8, RGB64F, counters) between the timing events; the ray sums; asynchronous copies back on the
// render stream (rt_host_alloc memory: a copy kernel; other memory: hipMemcpyAsync) and one synchronisation of that
// stream (not of the device: other streams' work is not waited for).  Then primary(&n) gives the primary rays traced
// (every sample is one: the summed segment counters hold them all), from which the statistics are written.
template <class Render, class Primary>
static int host_render(rt_ctx* c, size_t npx, int rc_words, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                       rt_stats* stats, ExtraBuf* extra, int n_extra, Render&& render, Primary&& primary) {
    RT_HIP(hipSetDevice(c->device));
    int rc;
    void* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[5] = {npx * 16, npx * 4, npx * 24, npx * 4 * rc_words, 2 * sizeof(unsigned long long)};
    const bool want[5] = {rgba32f != nullptr, rgba8 != nullptr, rgb64f != nullptr, stats != nullptr, stats != nullptr};
    for (int k = 0; k < 5; ++k)
        if (want[k] && npx > 0 && (rc = ctx_buffer(c, k, bytes[k], &d[k])) != RT_OK) return rc;
    for (int k = 0; k < n_extra; ++k)
        if (extra[k].bytes && (rc = ctx_buffer(c, extra[k].k, extra[k].bytes, &extra[k].dev)) != RT_OK) return rc;
    RT_HIP(hipEventRecord(c->frames.ev0, c->frames.rs));
    if ((rc = render(d)) != RT_OK) return rc;
    RT_HIP(hipEventRecord(c->frames.ev1, c->frames.rs));
    if (stats && npx > 0 && (rc = queue_raysum(c, npx, rc_words, (uint32_t*)d[3], (unsigned long long*)d[4]))) return rc;
    void* host[3] = {rgba32f, rgba8, rgb64f};
    for (int k = 0; k < 3; ++k)
        if (host[k] && npx && (rc = copy_to_host(c, host[k], d[k], bytes[k], c->frames.rs))) return rc;
    for (int k = 0; k < n_extra; ++k)
        if (extra[k].host && (rc = copy_to_host(c, extra[k].host, extra[k].dev, extra[k].bytes, c->frames.rs))) return rc;
    RT_HIP(hipStreamSynchronize(c->frames.rs));
    uint64_t prim = 0;
    if ((rc = primary(&prim)) != RT_OK || !stats) return rc;
    if ((rc = read_stats(c, npx, (const unsigned long long*)d[4], stats)) != RT_OK) return rc;
    stats->reflect_rays = stats->primary_rays + stats->reflect_rays - prim;
    stats->primary_rays = prim;
    return RT_OK;
}

extern "C" int rt_render(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                         const rt_rows* rows, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats) {
    if (!c) return rt_fail(RT_EINVAL, "rt_render: null context");
    int rc = rt_set_scene(c, scene);                    // no device work when the scene is unchanged
    if (rc) return rc;
    int nl = 0;
    rc = render_local_rows(c, cam, W, H, depth, rows, &nl);
    if (rc) return rc;
    const size_t npx = (size_t)nl * W;
    return host_render(
        c, npx, 1, rgba32f, rgba8, rgb64f, stats, nullptr, 0,
        [&](void* const* d) {
            return rt_render_dev(c, cam, W, H, depth, rows, (float*)d[0], (uint8_t*)d[1], (double*)d[2], (uint32_t*)d[3],
                                 c->frames.rs);
        },
        [&](uint64_t* prim) { *prim = npx; return RT_OK; });
}

// The checks the host entry points of the sampled renders share (the _dev calls check the rest).
static int sampled_host_checks(const char* who, const rt_ctx* c, int W, int H, int samples) {
    if (!c) return rt_fail(RT_EINVAL, std::string(who) + ": null context");
    if (ss_log2_of(samples) < 0) return rt_fail(RT_EINVAL, std::string(who) + ": samples must be 1, 2, 4 or 8");
    if (W <= 0 || H <= 0 || (long long)W * H > (1LL << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": bad image size (width, height)");
    return RT_OK;
}

// rt_render for a supersampled frame (rt_render_ss_dev into the context's device buffers, then the copies back).
extern "C" int rt_render_ss(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                            int samples, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats) {
    int rc = sampled_host_checks("rt_render_ss", c, W, H, samples);
    if (rc || (rc = rt_set_scene(c, scene))) return rc;     // no device work when the scene is unchanged
    const size_t npx = (size_t)W * H;
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, nullptr, 0,
        [&](void* const* d) {
            return rt_render_ss_dev(c, cam, W, H, depth, samples, nullptr, (float*)d[0], (uint8_t*)d[1], (double*)d[2],
                                    (uint32_t*)d[3], c->frames.rs);
        },
        [&](uint64_t* prim) { *prim = (uint64_t)npx * (uint64_t)samples * (uint64_t)samples; return RT_OK; });
}

// rt_render for an adaptively supersampled frame: rt_render_adaptive_dev into the context's device buffers (its
// workspace among them), then the copies back.
extern "C" int rt_render_adaptive(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                                  int samples, int threshold, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                  uint8_t* refined, rt_stats* stats, uint64_t* n_refined) {
    int rc = sampled_host_checks("rt_render_adaptive", c, W, H, samples);
    if (rc) return rc;
    if (threshold < -1 || threshold > 255)
        return rt_fail(RT_EINVAL, "rt_render_adaptive: threshold must lie in -1 .. 255");
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    const size_t npx = (size_t)W * H;
    const size_t ws_bytes = rt_adaptive_layout(npx).bytes;
    ExtraBuf x[2] = {{rt_ctx::Frames::kBufRefined, refined ? npx : 0, refined, nullptr},
                     {rt_ctx::Frames::kBufAdaptive, ws_bytes, nullptr, nullptr}};
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, x, 2,
        [&](void* const* d) {
            return rt_render_adaptive_dev(c, cam, W, H, depth, samples, threshold, (float*)d[0], (uint8_t*)d[1],
                                          (double*)d[2], (uint32_t*)d[3], (uint8_t*)x[0].dev, x[1].dev, ws_bytes, c->frames.rs);
        },
        [&](uint64_t* prim) {
            uint32_t n = 0;                                 // the work list's length: the refined pixels
            RT_HIP(hipMemcpy(&n, x[1].dev, sizeof(n), hipMemcpyDeviceToHost));
            if (n_refined) *n_refined = n;
            // one primary ray per unrefined pixel, S * S per refined one
            *prim = (uint64_t)(npx - n) + (uint64_t)n * (uint64_t)samples * (uint64_t)samples;
            return RT_OK;
        });
}

// rt_render for a frame of the kind: lens_render_dev (as `who`_dev) into the context's device buffers, then the copies
// back.  Motion: rt_set_motion after rt_set_scene; displacement = nullptr: no motion.
static int lens_render_host(LensKind kind, const char* who, rt_ctx* c, const rt_scene* scene,
                            const double* displacement, const rt_camera* cam, int W, int H, int depth, int samples,
                            double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                            double* rgb64f, rt_stats* stats) {
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc || (rc = lens_arg_checks(kind, who, aperture, light_size, shutter))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if (kind == kLensMotion && (rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0)))
        return rc;                                          // nor when the motion is
    const size_t npx = (size_t)W * H;
    const std::string dev = std::string(who) + "_dev";
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, nullptr, 0,
        [&](void* const* d) {
            return lens_render_dev(kind, dev.c_str(), c, cam, W, H, depth, samples, aperture, light_size, shutter,
                                   (float*)d[0], (uint8_t*)d[1], (double*)d[2], (uint32_t*)d[3], c->frames.rs);
        },
        [&](uint64_t* prim) { *prim = (uint64_t)npx * (uint64_t)samples * (uint64_t)samples; return RT_OK; });
}

extern "C" int rt_render_dof(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                             int samples, double aperture, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                             rt_stats* stats) {
    return lens_render_host(kLensDof, "rt_render_dof", c, scene, nullptr, cam, W, H, depth, samples, aperture, 0.0, 0.0,
                            rgba32f, rgba8, rgb64f, stats);
}

extern "C" int rt_render_soft(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                              int samples, double aperture, double light_size, float* rgba32f, uint8_t* rgba8,
                              double* rgb64f, rt_stats* stats) {
    return lens_render_host(kLensSoft, "rt_render_soft", c, scene, nullptr, cam, W, H, depth, samples, aperture,
                            light_size, 0.0, rgba32f, rgba8, rgb64f, stats);
}

extern "C" int rt_render_motion(rt_ctx* c, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                                int W, int H, int depth, int samples, double aperture, double light_size,
                                double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats) {
    return lens_render_host(kLensMotion, "rt_render_motion", c, scene, displacement, cam, W, H, depth, samples,
                            aperture, light_size, shutter, rgba32f, rgba8, rgb64f, stats);
}

// rt_render for a jittered frame: rt_render_motion's steps with jitter_render_dev (as rt_render_jitter_dev).
extern "C" int rt_render_jitter(rt_ctx* c, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                                int W, int H, int depth, int samples, int jitter, uint32_t seed, double aperture,
                                double light_size, double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                rt_stats* stats) {
    const char* who = "rt_render_jitter";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc || (rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const size_t npx = (size_t)W * H;
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, nullptr, 0,
        [&](void* const* d) {
            return jitter_render_dev("rt_render_jitter_dev", c, cam, W, H, depth, samples, jitter, seed, aperture,
                                     light_size, shutter, (float*)d[0], (uint8_t*)d[1], (double*)d[2], (uint32_t*)d[3],
                                     c->frames.rs);
        },
        [&](uint64_t* prim) { *prim = (uint64_t)npx * (uint64_t)samples * (uint64_t)samples; return RT_OK; });
}

// rt_render for a frame with a moving camera: rt_render_jitter's steps with shutter_render_dev (as rt_render_shutter_dev).
extern "C" int rt_render_shutter(rt_ctx* c, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                                 const rt_camera_motion* motion, int W, int H, int depth, int samples, int jitter,
                                 uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f,
                                 uint8_t* rgba8, double* rgb64f, rt_stats* stats) {
    const char* who = "rt_render_shutter";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc || (rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const size_t npx = (size_t)W * H;
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, nullptr, 0,
        [&](void* const* d) {
            return shutter_render_dev("rt_render_shutter_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                                      aperture, light_size, shutter, (float*)d[0], (uint8_t*)d[1], (double*)d[2],
                                      (uint32_t*)d[3], c->frames.rs);
        },
        [&](uint64_t* prim) { *prim = (uint64_t)npx * (uint64_t)samples * (uint64_t)samples; return RT_OK; });
}

// rt_render for accumulated passes: rt_render_shutter's steps with accum_render_dev (as rt_render_accum_dev) on a
// device copy of `accum`, which is uploaded first when the call continues a sum (first_pass > 0) and copied back after
// the render.  The counters behind *stats are the call's, so its primary rays are those of all its passes.
extern "C" int rt_render_accum(rt_ctx* c, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                               const rt_camera_motion* motion, int W, int H, int depth, int samples, int jitter,
                               uint32_t seed, uint32_t first_pass, int passes, double aperture, double light_size,
                               double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                               rt_stats* stats) {
    const char* who = "rt_render_accum";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc || (rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (passes < 1 || passes > kAccumCallPasses)
        return rt_fail(RT_EINVAL, std::string(who) + ": passes must lie in 1 .. 65536");
    if ((uint64_t)first_pass + (uint64_t)passes > (1ull << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": first_pass + passes must not exceed 2^31");
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const size_t npx = (size_t)W * H;
    ExtraBuf x[1] = {{rt_ctx::Frames::kBufAccum, npx * 24, accum, nullptr}};
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, x, 1,
        [&](void* const* d) {
            if (first_pass > 0) RT_HIP(hipMemcpyAsync(x[0].dev, accum, npx * 24, hipMemcpyHostToDevice, c->frames.rs));
            return accum_render_dev("rt_render_accum_dev", c, cam, motion, W, H, depth, samples, jitter, seed, first_pass,
                                    passes, aperture, light_size, shutter, (double*)x[0].dev, (float*)d[0],
                                    (uint8_t*)d[1], (double*)d[2], (uint32_t*)d[3], c->frames.rs);
        },
        [&](uint64_t* prim) {
            *prim = (uint64_t)npx * (uint64_t)samples * (uint64_t)samples * (uint64_t)passes;
            return RT_OK;
        });
}

// rt_render for converging passes: rt_render_accum's steps with converge_render_dev (as rt_render_converge_dev) on
// device copies of the three state arrays, all uploaded first (a pixel's `count` says whether its sums are read) and
// copied back after the render.  The pass counts before the call are kept on the host, so that the primary rays behind
// *stats are those of the pixel-passes this call traced for the pixels that received them.
extern "C" int rt_render_converge(rt_ctx* c, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                                  const rt_camera_motion* motion, int W, int H, int depth, int samples, int jitter,
                                  uint32_t seed, int passes, uint32_t min_passes, double tolerance, double aperture,
                                  double light_size, double shutter, double* accum, double* accum2, uint32_t* count,
                                  float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats, uint64_t* n_active) {
    const char* who = "rt_render_converge";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc || (rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (!accum2) return rt_fail(RT_EINVAL, std::string(who) + ": null accum2");
    if (!count) return rt_fail(RT_EINVAL, std::string(who) + ": null count");
    if ((rc = converge_arg_checks(who, passes, min_passes, tolerance))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const size_t npx = (size_t)W * H;
    uint64_t before = 0;                                    // the pixel-passes the state holds
    for (size_t k = 0; k < npx; ++k) before += count[k];
    ExtraBuf x[4] = {{rt_ctx::Frames::kBufAccum, npx * 24, accum, nullptr},
                     {rt_ctx::Frames::kBufAccum2, npx * 24, accum2, nullptr},
                     {rt_ctx::Frames::kBufCount, npx * 4, count, nullptr},
                     {rt_ctx::Frames::kBufActive, 4, nullptr, nullptr}};
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, x, 4,
        [&](void* const* d) {
            RT_HIP(hipMemcpyAsync(x[0].dev, accum, npx * 24, hipMemcpyHostToDevice, c->frames.rs));
            RT_HIP(hipMemcpyAsync(x[1].dev, accum2, npx * 24, hipMemcpyHostToDevice, c->frames.rs));
            RT_HIP(hipMemcpyAsync(x[2].dev, count, npx * 4, hipMemcpyHostToDevice, c->frames.rs));
            return converge_render_dev("rt_render_converge_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                                       passes, min_passes, tolerance, aperture, light_size, shutter, (double*)x[0].dev,
                                       (double*)x[1].dev, (uint32_t*)x[2].dev, (float*)d[0], (uint8_t*)d[1],
                                       (double*)d[2], (uint32_t*)d[3], (uint32_t*)x[3].dev, c->frames.rs);
        },
        [&](uint64_t* prim) {
            uint32_t n = 0;
            RT_HIP(hipMemcpy(&n, x[3].dev, sizeof(n), hipMemcpyDeviceToHost));
            if (n_active) *n_active = n;
            uint64_t after = 0;                             // (the copies back are done: host_render synchronised)
            for (size_t k = 0; k < npx; ++k) after += count[k];
            *prim = (after - before) * (uint64_t)samples * (uint64_t)samples;
            return RT_OK;
        });
}

// ---- windows of the accumulating and converging renders into host memory (include/rt_api.h) -------------------------
// One per-pixel host array of a windowed host render: context buffer k, `elem` bytes per pixel, addressed on the host
// with the window's stride; dev: its dense width x height device copy, filled in by host_render_window.
struct WinBuf {
    int k;
    size_t elem;
    void* host;
    void* dev;
};

// Rows of a window between a strided host array and its dense device copy: only the window's own elements move.
static int window_copy(const rt_window& w, const WinBuf& b, bool to_device, hipStream_t st) {
    const size_t row = (size_t)w.width * b.elem, pitch = (size_t)w.stride * b.elem;
    if (to_device) RT_HIP(hipMemcpy2DAsync(b.dev, row, b.host, pitch, row, (size_t)w.height, hipMemcpyHostToDevice, st));
    else RT_HIP(hipMemcpy2DAsync(b.host, pitch, b.dev, row, row, (size_t)w.height, hipMemcpyDeviceToHost, st));
    return RT_OK;
}

// host_render for a window: dense device buffers of the window's pixels (b[0..2]: RGBA32F, RGBA8, RGB64F as the caller
// gave them; then n_extra more), render(dense window, counters) between the timing events, the ray sums, the rows back
// with the stride, one synchronisation of the render stream, then the statistics from primary(&n).
template <class Render, class Primary>
static int host_render_window(rt_ctx* c, const rt_window& w, WinBuf* b, int n_extra, rt_stats* stats, Render&& render,
                              Primary&& primary) {
    RT_HIP(hipSetDevice(c->device));
    int rc;
    const size_t npx = (size_t)w.width * (size_t)w.height;
    for (int k = 0; k < 3 + n_extra; ++k)
        if ((b[k].host || k >= 3) && (rc = ctx_buffer(c, b[k].k, npx * b[k].elem, &b[k].dev)) != RT_OK) return rc;
    void *d_rc = nullptr, *d_sums = nullptr;
    if (stats && ((rc = ctx_buffer(c, 3, npx * 8, &d_rc)) || (rc = ctx_buffer(c, 4, 2 * sizeof(unsigned long long), &d_sums))))
        return rc;
    const rt_window dense{w.x0, w.y0, w.width, w.height, w.width};
    RT_HIP(hipEventRecord(c->frames.ev0, c->frames.rs));
    if ((rc = render(dense, (uint32_t*)d_rc)) != RT_OK) return rc;
    RT_HIP(hipEventRecord(c->frames.ev1, c->frames.rs));
    if (stats && (rc = queue_raysum(c, npx, 2, (uint32_t*)d_rc, (unsigned long long*)d_sums))) return rc;
    for (int k = 0; k < 3 + n_extra; ++k)
        if (b[k].host && (rc = window_copy(w, b[k], false, c->frames.rs))) return rc;
    RT_HIP(hipStreamSynchronize(c->frames.rs));
    uint64_t prim = 0;
    if ((rc = primary(&prim)) != RT_OK || !stats) return rc;
    if ((rc = read_stats(c, npx, (const unsigned long long*)d_sums, stats)) != RT_OK) return rc;
    stats->reflect_rays = stats->primary_rays + stats->reflect_rays - prim;
    stats->primary_rays = prim;
    return RT_OK;
}

// rt_render_accum for a window: the checks first, then only the window's rows of `accum` go up (first_pass > 0) and only
// the window's rows of every array come back.
extern "C" int rt_render_accum_window(rt_ctx* c, const rt_scene* scene, const double* displacement,
                                      const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                      const rt_window* win, int depth, int samples, int jitter, uint32_t seed,
                                      uint32_t first_pass, int passes, double aperture, double light_size,
                                      double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                      rt_stats* stats) {
    const char* who = "rt_render_accum_window";
    int rc = window_arg_checks(who, win, W, H);             // first: no context is needed to reject a window
    if (rc || (rc = sampled_host_checks(who, c, W, H, samples))) return rc;
    if ((rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (passes < 1 || passes > kAccumCallPasses)
        return rt_fail(RT_EINVAL, std::string(who) + ": passes must lie in 1 .. 65536");
    if ((uint64_t)first_pass + (uint64_t)passes > (1ull << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": first_pass + passes must not exceed 2^31");
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    WinBuf b[4] = {{0, 16, rgba32f, nullptr}, {1, 4, rgba8, nullptr}, {2, 24, rgb64f, nullptr},
                   {rt_ctx::Frames::kBufAccum, 24, accum, nullptr}};
    return host_render_window(
        c, *win, b, 1, stats,
        [&](const rt_window& dense, uint32_t* d_rc) {
            int r;
            if (first_pass > 0 && (r = window_copy(*win, b[3], true, c->frames.rs))) return r;
            return accum_render_dev("rt_render_accum_window_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                                    first_pass, passes, aperture, light_size, shutter, (double*)b[3].dev,
                                    (float*)b[0].dev, (uint8_t*)b[1].dev, (double*)b[2].dev, d_rc, c->frames.rs, &dense);
        },
        [&](uint64_t* prim) {
            *prim = (uint64_t)win->width * (uint64_t)win->height * (uint64_t)samples * (uint64_t)samples * (uint64_t)passes;
            return RT_OK;
        });
}

// rt_render_converge for a window: the window's rows of the three state arrays go up and come back; *n_active and the
// primary rays behind *stats are the window's.
extern "C" int rt_render_converge_window(rt_ctx* c, const rt_scene* scene, const double* displacement,
                                         const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                                         const rt_window* win, int depth, int samples, int jitter, uint32_t seed,
                                         int passes, uint32_t min_passes, double tolerance, double aperture,
                                         double light_size, double shutter, double* accum, double* accum2,
                                         uint32_t* count, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                         rt_stats* stats, uint64_t* n_active) {
    const char* who = "rt_render_converge_window";
    int rc = window_arg_checks(who, win, W, H);             // first: no context is needed to reject a window
    if (rc || (rc = sampled_host_checks(who, c, W, H, samples))) return rc;
    if ((rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (!accum2) return rt_fail(RT_EINVAL, std::string(who) + ": null accum2");
    if (!count) return rt_fail(RT_EINVAL, std::string(who) + ": null count");
    if ((rc = converge_arg_checks(who, passes, min_passes, tolerance))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const auto passes_held = [&]() {                        // the pixel-passes the window's state holds
        uint64_t n = 0;
        for (int j = 0; j < win->height; ++j)
            for (int i = 0; i < win->width; ++i) n += count[(size_t)j * (size_t)win->stride + (size_t)i];
        return n;
    };
    const uint64_t before = passes_held();
    WinBuf b[6] = {{0, 16, rgba32f, nullptr}, {1, 4, rgba8, nullptr}, {2, 24, rgb64f, nullptr},
                   {rt_ctx::Frames::kBufAccum, 24, accum, nullptr}, {rt_ctx::Frames::kBufAccum2, 24, accum2, nullptr},
                   {rt_ctx::Frames::kBufCount, 4, count, nullptr}};
    void* d_active = nullptr;
    if ((rc = ctx_buffer(c, rt_ctx::Frames::kBufActive, 4, &d_active))) return rc;
    return host_render_window(
        c, *win, b, 3, stats,
        [&](const rt_window& dense, uint32_t* d_rc) {
            int r;
            for (int k = 3; k < 6; ++k)
                if ((r = window_copy(*win, b[k], true, c->frames.rs))) return r;
            return converge_render_dev("rt_render_converge_window_dev", c, cam, motion, W, H, depth, samples, jitter,
                                       seed, passes, min_passes, tolerance, aperture, light_size, shutter,
                                       (double*)b[3].dev, (double*)b[4].dev, (uint32_t*)b[5].dev, (float*)b[0].dev,
                                       (uint8_t*)b[1].dev, (double*)b[2].dev, d_rc, (uint32_t*)d_active, c->frames.rs,
                                       &dense);
        },
        [&](uint64_t* prim) {
            uint32_t n = 0;
            RT_HIP(hipMemcpy(&n, d_active, sizeof(n), hipMemcpyDeviceToHost));
            if (n_active) *n_active = n;
            *prim = (passes_held() - before) * (uint64_t)samples * (uint64_t)samples;
            return RT_OK;
        });
}

// ---- lists of windows of the accumulating and converging renders into host memory (include/rt_api.h) ----------------
// Rows of every window of the context's list between a host array and its device copy, both laid out as the plan says
// (window k's pixel (0, 0) at element offset[k], rows `stride` elements apart): only the windows' own elements move.  A
// packed list is one run of elements, moved in one copy.
static int window_list_copy(const rt_ctx* c, const WinBuf& b, bool to_device, hipStream_t st) {
    const rt_ctx::Windows& L = c->windows;
    if (L.layout == RT_WINDOWS_PACKED) {
        const size_t bytes = (size_t)L.elements * b.elem;
        if (to_device) RT_HIP(hipMemcpyAsync(b.dev, b.host, bytes, hipMemcpyHostToDevice, st));
        else RT_HIP(hipMemcpyAsync(b.host, b.dev, bytes, hipMemcpyDeviceToHost, st));
        return RT_OK;
    }
    for (size_t k = 0; k < L.list.size(); ++k) {
        const rt_window& w = L.list[k];
        const size_t off = (size_t)L.offset[k] * b.elem;
        const size_t row = (size_t)w.width * b.elem, pitch = (size_t)w.stride * b.elem;
        char *h = (char*)b.host + off, *d = (char*)b.dev + off;
        if (to_device) RT_HIP(hipMemcpy2DAsync(d, pitch, h, pitch, row, (size_t)w.height, hipMemcpyHostToDevice, st));
        else RT_HIP(hipMemcpy2DAsync(h, pitch, d, pitch, row, (size_t)w.height, hipMemcpyDeviceToHost, st));
    }
    return RT_OK;
}

// The pixels of the context's list.
static uint64_t window_list_pixels(const rt_ctx* c) {
    uint64_t n = 0;
    for (const rt_window& w : c->windows.list) n += (uint64_t)w.width * (uint64_t)w.height;
    return n;
}

// host_render_window for the context's list: device buffers of the plan's `elements` elements in the plan's layout.  The
// counters of elements that belong to no window are zeroed before the render, so the ray sums are the list's.
template <class Render, class Primary>
static int host_render_windows(rt_ctx* c, WinBuf* b, int n_extra, rt_stats* stats, Render&& render, Primary&& primary) {
    RT_HIP(hipSetDevice(c->device));
    int rc;
    const size_t nel = (size_t)c->windows.elements;
    for (int k = 0; k < 3 + n_extra; ++k)
        if ((b[k].host || k >= 3) && (rc = ctx_buffer(c, b[k].k, nel * b[k].elem, &b[k].dev)) != RT_OK) return rc;
    void *d_rc = nullptr, *d_sums = nullptr;
    if (stats && ((rc = ctx_buffer(c, 3, nel * 8, &d_rc)) || (rc = ctx_buffer(c, 4, 2 * sizeof(unsigned long long), &d_sums))))
        return rc;
    if (stats) RT_HIP(hipMemsetAsync(d_rc, 0, nel * 8, c->frames.rs));
    RT_HIP(hipEventRecord(c->frames.ev0, c->frames.rs));
    if ((rc = render((uint32_t*)d_rc)) != RT_OK) return rc;
    RT_HIP(hipEventRecord(c->frames.ev1, c->frames.rs));
    if (stats && (rc = queue_raysum(c, nel, 2, (uint32_t*)d_rc, (unsigned long long*)d_sums))) return rc;
    for (int k = 0; k < 3 + n_extra; ++k)
        if (b[k].host && (rc = window_list_copy(c, b[k], false, c->frames.rs))) return rc;
    RT_HIP(hipStreamSynchronize(c->frames.rs));
    uint64_t prim = 0;
    if ((rc = primary(&prim)) != RT_OK || !stats) return rc;
    if ((rc = read_stats(c, nel, (const unsigned long long*)d_sums, stats)) != RT_OK) return rc;
    stats->reflect_rays = stats->primary_rays + stats->reflect_rays - prim;
    stats->primary_rays = prim;
    return RT_OK;
}

// rt_render_accum for a list of windows: the checks first, then the list, the scene and the motion are set, only the windows' rows of `accum` go up
// (first_pass > 0) and only the windows' rows of every array come back.
extern "C" int rt_render_accum_windows(rt_ctx* c, const rt_scene* scene, const double* displacement,
                                       const rt_camera* cam, const rt_camera_motion* motion, int W, int H, int depth,
                                       int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes,
                                       double aperture, double light_size, double shutter, double* accum, float* rgba32f,
                                       uint8_t* rgba8, double* rgb64f, rt_stats* stats, const rt_window* wins, int n,
                                       int layout) {
    const char* who = "rt_render_accum_windows";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc) return rc;
    if ((rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (passes < 1 || passes > kAccumCallPasses)
        return rt_fail(RT_EINVAL, std::string(who) + ": passes must lie in 1 .. 65536");
    if ((uint64_t)first_pass + (uint64_t)passes > (1ull << 31))
        return rt_fail(RT_EINVAL, std::string(who) + ": first_pass + passes must not exceed 2^31");
    // the list first: a bad one is rejected before the scene changes; the list in force again costs no check
    if (!wins) return rt_fail(RT_EINVAL, std::string(who) + ": null wins");
    if ((rc = rt_set_windows(c, W, H, wins, n, layout))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    WinBuf b[4] = {{0, 16, rgba32f, nullptr}, {1, 4, rgba8, nullptr}, {2, 24, rgb64f, nullptr},
                   {rt_ctx::Frames::kBufAccum, 24, accum, nullptr}};
    return host_render_windows(
        c, b, 1, stats,
        [&](uint32_t* d_rc) {
            int r;
            if (first_pass > 0 && (r = window_list_copy(c, b[3], true, c->frames.rs))) return r;
            return accum_render_dev("rt_render_accum_windows_dev", c, cam, motion, W, H, depth, samples, jitter, seed,
                                    first_pass, passes, aperture, light_size, shutter, (double*)b[3].dev,
                                    (float*)b[0].dev, (uint8_t*)b[1].dev, (double*)b[2].dev, d_rc, c->frames.rs, nullptr,
                                    true);
        },
        [&](uint64_t* prim) {
            *prim = window_list_pixels(c) * (uint64_t)samples * (uint64_t)samples * (uint64_t)passes;
            return RT_OK;
        });
}

// rt_render_converge for a list of windows: the windows' rows of the three state arrays go up and come back; *n_active
// and the primary rays behind *stats are the list's.
extern "C" int rt_render_converge_windows(rt_ctx* c, const rt_scene* scene, const double* displacement,
                                          const rt_camera* cam, const rt_camera_motion* motion, int W, int H, int depth,
                                          int samples, int jitter, uint32_t seed, int passes, uint32_t min_passes,
                                          double tolerance, double aperture, double light_size, double shutter,
                                          double* accum, double* accum2, uint32_t* count, float* rgba32f, uint8_t* rgba8,
                                          double* rgb64f, rt_stats* stats, uint64_t* n_active, const rt_window* wins,
                                          int n, int layout) {
    const char* who = "rt_render_converge_windows";
    int rc = sampled_host_checks(who, c, W, H, samples);
    if (rc) return rc;
    if ((rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = jitter_arg_checks(who, jitter))) return rc;
    if (!accum) return rt_fail(RT_EINVAL, std::string(who) + ": null accum");
    if (!accum2) return rt_fail(RT_EINVAL, std::string(who) + ": null accum2");
    if (!count) return rt_fail(RT_EINVAL, std::string(who) + ": null count");
    if ((rc = converge_arg_checks(who, passes, min_passes, tolerance))) return rc;
    // the list first: a bad one is rejected before the scene changes; the list in force again costs no check
    if (!wins) return rt_fail(RT_EINVAL, std::string(who) + ": null wins");
    if ((rc = rt_set_windows(c, W, H, wins, n, layout))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const auto passes_held = [&]() {                        // the pixel-passes the list's state holds
        uint64_t held = 0;
        for (size_t k = 0; k < c->windows.list.size(); ++k) {
            const rt_window& w = c->windows.list[k];
            const uint32_t* p = count + c->windows.offset[k];
            for (int j = 0; j < w.height; ++j)
                for (int i = 0; i < w.width; ++i) held += p[(size_t)j * (size_t)w.stride + (size_t)i];
        }
        return held;
    };
    const uint64_t before = passes_held();
    WinBuf b[6] = {{0, 16, rgba32f, nullptr}, {1, 4, rgba8, nullptr}, {2, 24, rgb64f, nullptr},
                   {rt_ctx::Frames::kBufAccum, 24, accum, nullptr}, {rt_ctx::Frames::kBufAccum2, 24, accum2, nullptr},
                   {rt_ctx::Frames::kBufCount, 4, count, nullptr}};
    void* d_active = nullptr;
    if ((rc = ctx_buffer(c, rt_ctx::Frames::kBufActive, 4, &d_active))) return rc;
    return host_render_windows(
        c, b, 3, stats,
        [&](uint32_t* d_rc) {
            int r;
            for (int k = 3; k < 6; ++k)
                if ((r = window_list_copy(c, b[k], true, c->frames.rs))) return r;
            return converge_render_dev("rt_render_converge_windows_dev", c, cam, motion, W, H, depth, samples, jitter,
                                       seed, passes, min_passes, tolerance, aperture, light_size, shutter,
                                       (double*)b[3].dev, (double*)b[4].dev, (uint32_t*)b[5].dev, (float*)b[0].dev,
                                       (uint8_t*)b[1].dev, (double*)b[2].dev, d_rc, (uint32_t*)d_active, c->frames.rs,
                                       nullptr, true);
        },
        [&](uint64_t* prim) {
            uint32_t live = 0;
            RT_HIP(hipMemcpy(&live, d_active, sizeof(live), hipMemcpyDeviceToHost));
            if (n_active) *n_active = live;
            *prim = (passes_held() - before) * (uint64_t)samples * (uint64_t)samples;
            return RT_OK;
        });
}

// rt_render for an adaptively sampled frame of the lens family: rt_set_scene, rt_set_motion (nullptr: none), then
// rt_render_lens_adaptive_dev into the context's device buffers (rt_render_adaptive's two among them), then the copies
// back.
extern "C" int rt_render_lens_adaptive(rt_ctx* c, const rt_scene* scene, const double* displacement,
                                       const rt_camera* cam, int W, int H, int depth, int samples_lo, int samples_hi,
                                       int threshold, double aperture, double light_size, double shutter,
                                       float* rgba32f, uint8_t* rgba8, double* rgb64f, uint8_t* refined,
                                       rt_stats* stats, uint64_t* n_refined) {
    const char* who = "rt_render_lens_adaptive";
    int rc = sampled_host_checks(who, c, W, H, samples_lo);
    if (rc || (rc = sampled_host_checks(who, c, W, H, samples_hi))) return rc;
    if (samples_lo > samples_hi) return rt_fail(RT_EINVAL, std::string(who) + ": samples_lo must not exceed samples_hi");
    if (threshold < -1 || threshold > 255)
        return rt_fail(RT_EINVAL, std::string(who) + ": threshold must lie in -1 .. 255");
    if ((rc = lens_arg_checks(kLensMotion, who, aperture, light_size, shutter))) return rc;
    if ((rc = rt_set_scene(c, scene))) return rc;           // no device work when the scene is unchanged
    if ((rc = rt_set_motion(c, displacement, displacement ? scene->n_spheres : 0))) return rc;   // nor when the motion is
    const size_t npx = (size_t)W * H;
    const size_t ws_bytes = rt_lens_adaptive_layout(npx).bytes;
    ExtraBuf x[2] = {{rt_ctx::Frames::kBufRefined, refined ? npx : 0, refined, nullptr},
                     {rt_ctx::Frames::kBufAdaptive, ws_bytes, nullptr, nullptr}};
    return host_render(
        c, npx, 2, rgba32f, rgba8, rgb64f, stats, x, 2,
        [&](void* const* d) {
            return rt_render_lens_adaptive_dev(c, cam, W, H, depth, samples_lo, samples_hi, threshold, aperture,
                                               light_size, shutter, (float*)d[0], (uint8_t*)d[1], (double*)d[2],
                                               (uint32_t*)d[3], (uint8_t*)x[0].dev, x[1].dev, ws_bytes, c->frames.rs);
        },
        [&](uint64_t* prim) {
            uint32_t n = 0;                                 // the work list's length: the refined pixels
            RT_HIP(hipMemcpy(&n, x[1].dev, sizeof(n), hipMemcpyDeviceToHost));
            if (n_refined) *n_refined = n;
            *prim = (uint64_t)(npx - n) * (uint64_t)(samples_lo * samples_lo) +
                    (uint64_t)n * (uint64_t)(samples_hi * samples_hi);
            return RT_OK;
        });
}

// ---- copy_mode 3: device-to-host frames on an SDMA engine (HSA runtime, hsa_amd_memory_async_copy_on_engine) ----
struct SdmaAgents {
    uint32_t domain = 0, bdf = 0;
    hsa_agent_t gpu{0}, cpu{0};
};
static hsa_status_t sdma_find_agent(hsa_agent_t a, void* data) {
    SdmaAgents* f = static_cast<SdmaAgents*>(data);
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (t == HSA_DEVICE_TYPE_CPU && f->cpu.handle == 0) f->cpu = a;
    if (t == HSA_DEVICE_TYPE_GPU) {
        uint32_t dom = 0, bdf = 0;
        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &dom);
        hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf);
        if (dom == f->domain && bdf == f->bdf) f->gpu = a;
    }
    return HSA_STATUS_SUCCESS;
}

__global__ void __launch_bounds__(64) rt_signal_fire_kernel(int64_t* value) {
    if (threadIdx.x == 0) __hip_atomic_store(value, (int64_t)0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Queue "slot b's frame is in its device buffer" on the render stream: store 0 into sdma.dep[b] (writer 1: the
// stream's write-value operation, 2: a one-wave kernel behind the render).
static hipError_t sdma_fire(rt_ctx* c, int b, int writer) {
    if (writer == 1) return hipStreamWriteValue64(c->frames.rs, (void*)c->sdma.dep_ptr[b], 0, 0);
    hipLaunchKernelGGL(rt_signal_fire_kernel, dim3(1), dim3(64), 0, c->frames.rs, (int64_t*)c->sdma.dep_ptr[b]);
    return hipGetLastError();
}

// The context's GPU agent (matched to its HIP device by PCI domain / bus / device / function), a CPU agent, a free SDMA
// engine between them and the per-slot signals; false (once, remembered) when any of it is missing.
static bool sdma_init(rt_ctx* c) {
    if (c->sdma.tried) return c->sdma.ok;
    c->sdma.tried = true;
    char bus[64] = {};
    unsigned dom = 0, b = 0, d = 0, f = 0;
    if (hipDeviceGetPCIBusId(bus, sizeof bus, c->device) != hipSuccess ||
        sscanf(bus, "%x:%x:%x.%x", &dom, &b, &d, &f) != 4 || hsa_init() != HSA_STATUS_SUCCESS)
        return false;
    SdmaAgents ag;
    ag.domain = dom;
    ag.bdf = (b << 8) | (d << 3) | f;
    uint32_t mask = 0;
    if (hsa_iterate_agents(sdma_find_agent, &ag) != HSA_STATUS_SUCCESS || !ag.gpu.handle || !ag.cpu.handle ||
        hsa_amd_memory_copy_engine_status(ag.cpu, ag.gpu, &mask) != HSA_STATUS_SUCCESS || mask == 0) {
        hsa_shut_down();
        return false;
    }
    // sdma.dep is waited on by the copy engine only (GPU_ONLY: the one kind whose value a stream or kernel may store)
    bool ok = true;
    for (int k = 0; k < rt_ctx::kSlots && ok; ++k)
        ok = hsa_amd_signal_create(1, 0, nullptr, HSA_AMD_SIGNAL_AMD_GPU_ONLY, &c->sdma.dep[k]) == HSA_STATUS_SUCCESS &&
             hsa_signal_create(0, 0, nullptr, &c->sdma.done[k][0]) == HSA_STATUS_SUCCESS &&
             hsa_signal_create(0, 0, nullptr, &c->sdma.done[k][1]) == HSA_STATUS_SUCCESS &&
             hsa_amd_signal_value_pointer(c->sdma.dep[k], &c->sdma.dep_ptr[k]) == HSA_STATUS_SUCCESS &&
             hipEventCreateWithFlags(&c->sdma.fired[k], hipEventDisableTiming) == hipSuccess;
    // how the render stream fires it: a one-wave kernel's system-scope store, else the stream's own write
    // (hipStreamWriteValue64); each is tried once on slot 0's signal and must be seen from the host.  (r06: the kernel
    // first — the same speed, profiles/r06/ab/copy_ab_sdma_writer.json — and a plain store into memory the HSA runtime
    // allocated, where the write-value hands the runtime a pointer it did not allocate.)
    if (ok) {
        c->sdma.writer = 0;
        for (int w : {2, 1}) {
            if (c->sdma.writer) break;
            if (c->knobs.sd_writer_req && w != c->knobs.sd_writer_req) continue;
            hsa_signal_store_screlease(c->sdma.dep[0], 1);
            if (sdma_fire(c, 0, w) == hipSuccess && hipStreamSynchronize(c->frames.rs) == hipSuccess &&
                hsa_signal_load_scacquire(c->sdma.dep[0]) == 0)
                c->sdma.writer = w;
            (void)hipGetLastError();
        }
        ok = c->sdma.writer != 0;
    }
    if (!ok) {
        for (int k = 0; k < rt_ctx::kSlots; ++k) {
            if (c->sdma.dep[k].handle) hsa_signal_destroy(c->sdma.dep[k]);
            for (int h = 0; h < 2; ++h)
                if (c->sdma.done[k][h].handle) hsa_signal_destroy(c->sdma.done[k][h]);
            if (c->sdma.fired[k]) (void)hipEventDestroy(c->sdma.fired[k]);
            c->sdma.fired[k] = nullptr;
        }
        hsa_shut_down();
        return false;
    }
    c->sdma.gpu = ag.gpu;
    c->sdma.cpu = ag.cpu;
    c->sdma.engine = mask & (~mask + 1);                 // the lowest free engine
    const uint32_t rest = mask & ~c->sdma.engine;
    c->sdma.engine2 = rest & (~rest + 1);                 // and the next (0: none)
    c->sdma.ok = true;
    return true;
}

// Wait until slot b's SDMA copies are done.  Elapsed time alone is not a failure: a deep frame may still be queued
// behind others on the render stream.  Every knobs.sd_wait_ms the render stream's progress is checked (sdma.fired, recorded
// right after the frame's sdma_fire): while that event is pending the render is running, and once it has completed the
// dependency has fired and the engines finish the copy — both keep waiting.  Only a render stream that reports an
// error (its write never comes) has its dependency released by hand, so the engines are not left waiting; the stream
// is then drained before the slot is reused, so no stale write of this frame can release a later frame's copy early.
static int sdma_wait(rt_ctx* c, int b) {
    if (!c->sdma.pending[b]) return RT_OK;
    // (the wait's timeout is a hint in timestamp ticks and may return early: the deadline is kept here)
    uint64_t freq = 0;
    if (hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &freq) != HSA_STATUS_SUCCESS || freq == 0) freq = 1000000000;
    const auto period = std::chrono::milliseconds(c->knobs.sd_wait_ms);
    auto done_by = [&](std::chrono::steady_clock::time_point deadline) {
        for (int h = 0; h < c->sdma.copies[b]; ++h) {
            hsa_signal_value_t v = 1;
            for (;;) {
                // the wait's hint: at most 100 ms and no later than the deadline (0 at RT_SDMA_WAIT_MS=0: a poll)
                const auto left = std::chrono::duration_cast<std::chrono::nanoseconds>(
                    deadline - std::chrono::steady_clock::now()).count();
                const uint64_t hint = left <= 0 ? 0 : std::min<uint64_t>(freq / 10, (uint64_t)((double)left * 1e-9 * freq));
                v = hsa_signal_wait_scacquire(c->sdma.done[b][h], HSA_SIGNAL_CONDITION_LT, 1, hint, HSA_WAIT_STATE_BLOCKED);
                if (v < 1 || std::chrono::steady_clock::now() >= deadline) break;
            }
            if (v >= 1) return false;
        }
        return true;
    };
    hipError_t q = hipSuccess;
    for (;;) {
        if (done_by(std::chrono::steady_clock::now() + period)) {
            c->sdma.pending[b] = false;
            return RT_OK;
        }
        q = hipEventQuery(c->sdma.fired[b]);
        if (q != hipSuccess && q != hipErrorNotReady) break;       // the render stream failed
    }
    (void)hipGetLastError();
    hsa_signal_store_screlease(c->sdma.dep[b], 0);
    for (int h = 0; h < c->sdma.copies[b]; ++h)
        hsa_signal_wait_scacquire(c->sdma.done[b][h], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
    (void)hipStreamSynchronize(c->frames.rs);
    (void)hipGetLastError();
    c->sdma.pending[b] = false;
    return rt_fail(RT_EHIP, std::string("rt_render_packed: the frame's render failed before its SDMA copy: ") +
                                hipGetErrorString(q));
}

void sdma_destroy(rt_ctx* c) {
    if (!c->sdma.ok) return;
    for (int b = 0; b < rt_ctx::kSlots; ++b) {
        (void)sdma_wait(c, b);                         // (the render stream has drained: its signal has fired)
        hsa_signal_destroy(c->sdma.dep[b]);
        hsa_signal_destroy(c->sdma.done[b][0]);
        hsa_signal_destroy(c->sdma.done[b][1]);
        (void)hipEventDestroy(c->sdma.fired[b]);
    }
    hsa_shut_down();
}

// rt_render_packed / rt_render_packed_async: one image in `format`, copied to host memory.
// async: the copy goes to an SDMA engine (or, for pageable memory, the copy kernel on the copy stream; pipelined frames:
// it runs beside the next render), else behind the render on the render stream (see the table at copy_to_host).
static int render_packed_queue(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                               int format, void* host, int slot, bool with_stats, size_t* npx_out, void** sums,
                               bool async) {
    if (!c) return rt_fail(RT_EINVAL, "rt_render_packed: null context");
    if (!host) return rt_fail(RT_EINVAL, "rt_render_packed: null host buffer");
    int pb = 0;
    int rc = rt_pixel_bytes(format, &pb);
    if (rc) return rc;
    rc = rt_set_scene(c, scene);
    if (rc) return rc;
    int nl = 0;
    rc = render_local_rows(c, cam, W, H, depth, nullptr, &nl);
    if (rc) return rc;
    RT_HIP(hipSetDevice(c->device));
    const size_t npx = (size_t)W * H;
    *npx_out = npx;
    void* px = nullptr;
    void* rcb = nullptr;
    // RT_COPY_MODE=2 (A/B): the kernel stores the frame straight into the pinned host buffer (mapped into the
    // device's address space), no device buffer and no copy; 3: an SDMA engine copies it (rt_ctx::Sdma)
    int mode = c->knobs.copy_mode >= 0 ? c->knobs.copy_mode : (async ? 3 : 1);
    // (the engine needs page-locked host memory: pageable buffers take the copy-kernel / hipMemcpyAsync path; it is
    // given the buffer's device-side address, which for memory registered after allocation may differ from `host`)
    void* const hdev = mode == 3 ? host_device_ptr(host, npx * pb) : nullptr;
    if (mode == 3 && (!hdev || !sdma_init(c))) mode = async ? 0 : 1;
    // the slot's device buffer: an SDMA copy of an earlier frame may still read it (whatever this call's mode)
    if ((rc = sdma_wait(c, slot))) return rc;
    c->frames.last_copy_mode = mode;
    void* direct = mode == 2 ? pinned_device_ptr(host, npx * pb) : nullptr;
    if (direct) px = direct;
    else if ((rc = ctx_buffer(c, 5 + slot, npx * pb, &px))) return rc;
    if (with_stats && ((rc = ctx_buffer(c, 3, npx * 4, &rcb)) || (rc = ctx_buffer(c, 4, 16, sums)))) return rc;
    const hipStream_t cs = mode != 0 ? c->frames.rs : c->frames.cs;
    // mode 3: the copy in halves on two engines when two are free (r05, tools/copy_ab.py: 49.3 vs 50.3 us per
    // pipelined c2 GRAY8 frame), each half decrementing sdma.done.  (Rendering a synchronous frame in two row chunks,
    // each copied as soon as it is in its buffer, measured no faster: 83.9 vs 83.1 us — the chunks are two views to
    // the per-view tile-order and cone caches, and each copy's start after its signal costs ~8 us.)
    const size_t nbytes = npx * pb;
    const size_t half = c->sdma.engine2 && c->knobs.sd_split >= 2 && nbytes >= 65536 ? nbytes / 2 & ~(size_t)255 : 0;
    if (mode == 3) {                                    // before the render is queued: it fires sdma.dep
        hsa_signal_store_relaxed(c->sdma.dep[slot], 1);
        hsa_signal_store_relaxed(c->sdma.done[slot][0], 1);
        hsa_signal_store_relaxed(c->sdma.done[slot][1], 1);
    }
    // the slot's device buffer is free once its previous frame's copy has left (ordered by the stream when that
    // copy ran on the render stream)
    if (c->frames.copied_rec[slot] && c->frames.copied_cs[slot])
        RT_HIP(hipStreamWaitEvent(c->frames.rs, c->frames.copied[slot], 0));
    if (with_stats) RT_HIP(hipEventRecord(c->frames.ev0, c->frames.rs));
    const bool f = float_format(format);
    rc = render_dev_impl(c, cam, W, H, depth, nullptr, f ? format : RT_PIXEL_RGBA32F, f ? px : nullptr,
                         f ? RT_PIXEL_RGBA8 : format, f ? nullptr : px, nullptr, (uint32_t*)rcb, c->frames.rs);
    if (rc) return rc;
    if (with_stats) RT_HIP(hipEventRecord(c->frames.ev1, c->frames.rs));
    if (with_stats && (rc = queue_raysum(c, npx, 1, (uint32_t*)rcb, (unsigned long long*)*sums))) return rc;
    if (mode == 3) {
        RT_HIP(sdma_fire(c, slot, c->sdma.writer));      // the frame is in px
        RT_HIP(hipEventRecord(c->sdma.fired[slot], c->frames.rs));
        const hsa_status_t hs = hsa_amd_memory_async_copy_on_engine(
            hdev, c->sdma.cpu, px, c->sdma.gpu, half ? half : nbytes, 1, &c->sdma.dep[slot], c->sdma.done[slot][0],
            (hsa_amd_sdma_engine_id_t)c->sdma.engine, true);
        if (hs != HSA_STATUS_SUCCESS) {
            RT_HIP(hipStreamSynchronize(c->frames.rs));
            return rt_fail(RT_EHIP, "rt_render_packed: hsa_amd_memory_async_copy_on_engine failed");
        }
        c->sdma.pending[slot] = true;                     // (the first copy is queued: its slot must be waited for)
        c->sdma.copies[slot] = 1;
        if (half) {
            const hsa_status_t h2 = hsa_amd_memory_async_copy_on_engine(
                (char*)hdev + half, c->sdma.cpu, (char*)px + half, c->sdma.gpu, nbytes - half, 1, &c->sdma.dep[slot],
                c->sdma.done[slot][1], (hsa_amd_sdma_engine_id_t)c->sdma.engine2, true);
            if (h2 != HSA_STATUS_SUCCESS) {
                (void)sdma_wait(c, slot);
                return rt_fail(RT_EHIP, "rt_render_packed: hsa_amd_memory_async_copy_on_engine failed");
            }
            c->sdma.copies[slot] = 2;
        }
        c->frames.copied_rec[slot] = false;
        return RT_OK;
    }
    if (cs != c->frames.rs) {
        // the copy runs on the copy stream, so it overlaps the next frame's render
        RT_HIP(hipEventRecord(c->frames.rendered[slot], c->frames.rs));
        RT_HIP(hipStreamWaitEvent(cs, c->frames.rendered[slot], 0));
    }
    if (!direct && (rc = copy_to_host(c, host, px, npx * pb, cs, mode == 0 ? kCopyStreamBlocks : 0))) return rc;
    RT_HIP(hipEventRecord(c->frames.copied[slot], cs));
    c->frames.copied_rec[slot] = true;
    c->frames.copied_cs[slot] = cs != c->frames.rs;
    return RT_OK;
}

extern "C" int rt_render_packed(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H, int depth,
                                int format, void* host_pixels, rt_stats* stats) {
    size_t npx = 0;
    void* sums = nullptr;
    if (!c) return rt_fail(RT_EINVAL, "rt_render_packed: null context");
    const uint64_t t = c->frames.ticket + 1;                   // issued only once the frame is queued
    int rc = render_packed_queue(c, scene, cam, W, H, depth, format, host_pixels, (int)(t % rt_ctx::kSlots), stats != nullptr,
                                 &npx, &sums, false);
    if (rc) return rc;
    c->frames.ticket = t;
    if (c->sdma.pending[t % rt_ctx::kSlots]) {
        if ((rc = sdma_wait(c, (int)(t % rt_ctx::kSlots)))) return rc;
    } else {
        RT_HIP(hipEventSynchronize(c->frames.copied[t % rt_ctx::kSlots]));
    }
    if (stats) {
        RT_HIP(hipStreamSynchronize(c->frames.rs));
        return read_stats(c, npx, (const unsigned long long*)sums, stats);
    }
    return RT_OK;
}

extern "C" int rt_render_packed_async(rt_ctx* c, const rt_scene* scene, const rt_camera* cam, int W, int H,
                                      int depth, int format, void* host_pixels, uint64_t* ticket) {
    size_t npx = 0;
    void* sums = nullptr;
    if (!c) return rt_fail(RT_EINVAL, "rt_render_packed_async: null context");
    const uint64_t t = c->frames.ticket + 1;
    int rc = render_packed_queue(c, scene, cam, W, H, depth, format, host_pixels, (int)(t % rt_ctx::kSlots), false, &npx,
                                 &sums, true);
    if (rc) return rc;
    c->frames.ticket = t;
    if (ticket) *ticket = t;
    return RT_OK;
}

extern "C" int rt_ctx_wait(rt_ctx* c, uint64_t ticket) {
    if (!c) return rt_fail(RT_EINVAL, "rt_ctx_wait: null context");
    if (ticket > c->frames.ticket) return rt_fail(RT_EINVAL, "rt_ctx_wait: ticket not issued");
    RT_HIP(hipSetDevice(c->device));
    if (ticket == 0) {                                  // everything queued on the context's streams
        RT_HIP(hipStreamSynchronize(c->frames.rs));
        RT_HIP(hipStreamSynchronize(c->frames.cs));
        for (int b = 0; b < rt_ctx::kSlots; ++b) {
            const int rc = sdma_wait(c, b);
            if (rc) return rc;
        }
        return RT_OK;
    }
    // slot (ticket % kSlots) holds this frame's copy or a later one's (which the GPU orders after it)
    const int sl = (int)(ticket % rt_ctx::kSlots);
    if (c->sdma.pending[sl]) return sdma_wait(c, sl);
    if (c->frames.copied_rec[sl]) RT_HIP(hipEventSynchronize(c->frames.copied[sl]));
    return RT_OK;
}

extern "C" int rt_diag_copy_path(rt_ctx* c, int* mode, int* writer) {
    if (!c) return rt_fail(RT_EINVAL, "rt_diag_copy_path: null context");
    if (mode) *mode = c->frames.last_copy_mode;
    if (writer) *writer = c->sdma.ok ? c->sdma.writer : 0;
    return RT_OK;
}

extern "C" int rt_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return rt_fail(RT_EINVAL, "rt_host_alloc: bad arguments");
    *out = nullptr;
    // RT_HOST_NONCOHERENT=1 (A/B): non-coherent pinned memory (the GPU may cache its writes until the kernel ends)
    const char* nc = getenv("RT_HOST_NONCOHERENT");
    RT_HIP(hipHostMalloc(out, bytes, nc && atoi(nc) ? hipHostMallocNonCoherent : hipHostMallocDefault));
    void* dmap = nullptr;
    if (hipHostGetDevicePointer(&dmap, *out, 0) != hipSuccess || !dmap) dmap = nullptr;
    if (dmap) {                                         // host frames in it are copied by rt_copy_out_kernel
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned[(uintptr_t)*out] = {bytes, (uintptr_t)dmap};
    }
    return RT_OK;
}

extern "C" int rt_host_free(void* p) {
    if (!p) return RT_OK;
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned.erase((uintptr_t)p);
    }
    RT_HIP(hipHostFree(p));
    return RT_OK;
}
