// rt_rays.hip — the ray-list entry points: rt_trace_rays_dev and rt_render_screen's chunks (rt_trace_rays_kernel,
// rt_render.hpp), the primitive intersections of the KATs and the arithmetic probe of include/rt_diag.h.
#include <cstdlib>
#include <string>

#include "../../include/rt_diag.h"
#include "rt_ctx.hpp"
#include "rt_render.hpp"

using namespace rt;

namespace {

using namespace rtk;

__global__ __launch_bounds__(kThreads) void rt_intersect_kernel(const DevScene* __restrict__ S,
                                                                const double* __restrict__ starts,
                                                                const double* __restrict__ ends, int n,
                                                                rt_hit* __restrict__ hits) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    const SceneView V = view_of(S, S, S->n_padded, S->n_stride, S->n_lights);
    Ray r;
    r.p0 = ld3(starts + 3 * k);
    d3 d = sub(ld3(ends + 3 * k), r.p0);
    set_dir(&r, d, unit(d));
    set_origin_f32(S, &r);
    d3 p;
    int kind = closest_hit<true>(V, r, &p);
    rt_hit h;
    h.hit = kind >= 0;
    h.material = -1;
    for (int q = 0; q < 3; ++q) {
        h.point[q] = 0.0; h.normal[q] = 0.0; h.reflected_end[q] = 0.0; h.transmitted_end[q] = 0.0;
    }
    if (kind >= 0) {
        d3 n, pe;
        int mat;
        surface(V, kind, p, r.u, &n, &mat, &pe);
        d3 pt = transmitted_end(V, kind, mat, p, r.u, n);
        h.transmitted_end[0] = pt.x; h.transmitted_end[1] = pt.y; h.transmitted_end[2] = pt.z;
        h.material = mat;
        h.point[0] = p.x; h.point[1] = p.y; h.point[2] = p.z;
        h.normal[0] = n.x; h.normal[1] = n.y; h.normal[2] = n.z;
        h.reflected_end[0] = pe.x; h.reflected_end[1] = pe.y; h.reflected_end[2] = pe.z;
    }
    hits[k] = h;
}

// Diagnostics (include/rt_diag.h): the exact-arithmetic fast paths of rt_device.hpp beside the compiler's
// IEEE sequences, on caller-supplied operands.  op 0: per vector v (3 doubles) -> 9 doubles
// [divs(v, len(v)), len(v), unit(v), |v| from unit(), len_fast(v)]; op 1: per pair (a, b) -> 2 doubles
// [a / b, div_core(a, b, rcp_core(b))].
__global__ __launch_bounds__(kThreads) void rt_probe_math_kernel(int op, const double* __restrict__ in, int n,
                                                                 double* __restrict__ out) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k >= n) return;
    if (op == 1) {                                          // (a, b) -> [a / b, div_core(a, b, rcp_core(b))]
        const double a = in[2 * k], b = in[2 * k + 1];
        out[2 * k] = a / b;
        out[2 * k + 1] = div_core(a, b, rcp_core(b));
        return;
    }
    const d3 v = mk(in[3 * k], in[3 * k + 1], in[3 * k + 2]);
    double* o = out + 9 * (size_t)k;
    const double l0 = len(v);
    const d3 u0 = divs(v, l0);
    double l1;
    const d3 u1 = unit(v, &l1);
    o[0] = u0.x, o[1] = u0.y, o[2] = u0.z, o[3] = l0;
    o[4] = u1.x, o[5] = u1.y, o[6] = u1.z, o[7] = l1;
    o[8] = len_fast(v);
}

}  // namespace

constexpr size_t kScreenLdsMax = 64 * 1024;       // screen chunks: scene record in LDS when it fits beside the slots

static int trace_rays_launch(rt_ctx* c, const double* starts, const double* ends, int n, int depth, double* rgb64f,
                             uint32_t* raycount, hipStream_t st, const ScreenArgs& sa) {
    RT_HIP(hipSetDevice(c->device));
    const dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
    const int v = trace_variant(c->scene.tree, c->scene.transparent);
    const hipError_t e = with_depth(depth, [&](auto B) {
        return launch_trace_rays<decltype(B)::value>(v, grid, st, c->scene.d_scene, starts, ends, n, rgb64f, raycount, sa);
    });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_trace_rays_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_trace_rays_dev(rt_ctx* c, const double* starts, const double* ends, int n, int depth,
                                 double* rgb64f, uint32_t* raycount, void* stream) {
    if (!c || !c->scene.set) return rt_fail(RT_EINVAL, "rt_trace_rays_dev: no context/scene");
    if (n < 0 || (n > 0 && (!starts || !ends))) return rt_fail(RT_EINVAL, "rt_trace_rays_dev: bad rays");
    if (depth < 0 || depth > RT_MAX_DEPTH) return rt_fail(RT_EINVAL, "rt_trace_rays_dev: depth out of range");
    if (n == 0) return RT_OK;
    return trace_rays_launch(c, starts, ends, n, depth, rgb64f, raycount, (hipStream_t)stream, ScreenArgs{});
}

int rt_trace_screen_dev(rt_ctx* c, const double cam[3], const ScreenPix* pix, const int32_t* first, int m,
                        const double* jit, int n, int depth, double* rgb64f, uint32_t* done, uint32_t seq,
                        void* stream) {
    if (!c || !c->scene.set) return rt_fail(RT_EINVAL, "rt_trace_screen_dev: no context/scene");
    if (depth < 0 || depth > RT_MAX_DEPTH) return rt_fail(RT_EINVAL, "rt_trace_screen_dev: depth out of range");
    if (n <= 0 || m <= 0) return RT_OK;
    ScreenArgs sa;
    sa.pix = pix, sa.m = m, sa.first = first, sa.jit = jit, sa.done = done, sa.seq = seq;
    // RT_SCREEN_LDS=0 (A/B): the scene record read from global memory instead of LDS
    static const bool lds = !getenv("RT_SCREEN_LDS") || atoi(getenv("RT_SCREEN_LDS")) != 0;
    const size_t slots = c->scene.tree ? 0 : slot_bytes(depth, c->scene.transparent, kScreenBlock);
    if (lds && c->scene.bytes % 8 == 0 && (size_t)c->scene.bytes + slots <= kScreenLdsMax) sa.scene_lds = c->scene.bytes;
    return trace_rays_launch(c, cam, nullptr, n, depth, rgb64f, nullptr, (hipStream_t)stream, sa);
}

extern "C" int rt_intersect_dev(rt_ctx* c, const double* starts, const double* ends, int n, rt_hit* hits,
                                void* stream) {
    if (!c || !c->scene.set) return rt_fail(RT_EINVAL, "rt_intersect_dev: no context/scene");
    if (n < 0 || (n > 0 && (!starts || !ends || !hits))) return rt_fail(RT_EINVAL, "rt_intersect_dev: bad rays");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    dim3 grid((unsigned)((n + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(rt_intersect_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, c->scene.d_scene, starts, ends,
                       n, hits);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_intersect_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_probe_math_dev(int op, const double* in, int n, double* out, void* stream) {
    if (op != 0 && op != 1) return rt_fail(RT_EINVAL, "rt_probe_math_dev: unknown op");
    if (n < 0 || (n > 0 && (!in || !out))) return rt_fail(RT_EINVAL, "rt_probe_math_dev: bad buffers");
    if (n == 0) return RT_OK;
    hipLaunchKernelGGL(rt_probe_math_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, op, in, n, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_probe_math_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}
