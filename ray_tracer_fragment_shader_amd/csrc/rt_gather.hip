// rt_gather.hip — multi-GPU: the gathered row bands of rt_render_multi back in image order, packed wire pixels
// expanded to RGBA (include/rt_api.h rt_unshuffle_dev, rt_unpack_dev).  Stateless: no context.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/rt_api.h"
#include "rt_internal.hpp"

namespace {

using namespace rtk;

// Row of the gathered buffer that holds image row j: rank = band % n_ranks, local row within its slab.  Rank 0's
// rows come from src0 when given (the group's root does not send its own slab to itself).
__device__ __forceinline__ const uint8_t* gathered_row(const uint8_t* src, const uint8_t* src0, int j, int band_height,
                                                       int n_ranks, int slab_rows, size_t row_bytes) {
    const int band = j / band_height;
    const int rank = band % n_ranks;
    const int lr = (band / n_ranks) * band_height + (j - band * band_height);
    return (rank == 0 && src0) ? src0 + (size_t)lr * row_bytes : src + ((size_t)rank * slab_rows + lr) * row_bytes;
}

// One workgroup per image row; copies the row from its rank's slab, 16 bytes per work-item step when rows are
// 16-byte multiples (RGBA8 rows of W % 4 == 0, every RGBA32F row), else 4.
template <int VEC>
__global__ __launch_bounds__(kThreads) void rt_unshuffle_kernel(const uint32_t* __restrict__ src,
                                                                const uint32_t* __restrict__ src0,
                                                                uint32_t* __restrict__ dst, int row_words,
                                                                int height, int band_height, int n_ranks,
                                                                int slab_rows) {
    const int j = blockIdx.x;
    if (j >= height) return;
    const uint32_t* s = reinterpret_cast<const uint32_t*>(
        gathered_row(reinterpret_cast<const uint8_t*>(src), reinterpret_cast<const uint8_t*>(src0), j, band_height,
                     n_ranks, slab_rows, (size_t)row_words * 4));
    uint32_t* d = dst + (size_t)j * row_words;
    if (VEC == 4) {
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
        uint4* d4 = reinterpret_cast<uint4*>(d);
        for (int w = threadIdx.x; w < (row_words >> 2); w += kThreads) d4[w] = s4[w];
    } else {
        for (int w = threadIdx.x; w < row_words; w += kThreads) d[w] = s[w];
    }
}

// Unshuffle + expand packed rows into RGBA images (the wire formats of rt_render_multi, include/rt_api.h):
//   kUnpackGray8: GRAY8 -> RGBA8 (g, g, g, 255);  kUnpackRgb8: RGB8 -> RGBA8 (r, g, b, 255);
//   kUnpackGray32f: GRAY32F -> RGBA32F (v, v, v, 1).
// Exact: the render kernel writes these very bytes into the RGBA images (achromatic scenes: R = G = B bit for
// bit).  VEC (16-byte aligned buffers, W % 4 == 0): 4 — 4 pixels per work-item step, 16-byte stores; 16 — a byte
// wire format: the same 16-byte stores, four steps per lane unrolled with their loads issued first, so a
// 4K row is one round trip per lane instead of four dependent ones (DESIGN §7 has the times).
constexpr int kUnpackGray8 = 0, kUnpackRgb8 = 1, kUnpackGray32f = 2;
__device__ __forceinline__ uint4 gray4_rgba(uint32_t g) {
    uint4 o;
    o.x = (g & 0xffu) * 0x010101u | 0xff000000u;
    o.y = ((g >> 8) & 0xffu) * 0x010101u | 0xff000000u;
    o.z = ((g >> 16) & 0xffu) * 0x010101u | 0xff000000u;
    o.w = (g >> 24) * 0x010101u | 0xff000000u;
    return o;
}
// three little-endian words r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 -> four RGBA8 pixels
__device__ __forceinline__ uint4 rgb4_rgba(uint32_t a, uint32_t b, uint32_t c) {
    uint4 o;
    o.x = (a & 0xffffffu) | 0xff000000u;
    o.y = (a >> 24) | ((b & 0xffffu) << 8) | 0xff000000u;
    o.z = (b >> 16) | ((c & 0xffu) << 16) | 0xff000000u;
    o.w = (c >> 8) | 0xff000000u;
    return o;
}
template <int MODE, int VEC>
__global__ __launch_bounds__(kThreads) void rt_unpack_kernel(const uint8_t* __restrict__ src,
                                                             const uint8_t* __restrict__ src0,
                                                             uint8_t* __restrict__ dst, int W, int height,
                                                             int band_height, int n_ranks, int slab_rows) {
    const int j = blockIdx.x;
    if (j >= height) return;
    constexpr size_t in_px = MODE == kUnpackGray8 ? 1 : MODE == kUnpackRgb8 ? 3 : 4;
    constexpr size_t out_px = MODE == kUnpackGray32f ? 16 : 4;
    const uint8_t* s = gathered_row(src, src0, j, band_height, n_ranks, slab_rows, (size_t)W * in_px);
    uint8_t* d = dst + (size_t)j * W * out_px;
    if (VEC == 16 && MODE != kUnpackGray32f) {
        // four 4-pixel quads per lane, kThreads apart (every load and store instruction covers a contiguous run of the
        // row), the four loads issued before the first store
        const int groups = W >> 2;
        uint4* d4 = reinterpret_cast<uint4*>(d);
        for (int q0 = threadIdx.x; q0 < groups; q0 += 4 * kThreads) {
            uint32_t a[4], b[4], c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * kThreads;
                if (q < groups) {
                    if (MODE == kUnpackGray8) {
                        a[u] = reinterpret_cast<const uint32_t*>(s)[q];
                    } else {
                        const uint32_t* s3 = reinterpret_cast<const uint32_t*>(s) + 3 * q;
                        a[u] = s3[0];
                        b[u] = s3[1];
                        c[u] = s3[2];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u * kThreads;
                if (q < groups) d4[q] = MODE == kUnpackGray8 ? gray4_rgba(a[u]) : rgb4_rgba(a[u], b[u], c[u]);
            }
        }
        return;
    }
    if (VEC) {
        const int groups = W >> 2;
        for (int q = threadIdx.x; q < groups; q += kThreads) {
            if (MODE == kUnpackGray8) {
                reinterpret_cast<uint4*>(d)[q] = gray4_rgba(reinterpret_cast<const uint32_t*>(s)[q]);
            } else if (MODE == kUnpackRgb8) {
                const uint32_t* s3 = reinterpret_cast<const uint32_t*>(s) + 3 * q;
                reinterpret_cast<uint4*>(d)[q] = rgb4_rgba(s3[0], s3[1], s3[2]);
            } else {
                const float4 v = reinterpret_cast<const float4*>(s)[q];
                float4* o = reinterpret_cast<float4*>(d) + 4 * q;
                o[0] = make_float4(v.x, v.x, v.x, 1.0f);
                o[1] = make_float4(v.y, v.y, v.y, 1.0f);
                o[2] = make_float4(v.z, v.z, v.z, 1.0f);
                o[3] = make_float4(v.w, v.w, v.w, 1.0f);
            }
        }
        return;
    }
    for (int x = threadIdx.x; x < W; x += kThreads) {
        if (MODE == kUnpackGray8) {
            const uint8_t g = s[x];
            d[4 * x] = g; d[4 * x + 1] = g; d[4 * x + 2] = g; d[4 * x + 3] = 255;
        } else if (MODE == kUnpackRgb8) {
            d[4 * x] = s[3 * x]; d[4 * x + 1] = s[3 * x + 1]; d[4 * x + 2] = s[3 * x + 2]; d[4 * x + 3] = 255;
        } else {
            float v;
            memcpy(&v, s + 4 * (size_t)x, 4);
            const float4 o = make_float4(v, v, v, 1.0f);
            memcpy(d + 16 * (size_t)x, &o, 16);
        }
    }
}

}  // namespace

static int check_band_geometry(const char* who, const void* gathered, const void* image, int W, int H,
                               int band_height, int n_ranks, int slab_rows) {
    if (!gathered || !image) return rt_fail(RT_EINVAL, std::string(who) + ": null buffer");
    if (W <= 0 || H <= 0 || band_height <= 0 || n_ranks <= 0 || slab_rows < 0)
        return rt_fail(RT_EINVAL, std::string(who) + ": bad geometry");
    rt_rows r = {band_height, n_ranks, 0, 0};
    for (int q = 0; q < n_ranks; ++q) {
        int nl = 0;
        r.rank = q;
        rt_local_rows(H, &r, &nl);
        if (nl > slab_rows) return rt_fail(RT_EINVAL, std::string(who) + ": slab_rows smaller than a rank's rows");
    }
    return RT_OK;
}

int rt_unshuffle_dev_ex(const void* gathered, const void* rank0_slab, void* image, int W, int H, int elem_bytes,
                        int band_height, int n_ranks, int slab_rows, void* stream) {
    int rc = check_band_geometry("rt_unshuffle_dev", gathered, image, W, H, band_height, n_ranks, slab_rows);
    if (rc) return rc;
    if (elem_bytes <= 0 || ((long long)W * elem_bytes) % 4 != 0)
        return rt_fail(RT_EINVAL, "rt_unshuffle_dev: row bytes must be a multiple of 4");
    const int row_words = (int)(((long long)W * elem_bytes) / 4);
    const bool vec = row_words % 4 == 0 && ((uintptr_t)gathered | (uintptr_t)rank0_slab | (uintptr_t)image) % 16 == 0;
    auto k = vec ? rt_unshuffle_kernel<4> : rt_unshuffle_kernel<1>;
    hipLaunchKernelGGL(k, dim3((unsigned)H), dim3(kThreads), 0, (hipStream_t)stream, (const uint32_t*)gathered,
                       (const uint32_t*)rank0_slab, (uint32_t*)image, row_words, H, band_height, n_ranks, slab_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_unshuffle_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_unshuffle_dev(const void* gathered, void* image, int W, int H, int elem_bytes, int band_height,
                                int n_ranks, int slab_rows, void* stream) {
    return rt_unshuffle_dev_ex(gathered, nullptr, image, W, H, elem_bytes, band_height, n_ranks, slab_rows, stream);
}

// RT_UNPACK_VEC4=1 (A/B): the 4-pixel steps for byte formats too (r05's kernel)
static const bool g_unpack_vec4 = [] {
    const char* e = getenv("RT_UNPACK_VEC4");
    return e && atoi(e) != 0;
}();

int rt_unpack_dev_ex(const void* gathered, const void* rank0_slab, void* image, int W, int H, int src_format,
                     int dst_format, int band_height, int n_ranks, int slab_rows, void* stream) {
    int sb = 0, db = 0;
    int rc = rt_pixel_bytes(src_format, &sb);
    if (!rc) rc = rt_pixel_bytes(dst_format, &db);
    if (rc) return rc;
    if (src_format == dst_format)
        return rt_unshuffle_dev_ex(gathered, rank0_slab, image, W, H, sb, band_height, n_ranks, slab_rows, stream);
    rc = check_band_geometry("rt_unpack_dev", gathered, image, W, H, band_height, n_ranks, slab_rows);
    if (rc) return rc;
    int mode;
    if (src_format == RT_PIXEL_GRAY8 && dst_format == RT_PIXEL_RGBA8) mode = kUnpackGray8;
    else if (src_format == RT_PIXEL_RGB8 && dst_format == RT_PIXEL_RGBA8) mode = kUnpackRgb8;
    else if (src_format == RT_PIXEL_GRAY32F && dst_format == RT_PIXEL_RGBA32F) mode = kUnpackGray32f;
    else return rt_fail(RT_EINVAL, "rt_unpack_dev: unsupported format pair");
    const bool al16 = ((uintptr_t)gathered | (uintptr_t)rank0_slab | (uintptr_t)image) % 16 == 0;
    const int vec = !al16 || W % 4 != 0 ? 0 : mode != kUnpackGray32f && !g_unpack_vec4 ? 16 : 4;
    const uint8_t* g = (const uint8_t*)gathered;
    const uint8_t* g0 = (const uint8_t*)rank0_slab;
    uint8_t* im = (uint8_t*)image;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)H), blk(kThreads);
#define RT_UNPACK(M, V) hipLaunchKernelGGL((rt_unpack_kernel<M, V>), grid, blk, 0, st, g, g0, im, W, H, band_height, \
                                           n_ranks, slab_rows)
    if (mode == kUnpackGray8) {
        if (vec == 16) RT_UNPACK(kUnpackGray8, 16); else if (vec) RT_UNPACK(kUnpackGray8, 4); else RT_UNPACK(kUnpackGray8, 0);
    } else if (mode == kUnpackRgb8) {
        if (vec == 16) RT_UNPACK(kUnpackRgb8, 16); else if (vec) RT_UNPACK(kUnpackRgb8, 4); else RT_UNPACK(kUnpackRgb8, 0);
    } else {
        if (vec) RT_UNPACK(kUnpackGray32f, 4); else RT_UNPACK(kUnpackGray32f, 0);
    }
#undef RT_UNPACK
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_unpack_kernel: ") + hipGetErrorString(e));
    return RT_OK;
}

extern "C" int rt_unpack_dev(const void* gathered, void* image, int W, int H, int src_format, int dst_format,
                             int band_height, int n_ranks, int slab_rows, void* stream) {
    return rt_unpack_dev_ex(gathered, nullptr, image, W, H, src_format, dst_format, band_height, n_ranks, slab_rows,
                            stream);
}
