// rt_plain.hip — the plain render path behind rt_render_dev, rt_render_dev_packed and rt_render_ss_dev: one
// render_dev_impl call in eight steps, and the view cache those steps own (rt_ctx::View, rt_ctx::Sync).
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>

#include "rt_ctx.hpp"
#include "rt_render.hpp"

using namespace rt;

namespace {

using namespace rtk;

#if RT_WAVE_TRACE
uint64_t* g_wtrace = nullptr;                  // diagnostic build only (tools/wave_trace.py)
#endif

// Tile-row dispatch order from a calibration render's per-row costs: rows by decreasing cost (ties by
// index), so the longest rows are dispatched first and the cheap ones fill the tail (longest-processing-
// time-first list scheduling).  One workgroup, bitonic sort of (~cost, row) keys in LDS; n <= kOrderMax.
__global__ __launch_bounds__(1024) void rt_order_kernel(const uint32_t* __restrict__ cost, int n,
                                                        int32_t* __restrict__ order) {
    __shared__ uint64_t key[kOrderMax];
    int m = 1;
    while (m < n) m <<= 1;
    for (int k = threadIdx.x; k < m; k += blockDim.x)
        key[k] = k < n ? ((uint64_t)(~cost[k]) << 32) | (uint32_t)k : ~0ull;
    __syncthreads();
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int k = threadIdx.x; k < m; k += blockDim.x) {
                const int o = k ^ stride;
                if (o > k) {
                    const bool up = (k & size) == 0;
                    const uint64_t a = key[k], b = key[o];
                    if ((a > b) == up) { key[k] = b; key[o] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (int k = threadIdx.x; k < n; k += blockDim.x) order[k] = (int32_t)(key[k] & 0xffffffffu);
}

// Per tile row, the sum of its tiles' wave times (the row order's cost); one workgroup per row.
__global__ __launch_bounds__(256) void rt_rowsum_kernel(const uint32_t* __restrict__ tile_cost, int tiles_x,
                                                        uint32_t* __restrict__ row_cost) {
    __shared__ uint32_t part[256];
    uint32_t acc = 0;
    for (int x = threadIdx.x; x < tiles_x; x += 256) acc += tile_cost[(size_t)blockIdx.x * tiles_x + x];
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) row_cost[blockIdx.x] = part[0];
}

__global__ __launch_bounds__(256) void rt_iota_kernel(int32_t* __restrict__ v, int n) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) v[k] = k;
}

// The dispatch table of a calibrated view: position L (linear workgroup id, L = gy * tiles_x + bx) traces tile
// by_pos[L] (tile order: tile indices by decreasing calibrated time) or, row order (by_pos = nullptr), tile column
// bx of tile row row_order[gy]; with the calibration render's per-tile primary cone masks when
// `cone` (else 0), and their sky verdicts (cone[n + tile], n the tile count).  Stored at cone_slot(L): grouped by the
// XCD workgroup L runs on.
// `cls` (or nullptr): the view's tile classes (rt_class_kernel); a sphere-free tile's record carries kDispSphereFree,
// and kDispFlat beside it when `flat` (or nullptr: rt_flat_kernel's verdicts) marks the tile (class_bits).
__device__ __forceinline__ uint32_t class_bits(const uint8_t* __restrict__ cls, const uint8_t* __restrict__ flat, size_t t,
                                               uint32_t sky) {
    return disp_sky_word(sky, cls && cls[t] == kClassSphereFree, flat && flat[t]);   // (sphere-free: sky was 0)
}

__global__ __launch_bounds__(256) void rt_disp_kernel(const int32_t* __restrict__ row_order,
                                                      const int32_t* __restrict__ by_pos,
                                                      const uint64_t* __restrict__ cone,
                                                      const uint8_t* __restrict__ cls,
                                                      const uint8_t* __restrict__ flat, int tiles_x, int tiles_y,
                                                      DispRec* __restrict__ disp) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)tiles_x * tiles_y;
    if (k >= n) return;
    int tx, ty;
    if (by_pos) {
        const int t = by_pos[k];
        ty = t / tiles_x;
        tx = t - ty * tiles_x;
    } else {
        const int gy = (int)(k / tiles_x), bx = (int)(k - (size_t)gy * tiles_x);
        ty = row_order[gy];
        tx = bx;
    }
    const uint64_t m = cone ? cone[(size_t)ty * tiles_x + tx] : 0;
    DispRec r;
    r.cone_lo = (uint32_t)m;
    r.cone_hi = (uint32_t)(m >> 32);
    r.tile = ((uint32_t)ty << 16) | (uint32_t)tx;
    r.sky = cone ? (uint32_t)cone[n + (size_t)ty * tiles_x + tx] : 0;   // (the verdicts follow the n masks)
    r.sky = class_bits(cls, flat, (size_t)ty * tiles_x + tx, r.sky);
    disp[cone_slot(k, n)] = r;
}

// The class of every tile of a fast-kernel view (rt_ctx::View::tile_class), from what its calibration left: the cone
// masks and sky verdicts of the calibration render (cone, then n verdicts) and the `slots` level masks per tile of the
// level-mask launch, whose buffer was zeroed before that launch, so a slot no wave reached reads 0.
__global__ __launch_bounds__(256) void rt_class_kernel(const uint64_t* __restrict__ cone,
                                                       const uint64_t* __restrict__ lmask, int slots, int np, int n,
                                                       uint8_t* __restrict__ cls) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const bool sky = cone[(size_t)n + t] != 0;
    cls[t] = sky ? kClassSky
                 : tile_sphere_free(cone[t], false, lmask + (size_t)t * slots, slots, np) ? kClassSphereFree : kClassTrace;
}

// Which sphere-free tiles of the view are flat (rt_device.hpp trace_flat has the proof this verdict feeds): one wave per
// tile forms the tile's 64 screen points exactly as render_body does — the same clamping of lanes past the frame, the
// same row map, the same screen_point — and evaluates the primary closest hit a sphere-free tile's render evaluates
// (closest_hit_primary<false, NOSPH> with an empty cone mask, lazy_u) on them: flat when every lane returns the board and
// the wave-uniform gates hold.  P is the calibration render's; the per-eye records (board_num, prim_bound_ok) are those
// of its eye, stream-ordered before this launch.  A cached render traces the same rays with the same operations, so the
// verdict is exact for the view.  Tiles of any other class leave 0.
// One 64-thread workgroup per tile of the whole view, most of which leave at the class test: simpler than compacting the
// sphere-free tiles first, and it runs once per calibration.  It is launched under RT_FLAT_TILES=0 and RT_TILE_CLASSES=0
// as well, on purpose: the diagnostics (rt_diag_flat_tiles, tools/wave_trace.py) then name the same tiles on the other
// path, which is what an A/B of the two paths compares.
__global__ __launch_bounds__(64) void rt_flat_kernel(const DevScene* __restrict__ g, RenderParams P,
                                                     const uint8_t* __restrict__ cls, int n,
                                                     uint8_t* __restrict__ flat) {
    const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (t >= n) return;
    bool all = false;
    const d3 eye = ld3(P.eye);
    if (cls[t] == kClassSphereFree && flat_gates(g, eye)) {      // (wave-uniform)
        const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
        const int i = tx * 8 + (lane & 7), lr = ty * kTileH + (lane >> 3);
        const int ic = i < P.width ? i : P.width - 1, lrc = lr < P.local_rows ? lr : P.local_rows - 1;
        const int j = global_row_of(P, lrc);
        const d3 sp = screen_point(P, ic, j, ld3(P.right), ld3(P.upp));
        const SceneView V = view_of(g, g, P.np, P.ns, P.nl);
        Ray r;
        r.p0 = eye;
        r.d = sub(sp, eye);
        d3 hp;
        const int kind = closest_hit_primary<false, true>(V, r, 0, &hp, true);
        all = __ballot(kind == 0) == ~0ull;
    }
    if (lane == 0) flat[t] = all ? 1 : 0;
}

// The run-compacted dispatch table of a calibrated view in tile-row order (include/rt_diag.h; the plain table stays
// beside it for every render that may not read runs).  rt_run_plan_kernel, one workgroup per dispatch row gy: the
// row's verdicts (the calibration render's) in LDS, one byte per tile (tiles_x bytes of dynamic LDS), then the plan
// (rt_cone.hpp sky_run_at) tile by tile, as a code per plain position — 0 covered by the run that starts to its left,
// 1 a tracing tile, 1 + len the head of a run of len sky tiles.  An inclusive prefix sum of (code != 0) then numbers
// the heads (hipcub, render_build_dispatch), and rt_run_disp_kernel writes each head's record at cone_slot(its number,
// the heads' count).
__global__ __launch_bounds__(256) void rt_run_plan_kernel(const int32_t* __restrict__ row_order,
                                                          const uint64_t* __restrict__ sky, int tiles_x, int run_max,
                                                          uint32_t* __restrict__ code) {
    extern __shared__ uint8_t row_sky[];
    const int gy = (int)blockIdx.x;
    const uint64_t* v = sky + (size_t)row_order[gy] * tiles_x;
    for (int x = threadIdx.x; x < tiles_x; x += 256) row_sky[x] = v[x] != 0;
    __syncthreads();
    for (int x = threadIdx.x; x < tiles_x; x += 256)
        code[(size_t)gy * tiles_x + x] =
            (uint32_t)(1 + sky_run_at(tiles_x, run_max, x, [&](int q) { return row_sky[q] != 0; }));
}

struct RunHead {
    __host__ __device__ uint32_t operator()(uint32_t code) const { return code != 0 ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void rt_run_disp_kernel(const int32_t* __restrict__ row_order,
                                                          const uint64_t* __restrict__ cone,
                                                          const uint8_t* __restrict__ cls,
                                                          const uint8_t* __restrict__ flat,
                                                          const uint32_t* __restrict__ code,
                                                          const uint32_t* __restrict__ number, int tiles_x, int tiles_y,
                                                          DispRec* __restrict__ disp) {
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)tiles_x * tiles_y;
    if (k >= n || code[k] == 0) return;
    const int gy = (int)(k / tiles_x), bx = (int)(k - (size_t)gy * tiles_x);
    const int ty = row_order[gy], tx = bx;
    const uint64_t m = cone[(size_t)ty * tiles_x + tx];
    DispRec r;
    r.cone_lo = (uint32_t)m;
    r.cone_hi = (uint32_t)(m >> 32);
    r.tile = ((uint32_t)ty << 16) | (uint32_t)tx;
    r.sky = code[k] - 1u;
    r.sky = class_bits(cls, flat, (size_t)ty * tiles_x + tx, r.sky);   // (a tracing tile: code 1, sky word 0)
    disp[cone_slot(number[k] - 1u, number[n - 1])] = r;   // (number[n - 1]: the heads' count, at most n)
}

// Per-eye primary-ray sphere data (run by rt_render_dev when the camera eye changes): deltaP = C - eye
// and dot(deltaP, deltaP) exactly as Shape::intersection computes them for p0 = camera (:740, :750), and
// the FP32 filter image f32(deltaP), c0 = (r2 - dd) + K (S0^2 + r2) rounded up, S0 = max|deltaP_i|.
// Filter error < 35 eps32 S0^2 + 2 eps32 r2 << K (S0^2 + r2), K = 256 eps32.  Padding spheres have
// r2 = -inf, hence c0 = -inf: always rejected.
__global__ __launch_bounds__(kThreads) void rt_prepare_kernel(DevScene* __restrict__ g, double ex, double ey,
                                                              double ez) {
    const int np = g->n_padded;
    const SceneArrays A = scene_arrays(g);
    const DevSphere* sph = A.sph;
    DevSpherePrim* prim = const_cast<DevSpherePrim*>(A.prim);      // the three per-eye arrays this kernel writes
    DevSpherePrimF* primf = const_cast<DevSpherePrimF*>(A.primf);
    DevSphereCone* cone = const_cast<DevSphereCone*>(A.cone);
    const d3 eye = mk(ex, ey, ez);
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k == 0) {
        g->eye[0] = ex; g->eye[1] = ey; g->eye[2] = ez;
        // board plane numerator for p0 = eye, as board_hit computes it (:657)
        g->board_num = dot(ld3(g->tri[0].n), sub(ld3(g->tri[0].v0), eye));
        g->hits_ok = hits_ok_from(g, eye);      // hit points of rays from this eye skip the cull (hits_inside)
        // A primary ray that hits an object passes g_scene's cull when every object lies within R - 1 of bc
        // (hits_inside) and the eye is at least R + 1 away: the line then passes within R - 1 of bc, so its exact
        // disc >= R^2 - (R - 1)^2 = 2R - 1, and the eye being outside the bound puts the entry root at
        // s >= D - R >= 1 (the hit lies ahead of the eye, past the entry); the FP64 rounding of disc and s is
        // ~2^-49 (D^2 + R^2) and ~2^-50 (D + R), far below 2R - 1 and 1 - eps for D <= 2^20 (R + 1).  (s >= 1 clears the
        // reference's |s| < eps cull only for eps < 1: required explicitly, as hits_inside does through inner2.)
        const double bx = eye.x - g->bc[0], by = eye.y - g->bc[1], bz = eye.z - g->bc[2];
        const double D2 = bx * bx + by * by + bz * bz, R1 = sqrt(g->br2) + 1.0;
        g->prim_bound_ok = (g->bound_on != 0) & (g->hits_inside != 0) & (g->eps < 0.5) &
                           (D2 >= R1 * R1 * (1.0 + 0x1p-30)) & (D2 <= R1 * R1 * 0x1p40);
    }
    // the board's four edges seen from this eye (the wave-level board miss of primary_cone_mask)
    if (k < 4) g->edge[k] = board_edge_record(g, ex, ey, ez, k);
    if (k >= np) return;
    d3 dP = sub(ld3(sph[k].c), eye);
    double dd = dot(dP, dP);
    DevSpherePrim pp;
    pp.dP[0] = dP.x; pp.dP[1] = dP.y; pp.dP[2] = dP.z;
    pp.dd = dd;
    prim[k] = pp;
    double s0 = fmax(fabs(dP.x), fmax(fabs(dP.y), fabs(dP.z)));
    double r2 = sph[k].r2;
    double c0 = (r2 - dd) + (double)kFilterK * (s0 * s0 + r2);
    DevSpherePrimF f;
    f.dx = (float)dP.x; f.dy = (float)dP.y; f.dz = (float)dP.z;
    f.c0 = __double2float_ru(c0);
    primf[k] = f;
    // Cone of directions from the eye that can hit sphere k (primary_cone_mask)
    cone[k] = sphere_cone_record(dP.x, dP.y, dP.z, dd, r2);
}

}  // namespace

#if RT_WAVE_TRACE
extern "C" int rt_debug_wave_trace(void* dev_buf) {
    g_wtrace = reinterpret_cast<uint64_t*>(dev_buf);
    return RT_OK;
}
#endif

// ---- the view cache (rt_ctx::View): only the functions from here to render_record_view write it ------------------------
// Its legal states are the values of View::cal and View::seen (rt_ctx.hpp): "no calibrated view" is cal.reset(), and
// render_build_dispatch alone makes one.  The buffers know their own capacities (DevBuf).
void view_forget(rt_ctx* c) {
    c->view.cal.reset();
    c->view.seen.reset();
}

template <class... B>
static void release_all(B&... b) {
    (b.release(), ...);
}

// The per-tile buffers freed, and with them the view they described.
static void view_release_tiles(rt_ctx::View& v) {
    v.cal.reset();
    release_all(v.disp, v.tile_cost, v.cone_tile, v.tile_class, v.tile_flat, v.sort_keys, v.sort_in, v.sort_out, v.sort_tmp,
                v.disp_run, v.run_code, v.run_num, v.run_tmp);
    v.tiles_cap = 0;
}

int view_create(rt_ctx* c) {
    rt_ctx::View& v = c->view;
    if (!v.tile_rows.reserve(sizeof(int32_t) * kOrderMax) || !v.row_cost.reserve(sizeof(uint32_t) * kOrderMax))
        return RT_ENOMEM;
    if (hipMemset(v.tile_rows.get(), 0, sizeof(int32_t) * kOrderMax) != hipSuccess ||
        hipEventCreateWithFlags(&v.run_ev, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc(&v.h_run_n, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
        return RT_EHIP;
    return RT_OK;
}

void view_release(rt_ctx* c) {
    rt_ctx::View& v = c->view;
    view_release_tiles(v);
    release_all(v.tile_rows, v.row_cost, v.lmask);
    if (v.run_ev) (void)hipEventDestroy(v.run_ev);
    if (v.h_run_n) (void)hipHostFree(v.h_run_n);
}

// The per-tile buffers grown to hold `tiles` tiles (the caller has drained the device: renders may read the old ones).
// False (and no buffers) when the device is out of memory: the view then keeps the identity order.
static bool rt_grow_view_bufs(rt_ctx* c, size_t tiles) {
    rt_ctx::View& v = c->view;
    if (tiles <= v.tiles_cap) return true;
    view_release_tiles(v);
    const size_t slots = cone_slots(tiles);
    size_t tmp = 0;
    const bool ok = v.disp.reserve(slots * sizeof(DispRec)) && v.tile_cost.reserve(tiles * sizeof(uint32_t)) &&
                    v.cone_tile.reserve(2 * tiles * sizeof(uint64_t)) &&   // masks, then sky verdicts
                    v.tile_class.reserve(tiles) && v.tile_flat.reserve(tiles) &&
                    v.sort_keys.reserve(tiles * sizeof(uint32_t)) && v.sort_in.reserve(tiles * sizeof(int32_t)) &&
                    v.sort_out.reserve(tiles * sizeof(int32_t)) &&
                    hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp, v.tile_cost.get(), v.sort_keys.get(),
                                                                 v.sort_in.get(), v.sort_out.get(),
                                                                 (int)tiles) == hipSuccess &&
                    v.sort_tmp.reserve(tmp);
    if (!ok) {
        (void)hipGetLastError();
        view_release_tiles(v);
        return false;
    }
    // the run table's buffers (all or none: without them every render reads the plain table)
    if (c->knobs.sky_run_max != 1) {
        tmp = 0;
        const hipcub::TransformInputIterator<uint32_t, RunHead, const uint32_t*> heads(v.run_code.get(), RunHead{});
        const bool run_ok = v.disp_run.reserve(slots * sizeof(DispRec)) && v.run_code.reserve(tiles * sizeof(uint32_t)) &&
                            v.run_num.reserve(tiles * sizeof(uint32_t)) &&
                            hipcub::DeviceScan::InclusiveSum(nullptr, tmp, heads, v.run_num.get(), (int)tiles) == hipSuccess &&
                            v.run_tmp.reserve(std::max(tmp, (size_t)16));
        if (!run_ok) {
            (void)hipGetLastError();
            release_all(v.disp_run, v.run_code, v.run_num, v.run_tmp);
        }
    }
    v.tiles_cap = tiles;
    return true;
}

static int render_params(const rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows,
                         RenderParams* P) {
    if (!c) return rt_fail(RT_EINVAL, "render: null context");
    if (!c->scene.set) return rt_fail(RT_EINVAL, "render: rt_set_scene has not been called");
    if (!cam) return rt_fail(RT_EINVAL, "render: null camera");
    if (W <= 0 || H <= 0 || (long long)W * H > (1LL << 31)) return rt_fail(RT_EINVAL, "render: bad image size");
    if (depth < 0 || depth > RT_MAX_DEPTH) return rt_fail(RT_EINVAL, "render: depth out of range [0, 7]");
    int nl = 0;
    int rc = rt_local_rows(H, rows, &nl);
    if (rc) return rc;
    memset(P, 0, sizeof(*P));
    double right[3], upp[3];
    rt_camera_basis(cam, right, upp);
    for (int q = 0; q < 3; ++q) {
        P->eye[q] = cam->eye[q];
        P->look[q] = cam->look_at[q];
        P->right[q] = right[q];
        P->upp[q] = upp[q];
    }
    P->pitch = cam->pitch;
    P->bottom_x = cam->bottom_x;
    P->bottom_y = cam->bottom_y;
    P->width = W;
    P->height = H;
    P->local_rows = nl;
    bool banded = rows && rows->n_ranks > 1;
    P->band_height = banded ? rows->band_height : H;
    P->n_ranks = banded ? rows->n_ranks : 1;
    P->rank = banded ? rows->rank : 0;
    P->frames = (rows && rows->frames > 1) ? rows->frames : 1;
    P->frame_rows = nl / P->frames;
    P->lds_bytes = c->scene.lds_bytes;
    P->np = c->scene.n_padded;
    P->ns = c->scene.n_stride;
    P->nl = c->scene.n_lights;
    P->wg_staging = c->knobs.wg_staging;
#if RT_WAVE_TRACE
    P->wtrace = g_wtrace;
#endif
    // FP32 camera for the per-wave cone culling, and the bound on its error (rt_cone.hpp)
    const ConeCam C = cone_camera(P->look, P->right, P->upp, P->eye, P->pitch, P->bottom_x, P->bottom_y, W, H);
    for (int q = 0; q < 3; ++q) {
        P->look32[q] = C.look[q];
        P->right32[q] = C.right[q];
        P->upp32[q] = C.upp[q];
        P->eye32[q] = C.eye[q];
    }
    P->pitch32 = C.pitch;
    P->cone_slack = C.slack;
    P->sky = c->knobs.sky_tiles ? 1 : 0;
    return RT_OK;
}

// render_params' checks alone, and the rows of the frame this process renders (the host-frame calls).
int render_local_rows(const rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows,
                      int* local_rows) {
    RenderParams P;
    const int rc = render_params(c, cam, W, H, depth, rows, &P);
    if (!rc) *local_rows = P.local_rows;
    return rc;
}

static bool byte_format(int f) { return f == RT_PIXEL_RGBA8 || f == RT_PIXEL_RGB8 || f == RT_PIXEL_GRAY8; }

// render_route() (rt_render.hpp) for this context's scene kind and A/B knobs.
static RenderRoute ctx_route(const rt_ctx* c, int depth, int mode, bool level_mask) {
    const rt_ctx::Scene& s = c->scene;
    const rt_ctx::Knobs& k = c->knobs;
    return render_route(RouteScene{s.tree, s.transparent, s.n_padded, s.n_stride, s.achromatic, s.lds_bytes},
                        RouteKnobs{k.use_lds != 0, k.wg_staging != 0, k.min_waves, k.achro_off}, depth, mode, level_mask);
}

// One render_dev_impl call: what it was asked for, and what its steps (below, in the order they run) decide.
struct RenderJob {
    const rt_camera* cam;
    int W, H, depth;
    const rt_rows* rows;
    void *pf, *p8;                                      // the outputs, each nullable
    double* o64;
    uint32_t* orc;
    hipStream_t st;
    int ss_log2;
    RenderParams P;                                     // step 1
    int mode;                                           // kModePlain / kModePacked / kModeSS
    RenderRoute route;                                  // the kernel instance, its LDS bytes and tile width
    int tiles_x, tiles_y;                               // step 2
    size_t tiles;
    bool capturing, cull_kernel;                        // (cull_kernel: the render kernel itself writes the level masks)
    int lm_stride;                                      // level-mask slots per tile (0: none)
    rt_ctx::ViewKey key;
    bool calibrate, cone_calib, lm_calib;               // this render times its tiles / records cone / level masks
    bool prepare;                                       // ... writes the per-eye scene records first
    bool runs;                                          // the launch reads the run-compacted table (c->view.run_*)
};

// The grid of a launch over n dispatch positions of a table of its own width: w positions per grid row, at most kGridY
// rows, so that the rows x w - n padding positions (each traces a clamped tile and stores nothing) number at most 7
// wherever such a width exists in the range searched (w = 8 always is one up to 8 kGridY positions), else the fewest.
static void run_grid(uint32_t n, int* w, int* rows) {
    if (n <= 1024) {
        *w = (int)n;
        *rows = 1;
        return;
    }
    const uint32_t lo = std::max(8u, (n + kGridY - 1) / kGridY);
    uint32_t best = std::max(lo, 1024u), best_pad = ~0u;
    for (uint32_t k = std::max(lo, 1024u); k >= lo; --k) {
        const uint32_t pad = (k - n % k) % k;
        if (pad < best_pad) best = k, best_pad = pad;
        if (pad <= 7) break;
    }
    *w = (int)best;
    *rows = (int)((n + best - 1) / best);
}

// Step 1: the kernel parameters, the pixel formats and the output mode; the kernel instance of the frame.
static int render_job_params(rt_ctx* c, int fmt_f, int fmt_8, RenderJob& J) {
    RenderParams& P = J.P;
    int rc = render_params(c, J.cam, J.W, J.H, J.depth, J.rows, &P);
    if (rc) return rc;
    const bool ss = J.ss_log2 >= 0;
    if (ss) {
        P.ss_log2 = J.ss_log2;
        P.wg_staging = 0;                           // one-wave direct-store instances only
    }
    if ((J.pf && !float_format(fmt_f)) || (J.p8 && !byte_format(fmt_8)))
        return rt_fail(RT_EINVAL, "render: bad pixel format for the float / byte image");
    if (((J.pf && fmt_f == RT_PIXEL_GRAY32F) || (J.p8 && fmt_8 == RT_PIXEL_GRAY8)) && !c->scene.achromatic)
        return rt_fail(RT_EINVAL, "render: GRAY pixel formats need an achromatic scene (rt_scene_achromatic)");
    P.fmt_f = fmt_f == RT_PIXEL_GRAY32F ? kFmtF_GRAY : kFmtF_RGBA;
    P.fmt_8 = fmt_8 == RT_PIXEL_GRAY8 ? kFmt8_GRAY : fmt_8 == RT_PIXEL_RGB8 ? kFmt8_RGB : kFmt8_RGBA;
    const bool packed = (J.pf && P.fmt_f != kFmtF_RGBA) || (J.p8 && P.fmt_8 != kFmt8_RGBA);
    if (packed) P.wg_staging = 0;                   // the LDS-staged stores (A/B variant) write RGBA only
    J.mode = ss ? kModeSS : packed ? kModePacked : kModePlain;
    // One-wave workgroups (8 x 8 tiles) by default: measured faster than 256-thread workgroups (32 x 8
    // tiles) at every config (c2 -1%, c3 -3%, c5 -12%: a finished wave's slot is refilled without
    // waiting for three siblings).  The A/B instances that share a workgroup-wide LDS copy (scene in LDS,
    // staged row stores) keep 256 threads; packed formats and supersampling have one-wave instances only.
    J.route = ctx_route(c, J.depth, J.mode, false);
    return RT_OK;
}

// r06: a moving camera renders in identity order (RT_MOVING_ORDER=1: the last calibrated order, re-timed every
// RT_RECALIBRATE-th render, 8 by default then — the r03-r05 policy).  tools/moving_probe.py, c2 orbit, 3 frames in
// flight: identity 22.8 us per frame, the static view's order kept 24.2, re-timed every 8th render 26.9 (the
// re-timing's order kernels stall the context's stream; the static view's row costs are not the orbit's).
//
// Step 2: the tiles, and which render of its view this is — a later one in calibrated order, one of a moving camera,
// the calibration render, or the first (identity order).
static int render_plan_view(rt_ctx* c, RenderJob& J) {
    rt_ctx::View& v = c->view;
    RenderParams& P = J.P;
    const bool big = J.route.key.WG == kThreads;    // 32 x 8 tiles, four waves each
    J.tiles_x = (J.W + J.route.tile_w - 1) / J.route.tile_w;
    J.tiles_y = (P.local_rows + kTileH - 1) / kTileH;
    J.tiles = (size_t)J.tiles_x * J.tiles_y;
    P.tile_rows_n = J.tiles_y;
    P.tiles_x = J.tiles_x;
    // A render captured into a hipGraph must be self-contained: it always prepares its eye's data and uses
    // the identity tile-row order (the context's order buffer belongs to whatever view it last calibrated).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    RT_HIP(hipStreamIsCapturing(J.st, &cap));
    J.capturing = cap != hipStreamCaptureStatusNone;
    if (J.capturing) c->eye.ever_captured = true;
    J.calibrate = J.cone_calib = J.lm_calib = J.runs = false;
    // level masks per tile (opaque scenes, one-wave tiles): B ray masks + (B + 1) nl shadow masks.  The culling
    // kernels compute them in their calibration render; for the fast kernels' scenes (< kConeMin spheres) a culling
    // kernel writes them in a launch of its own right after the calibration render (no image outputs), and later
    // renders skip the filter batches they rule out
    const bool opaque_tiles = !c->scene.tree && !c->scene.transparent && !big && RT_WG_FAST == 64;
    J.cull_kernel = c->scene.n_padded >= kConeMin && opaque_tiles;
    J.lm_stride = opaque_tiles && c->knobs.level_masks && c->knobs.cone_cache ? J.depth + (J.depth + 1) * c->scene.n_lights : 0;
    if (J.lm_stride > kLevelMaskSlotsMax) J.lm_stride = 0;
    J.key = rt_ctx::ViewKey{};
    // (dispatch records pack the tile as ty << 16 | tx)
    if (!J.capturing && c->knobs.order_mode == 0 && J.tiles_y <= kOrderMax && J.tiles_x < 65536 && J.tiles_y < 65536) {
        // Key of the frame's work: camera, size, outputs, row plan, depth and scene generation.
        unsigned char* kp = J.key.data();               // fixed size: no host allocation per render
        memcpy(kp, J.cam, sizeof(rt_camera)); kp += sizeof(rt_camera);
        // which outputs are written (and in which format) changes the rows' relative cost (an RGB64F parity
        // render writes 24 B per pixel): each output set gets its own calibration
        // (and a supersampled render its own: it shares the camera and size of a plain render of its sample grid,
        // not its stores)
        const int outs = (J.pf ? 1 : 0) | (J.p8 ? 2 : 0) | (J.o64 ? 4 : 0) | (J.orc ? 8 : 0) | (P.fmt_f << 4) |
                         (P.fmt_8 << 6) | ((J.mode == kModeSS ? J.ss_log2 + 1 : 0) << 8);
        const int ints[6] = {J.W, J.H, J.depth, J.tiles_x, J.tiles_y, outs};
        memcpy(kp, ints, sizeof(ints)); kp += sizeof(ints);
        if (J.rows) memcpy(kp, J.rows, sizeof(rt_rows));
        kp += sizeof(rt_rows);
        memcpy(kp, &c->scene.gen, sizeof(uint64_t));
        constexpr size_t kCam = sizeof(rt_camera);
        const bool same_shape = v.cal && memcmp(J.key.data() + kCam, v.cal->key.data() + kCam, J.key.size() - kCam) == 0;
        if (v.cal && J.key == v.cal->key) {
            rt_ctx::View::Calibrated& k = *v.cal;
            using Runs = rt_ctx::View::Runs;
            P.disp = v.disp.get();
            // (the cached masks hold one mask per one-wave 8 x 8 tile: the 256-thread A/B instances never read them)
            P.cone_use = k.cones && !big ? 1 : 0;
            // the run-compacted table of this view, once its position count has arrived (a wait that has, as a rule,
            // long passed: the copy was queued behind the calibration's table kernels)
            if (k.runs == Runs::pending) {
                k.runs = Runs::none;
                if (hipEventSynchronize(v.run_ev) == hipSuccess) {
                    k.run_n = *v.h_run_n;
                    if (k.run_n > 0 && k.run_n < J.tiles) {       // (no sky tile: the plain table)
                        k.runs = Runs::ready;
                        run_grid(k.run_n, &k.run_w, &k.run_rows);
                    }
                } else {
                    (void)hipGetLastError();
                }
            }
            J.runs = k.runs == Runs::ready && P.cone_use && P.sky;
            if (J.runs) P.disp = v.disp_run.get();
            v.last = {J.runs ? (int)k.run_n : (int)J.tiles, (int)J.tiles, J.runs ? k.run_built_max : 1};
            if (J.lm_stride > 0 && k.lmask_stride == J.lm_stride) {   // this view's level masks
                P.lmask_in = v.lmask.get();
                P.lmask_stride = J.lm_stride;
            }
        } else if (same_shape && c->knobs.moving_order) {
            P.disp = v.disp.get();                     // another camera: the last calibrated order, its own masks
            if (c->knobs.recalibrate > 0 && ++v.cal->stale >= c->knobs.recalibrate) {   // ... re-timed every recalibrate-th render
                J.calibrate = true;
                v.cal.reset();                          // (the render still dispatches by the old table, P.disp)
            }
        } else if (v.seen && J.key == *v.seen) {        // (by default a moving camera's views come here: the
                                                        // first render of a view in identity order, its second
                                                        // the calibration — a camera that stops is calibrated)
            J.calibrate = true;                         // calibration render (identity order)
            v.cal.reset();                              // rt_disp_kernel rewrites disp below, and disp_run
            // the calibration records one mask per tile from lane 0 of its wave: one-wave workgroups only
            J.cone_calib = c->knobs.cone_cache && c->scene.n_padded >= kPrimaryConeMin && !c->scene.tree &&
                           !c->scene.transparent && !big && RT_WG_FAST == 64;
            J.lm_calib = J.cone_calib && J.lm_stride > 0;
        } else {
            v.seen = J.key;                            // first render of this view: identity order
        }
    }
    J.prepare = J.capturing || c->eye.ever_captured || !c->eye.valid || memcmp(c->eye.pos, J.cam->eye, sizeof(c->eye.pos)) != 0;
    return RT_OK;
}

// Step 3: order this render against the renders queued on other streams (a captured render carries its own prepare
// launch and touches no view state).
static int render_order_streams(rt_ctx* c, const RenderJob& J) {
    if (J.capturing) return RT_OK;
    // read-after-write / write-after-write: the last write of the view state was queued on another stream
    if (c->sync.view_rec && c->sync.view_st != J.st) RT_HIP(hipStreamWaitEvent(J.st, c->sync.view_ev, 0));
    if (J.prepare || J.calibrate) {
        // write-after-read: renders queued on other streams may still read what this render rewrites (or frees)
        if ((c->sync.readers && (c->sync.readers_multi || c->sync.reader_st != J.st)) ||
            (J.calibrate && J.tiles > c->view.tiles_cap) ||
            (J.lm_calib && J.tiles * (size_t)J.lm_stride * sizeof(uint64_t) > c->view.lmask.bytes))
            RT_HIP(hipDeviceSynchronize());
        c->sync.readers = c->sync.readers_multi = false;      // same-stream renders are ordered before the rewrite
    }
    if (!c->sync.readers) {                              // this render reads the view state on st
        c->sync.readers = true;
        c->sync.reader_st = J.st;
    } else if (c->sync.reader_st != J.st) {
        c->sync.readers_multi = true;
    }
    return RT_OK;
}

// Step 4 (calibration renders): the buffers the render writes every tile's wave time and, a static view's, its cone
// and level masks to.  They grow here: step 3 drained the device.  (Step 2 dropped the calibrated view: nothing describes
// what the buffers hold until step 7.)
static void render_grow_calibration(rt_ctx* c, RenderJob& J) {
    rt_ctx::View& v = c->view;
    RenderParams& P = J.P;
    if (!rt_grow_view_bufs(c, J.tiles)) {           // out of memory: identity order, masks in the kernel
        J.calibrate = J.cone_calib = J.lm_calib = false;
        P.disp = nullptr;
        P.cone_use = 0;
    } else {
        P.tile_cost = v.tile_cost.get();
        if (J.cone_calib) P.cone_out = v.cone_tile.get();
    }
    // (out of memory: the masks stay in the kernel)
    if (J.lm_calib && !v.lmask.reserve(J.tiles * (size_t)J.lm_stride * sizeof(uint64_t))) J.lm_calib = false;
    if (J.lm_calib && J.cull_kernel) {              // (fast scenes: the level-mask launch of step 6 writes them)
        P.lmask_out = v.lmask.get();
        P.lmask_stride = J.lm_stride;
    }
}

// Step 5: the primary-ray sphere data for this eye (stream-ordered; only when the eye changes, or always once graphs
// that carry their own prepare launch exist).
static int render_prepare_eye(rt_ctx* c, const RenderJob& J) {
    c->eye.valid = false;
    dim3 pg((unsigned)((std::max(c->scene.n_padded, 1) + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(rt_prepare_kernel, pg, dim3(kThreads), 0, J.st, c->scene.d_scene, J.cam->eye[0], J.cam->eye[1],
                       J.cam->eye[2]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_prepare_kernel: ") + hipGetErrorString(e));
    memcpy(c->eye.pos, J.cam->eye, sizeof(c->eye.pos));
    c->eye.valid = true;
    return RT_OK;
}

// Step 6: the render, and behind a fast scene's calibration render the launch that writes its level masks.
static int render_launch(rt_ctx* c, const RenderJob& J) {
    RenderLaunch L;
    L.key = J.route.key;
    L.grid = dim3((unsigned)J.tiles_x, (unsigned)std::min(J.tiles_y, kGridY), (unsigned)((J.tiles_y + kGridY - 1) / kGridY));
    L.disp_w = J.tiles_x;
    L.disp_n = J.tiles_y * J.tiles_x;
    if (J.runs) {                                   // one position per tracing tile and per run of sky tiles
        const rt_ctx::View::Calibrated& k = *c->view.cal;
        L.grid = dim3((unsigned)k.run_w, (unsigned)k.run_rows, 1);
        L.disp_w = k.run_w;
        L.disp_n = (int32_t)k.run_n;
    }
    L.lds = (size_t)J.route.lds;
    L.stream = J.st;
    L.scene = c->scene.d_scene;
    L.P = J.P;
    L.o32 = J.pf;
    L.o8 = J.p8;
    L.o64 = J.o64;
    L.orc = J.orc;
    // A level-mask slot is written only where a wave reaches that level: the view's masks start as zeros, on the render
    // stream ahead of the launch that writes them (this one, or the level-mask launch below), so that an unreached slot
    // reads "keeps no sphere" — no render consumes such a slot, and the tile classes (rt_class_kernel) read them all.
    if (J.lm_calib &&
        hipMemsetAsync(c->view.lmask.get(), 0, J.tiles * (size_t)J.lm_stride * sizeof(uint64_t), J.st) != hipSuccess)
        return rt_fail(RT_EHIP, "level masks: hipMemsetAsync failed");
    hipError_t e = with_depth(J.depth, [&](auto B) { return launch_render<decltype(B)::value>(L); });
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("rt_render_kernel launch: ") + hipGetErrorString(e));
    if (J.lm_calib && !J.cull_kernel) {
        // a fast kernel's scene: the level masks of the view from a culling kernel that stores nothing else (identity
        // order, its own primary cone masks, no image) — stream-ordered before the renders that read them
        const RenderRoute mask = ctx_route(c, J.depth, J.mode, true);
        RenderLaunch M = L;
        M.key = mask.key;
        M.lds = (size_t)mask.lds;
        M.P.lmask_out = c->view.lmask.get();
        M.P.lmask_in = nullptr;
        M.P.lmask_stride = J.lm_stride;
        M.P.disp = nullptr;
        M.P.cone_use = 0;
        M.P.cone_out = nullptr;
        M.P.tile_cost = nullptr;
        M.o32 = M.o8 = nullptr;
        M.o64 = nullptr;
        M.orc = nullptr;
        e = with_depth(J.depth, [&](auto B) { return launch_render<decltype(B)::value>(M); });
        if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("level-mask launch: ") + hipGetErrorString(e));
    }
    return RT_OK;
}

// Step 7 (calibration renders): the dispatch table of this view, stream-ordered after the render that wrote the tile
// times; only then does the context call the view calibrated.
static int render_build_dispatch(rt_ctx* c, const RenderJob& J) {
    rt_ctx::View& v = c->view;
    const int tiles = (int)J.tiles, tiles_x = J.tiles_x, tiles_y = J.tiles_y;
    const hipStream_t st = J.st;
    hipError_t e;
    const dim3 tg((unsigned)((J.tiles + 255) / 256));
    rt_ctx::View::Calibrated k;                           // the view these kernels describe: the context's at the end
    k.key = J.key;
    k.tiles = J.tiles;
    k.cones = J.cone_calib;
    k.lmask_stride = J.lm_calib ? J.lm_stride : 0;
    const uint64_t* cones = J.cone_calib ? v.cone_tile.get() : nullptr;
    // The tile classes of a fast-kernel view with level masks, after the level-mask launch and ahead of the table
    // kernels; the records carry them unless RT_TILE_CLASSES=0.  Culling-kernel views and views without masks have none.
    const uint8_t *cls = nullptr, *flat = nullptr;
    if (J.cone_calib && J.lm_calib && !J.cull_kernel && c->scene.n_padded <= 64) {
        hipLaunchKernelGGL(rt_class_kernel, tg, dim3(256), 0, st, v.cone_tile.get(), v.lmask.get(), J.lm_stride,
                           c->scene.n_padded, tiles, v.tile_class.get());
        k.classes = true;
        // (only into the records of a view whose kernel instance reads the bit: rt_render.hpp class_instance)
        if (class_instance(J.mode == kModePacked, J.mode == kModeSS, J.depth)) {
            if (c->knobs.tile_classes) cls = v.tile_class.get();
            // ... and which of the sphere-free tiles are flat, for the same instances: the calibration render's rays,
            // re-formed from its parameters (rt_flat_kernel).  In the records unless RT_FLAT_TILES=0 (or no class is).
            hipLaunchKernelGGL(rt_flat_kernel, dim3((unsigned)tiles), dim3(64), 0, st, c->scene.d_scene, J.P,
                               v.tile_class.get(), tiles, v.tile_flat.get());
            k.flat = true;
            if (cls && c->knobs.flat_tiles) flat = v.tile_flat.get();
        }
    }
    if (c->knobs.order_policy == 1) {                     // tiles longest first
        hipLaunchKernelGGL(rt_iota_kernel, tg, dim3(256), 0, st, v.sort_in.get(), (int)tiles);
        size_t tmp = v.sort_tmp.bytes;
        e = hipcub::DeviceRadixSort::SortPairsDescending(v.sort_tmp.get(), tmp, v.tile_cost.get(), v.sort_keys.get(),
                                                         v.sort_in.get(), v.sort_out.get(), (int)tiles, 0, 32, st);
        if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("tile order sort: ") + hipGetErrorString(e));
        hipLaunchKernelGGL(rt_disp_kernel, tg, dim3(256), 0, st, nullptr, v.sort_out.get(), cones, cls, flat, tiles_x,
                           tiles_y, v.disp.get());
    } else {                                        // tile rows longest first
        hipLaunchKernelGGL(rt_rowsum_kernel, dim3((unsigned)tiles_y), dim3(256), 0, st, v.tile_cost.get(), tiles_x,
                           v.row_cost.get());
        hipLaunchKernelGGL(rt_order_kernel, dim3(1), dim3(1024), 0, st, v.row_cost.get(), tiles_y, v.tile_rows.get());
        hipLaunchKernelGGL(rt_disp_kernel, tg, dim3(256), 0, st, v.tile_rows.get(), nullptr, cones, cls, flat, tiles_x,
                           tiles_y, v.disp.get());
        // ... and beside it the run-compacted table, for the cached renders of a view with sky verdicts whose
        // instance stores runs (render_body: one-wave opaque tiles, which cone_calib implies; not supersampled).  The
        // plan runs along dispatch columns and the kernel stores image columns tx .. tx + r - 1: the same thing because
        // dispatch column bx traces image column bx in every row.
        const int run_max = c->knobs.sky_run_max == 0 ? 65535 : c->knobs.sky_run_max;
        if (J.cone_calib && c->knobs.sky_tiles && run_max > 1 && v.disp_run.get() && J.mode != kModeSS) {
            const hipcub::TransformInputIterator<uint32_t, RunHead, const uint32_t*> heads(v.run_code.get(), RunHead{});
            size_t tmp = v.run_tmp.bytes;
            hipLaunchKernelGGL(rt_run_plan_kernel, dim3((unsigned)tiles_y), dim3(256), (size_t)tiles_x, st,
                               v.tile_rows.get(), v.cone_tile.get() + J.tiles, tiles_x, run_max, v.run_code.get());
            if (hipcub::DeviceScan::InclusiveSum(v.run_tmp.get(), tmp, heads, v.run_num.get(), tiles, st) == hipSuccess) {
                hipLaunchKernelGGL(rt_run_disp_kernel, tg, dim3(256), 0, st, v.tile_rows.get(), v.cone_tile.get(), cls,
                                   flat, v.run_code.get(), v.run_num.get(), tiles_x, tiles_y, v.disp_run.get());
                if (hipMemcpyAsync(v.h_run_n, v.run_num.get() + (J.tiles - 1), sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   st) == hipSuccess &&
                    hipEventRecord(v.run_ev, st) == hipSuccess) {
                    k.runs = rt_ctx::View::Runs::pending;
                    k.run_built_max = run_max;
                }
            }
            if (k.runs != rt_ctx::View::Runs::pending) (void)hipGetLastError();   // (the view keeps the plain table)
        }
    }
    e = hipGetLastError();
    if (e != hipSuccess) return rt_fail(RT_EHIP, std::string("dispatch table: ") + hipGetErrorString(e));
    v.cal = k;                                     // only once the order kernel is queued
    return RT_OK;
}

// Step 8: later renders on other streams wait for this render's writes of the view state.
static int render_record_view(rt_ctx* c, const RenderJob& J) {
    RT_HIP(hipEventRecord(c->sync.view_ev, J.st));
    c->sync.view_st = J.st;
    c->sync.view_rec = true;
    return RT_OK;
}

// The device render behind rt_render_dev / rt_render_dev_packed: the float image (fmt_f) and the byte image
// (fmt_8) in their formats, the FP64 colour and the ray counters, each nullable.
// ss_log2 >= 0 (rt_render_ss_dev): cam, W, H and rows describe the SAMPLE grid of a supersampled render with
// S = 1 << ss_log2 samples per axis; the outputs hold (W / S) x (local rows / S) pixels, RGBA formats, and the ray
// counters are two words per pixel.  Everything per view (order, calibration, cached masks, capture rules) is the
// sample grid's, unchanged; the kernels are the supersampled instances, which differ in their epilogue only.
int render_dev_impl(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows, int fmt_f, void* pf,
                    int fmt_8, void* p8, double* rgb64f, uint32_t* raycount, void* stream, int ss_log2) {
    RenderJob J{cam, W, H, depth, rows, pf, p8, rgb64f, raycount, (hipStream_t)stream, ss_log2};
    int rc = render_job_params(c, fmt_f, fmt_8, J);                             // 1
    if (rc || J.P.local_rows == 0) return rc;
    RT_HIP(hipSetDevice(c->device));
    if ((rc = render_plan_view(c, J))) return rc;                               // 2
    if ((rc = render_order_streams(c, J))) return rc;                           // 3
    if (J.calibrate) render_grow_calibration(c, J);                             // 4
    if (J.prepare && (rc = render_prepare_eye(c, J))) return rc;                // 5
    if ((rc = render_launch(c, J))) return rc;                                  // 6
    if (J.calibrate && (rc = render_build_dispatch(c, J))) return rc;           // 7
    if ((J.prepare || J.calibrate) && !J.capturing) return render_record_view(c, J);   // 8
    return RT_OK;
}

extern "C" int rt_render_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows,
                             float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount, void* stream) {
    return render_dev_impl(c, cam, W, H, depth, rows, RT_PIXEL_RGBA32F, rgba32f, RT_PIXEL_RGBA8, rgba8, rgb64f,
                           raycount, stream);
}

extern "C" int rt_render_dev_packed(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows,
                                    int float_format, void* float_pixels, int byte_format, void* byte_pixels,
                                    void* stream) {
    return render_dev_impl(c, cam, W, H, depth, rows, float_format, float_pixels, byte_format, byte_pixels, nullptr,
                           nullptr, stream);
}


// The front of the sampled _dev entry points: the checks on samples (*s: its log2), context, camera and frame size;
// then, with P given (the list-free kernels of rt_sampled.hpp, which index a whole frame of at most 2^31 pixels), the
// sample-grid camera and the sample grid's RenderParams with ss_log2 set.
int sample_grid_front(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples, int* s,
                      RenderParams* P) {
    *s = ss_log2_of(samples);
    if (*s < 0) return rt_fail(RT_EINVAL, "render: samples must be 1, 2, 4 or 8");
    if (!c) return rt_fail(RT_EINVAL, "render: null context");
    if (!cam) return rt_fail(RT_EINVAL, "render: null camera");
    if (W <= 0 || H <= 0 || (P && (long long)W * H > (1LL << 31)) || (long long)W * samples > INT32_MAX ||
        (long long)H * samples > INT32_MAX)
        return rt_fail(RT_EINVAL, "render: bad image size (width, height)");
    if (!P) return RT_OK;
    rt_camera cam_s;
    int rc = rt_camera_supersample(cam, samples, &cam_s);   // (int32 overflow of the sample-grid camera)
    if (rc) return rc;
    rc = render_params(c, &cam_s, W * samples, H * samples, depth, nullptr, P);   // (at most 2^31 samples)
    if (rc) return rc;
    P->ss_log2 = *s;
    return RT_OK;
}

// rt_render_ss_dev: the render of the sample grid (camera rt_camera_supersample, S W x S H, row bands S times as
// high, so every S-row block of samples stays inside one band) through the supersampled kernel instances.
extern "C" int rt_render_ss_dev(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples,
                                const rt_rows* rows, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                                uint32_t* raycount2, void* stream) {
    int s, rc = sample_grid_front(c, cam, W, H, depth, samples, &s, nullptr);
    if (rc) return rc;
    int nl = 0;
    rc = rt_local_rows(H, rows, &nl);                   // the caller's row plan, checked as given
    if (rc) return rc;
    if (rows && rows->frames > 1 && samples > 1)
        return rt_fail(RT_EINVAL, "rt_render_ss_dev: frames > 1 is not supported with samples > 1");
    // S = 1 without counters is rt_render_dev itself (the two-word counters need the supersampled instances)
    if (s == 0 && !raycount2)
        return render_dev_impl(c, cam, W, H, depth, rows, RT_PIXEL_RGBA32F, rgba32f, RT_PIXEL_RGBA8, rgba8, rgb64f,
                               nullptr, stream);
    rt_camera cam_s;
    rc = rt_camera_supersample(cam, samples, &cam_s);
    if (rc) return rc;
    rt_rows rows_s{};
    if (rows) {
        rows_s = *rows;
        if (rows->n_ranks > 1) {
            if ((long long)rows->band_height * samples > INT32_MAX) return rt_fail(RT_EINVAL, "render: bad band height");
            rows_s.band_height = rows->band_height * samples;
        }
    }
    return render_dev_impl(c, &cam_s, W * samples, H * samples, depth, rows ? &rows_s : nullptr, RT_PIXEL_RGBA32F,
                           rgba32f, RT_PIXEL_RGBA8, rgba8, rgb64f, raycount2, stream, s);
}
