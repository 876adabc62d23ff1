// rt_diag.hip — the view diagnostics of include/rt_diag.h: what the view cache of rt_plain.hip holds, and which
// kernel instance a render launches.
#include <cstring>
#include <vector>

#include "../../include/rt_diag.h"
#include "rt_ctx.hpp"
#include "rt_render.hpp"

using namespace rt;
using namespace rtk;

// Diagnostics (include/rt_diag.h): tile-row dispatch order of later renders: 0 adaptive (default), 1
// bottom-to-top.
extern "C" int rt_diag_tile_order(rt_ctx* c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return rt_fail(RT_EINVAL, "rt_diag_tile_order: bad args");
    c->knobs.order_mode = mode;
    view_forget(c);                             // the next two renders calibrate afresh
    return RT_OK;
}

// Diagnostics (include/rt_diag.h): the sky verdicts the waves of the context's last calibration render reached (and
// every cached render of that view reads from its dispatch records), counted on the host.
extern "C" int rt_diag_sky_count(rt_ctx* c, int* tiles, int* sky) {
    if (!c || !tiles || !sky) return rt_fail(RT_EINVAL, "rt_diag_sky_count: bad args");
    *tiles = *sky = 0;
    const rt_ctx::View::Calibrated* k = view_with_cones(c);
    if (!k) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipDeviceSynchronize());
    std::vector<uint64_t> v(k->tiles);          // (the verdicts follow the view's cone masks)
    RT_HIP(hipMemcpy(v.data(), c->view.cone_tile.get() + k->tiles, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    int n = 0;
    for (uint64_t x : v) n += x != 0;
    *tiles = (int)v.size();
    *sky = n;
    return RT_OK;
}

// Diagnostics (include/rt_diag.h): the tile classes the last calibration decided (rt_plain.hip rt_class_kernel), copied
// out and counted on the host.  grid (or nullptr): n bytes for the view's n tiles.
static int tile_classes(rt_ctx* c, uint8_t* grid, size_t n, bool sized, int* tiles, int* sky, int* sphere_free) {
    *tiles = *sky = *sphere_free = 0;
    const rt_ctx::View::Calibrated* k = view_with_cones(c);
    const size_t have = k && k->classes ? k->tiles : 0;
    if (sized && n != have) return rt_fail(RT_EINVAL, "rt_diag_tile_class_grid: n is not the calibrated view's tile count");
    if (have == 0) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipDeviceSynchronize());
    std::vector<uint8_t> v(have);
    RT_HIP(hipMemcpy(v.data(), c->view.tile_class.get(), have, hipMemcpyDeviceToHost));
    for (uint8_t x : v) {
        *sky += x == kClassSky;
        *sphere_free += x == kClassSphereFree;
    }
    *tiles = (int)have;
    if (grid) memcpy(grid, v.data(), have);
    return RT_OK;
}

extern "C" int rt_diag_tile_classes(rt_ctx* c, int* tiles, int* sky, int* sphere_free) {
    if (!c || !tiles || !sky || !sphere_free) return rt_fail(RT_EINVAL, "rt_diag_tile_classes: bad args");
    return tile_classes(c, nullptr, 0, false, tiles, sky, sphere_free);
}

extern "C" int rt_diag_tile_class_grid(rt_ctx* c, uint8_t* out, size_t n) {
    if (!c || !out) return rt_fail(RT_EINVAL, "rt_diag_tile_class_grid: bad args");
    int tiles, sky, sphere_free;
    return tile_classes(c, out, n, true, &tiles, &sky, &sphere_free);
}

// Diagnostics (include/rt_diag.h): the flat verdicts the last calibration decided (rt_plain.hip rt_flat_kernel), copied
// out and counted on the host.  grid (or nullptr): n bytes for the view's n tiles.
static int flat_tiles(rt_ctx* c, uint8_t* grid, size_t n, bool sized, int* tiles, int* flat) {
    *tiles = *flat = 0;
    const rt_ctx::View::Calibrated* k = view_with_cones(c);
    const size_t have = k && k->flat ? k->tiles : 0;
    if (sized && n != have) return rt_fail(RT_EINVAL, "rt_diag_flat_tile_grid: n is not the calibrated view's tile count");
    if (have == 0) return RT_OK;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipDeviceSynchronize());
    std::vector<uint8_t> v(have);
    RT_HIP(hipMemcpy(v.data(), c->view.tile_flat.get(), have, hipMemcpyDeviceToHost));
    for (uint8_t x : v) *flat += x != 0;
    *tiles = (int)have;
    if (grid) memcpy(grid, v.data(), have);
    return RT_OK;
}

extern "C" int rt_diag_flat_tiles(rt_ctx* c, int* tiles, int* flat) {
    if (!c || !tiles || !flat) return rt_fail(RT_EINVAL, "rt_diag_flat_tiles: bad args");
    return flat_tiles(c, nullptr, 0, false, tiles, flat);
}

extern "C" int rt_diag_flat_tile_grid(rt_ctx* c, uint8_t* out, size_t n) {
    if (!c || !out) return rt_fail(RT_EINVAL, "rt_diag_flat_tile_grid: bad args");
    int tiles, flat;
    return flat_tiles(c, out, n, true, &tiles, &flat);
}

// Diagnostics (include/rt_diag.h): the dispatch positions of the last cached render of the calibrated view.
extern "C" int rt_diag_disp_count(rt_ctx* c, int* positions, int* tiles, int* run_max) {
    if (!c || !positions || !tiles || !run_max) return rt_fail(RT_EINVAL, "rt_diag_disp_count: bad args");
    *positions = c->view.last.positions;
    *tiles = c->view.last.tiles;
    *run_max = c->view.last.run_max;
    return RT_OK;
}

// Diagnostics (include/rt_diag.h): render_route() itself, no context and no device.  out: the key's fields in
// RenderKey's order, the launch's LDS bytes, the tile width.
extern "C" int rt_diag_render_route(int tree, int transparent, int n_padded, int n_stride, int achromatic,
                                    int lds_bytes, int use_lds, int wg_staging, int min_waves, int achro_off, int depth,
                                    int mode, int level_mask, int out[13]) {
    if (depth < 0 || depth > RT_MAX_DEPTH || mode < kModePlain || mode > kModeSS || n_padded < 0 || !out)
        return rt_fail(RT_EINVAL, "rt_diag_render_route: bad arguments");
    const RenderRoute r = render_route(RouteScene{tree != 0, transparent != 0, n_padded, n_stride, achromatic != 0, lds_bytes},
                                       RouteKnobs{use_lds != 0, wg_staging != 0, min_waves, achro_off != 0}, depth, mode,
                                       level_mask != 0);
    const RenderKey& k = r.key;
    const int v[13] = {k.kernel, k.LDS, k.MINW, k.TRANSP, k.CULL, k.WG, k.TREE, k.PACKED, k.FIX64, k.ACHRO, k.SS, r.lds,
                       r.tile_w};
    memcpy(out, v, sizeof(v));
    if (!with_depth(depth, [&](auto B) { return render_kernel_ptr<decltype(B)::value>(k); }))
        return rt_fail(RT_EINVAL, "rt_diag_render_route: no such instance");
    return RT_OK;
}

// The instance a render at the default knobs launches for `depth` and the scene kind `variant` of rt_diag_kernel_*
// (0 spheres + board, 1 a culling scene of stride kCullStride, 2 meshes / transparency, 3 ray trees, 4 / 5 the
// achromatic instances of 0 / 1), or nullptr: the build has none.
static const void* diag_kernel(int depth, int variant) {
    const int np = variant == 1 || variant == 5 ? kCullStride : kChunk;
    const RouteScene s{variant == 3, variant == 2, np, sphere_stride(np), variant >= 4, 0};
    const RenderKey k = render_route(s, RouteKnobs{false, false, 5, false}, depth, kModePlain, false).key;
    if (variant >= 4 && !k.ACHRO) return nullptr;   // (deeper than RT_ACHRO_MAX_B: three channels)
    return with_depth(depth, [&](auto B) { return render_kernel_ptr<decltype(B)::value>(k); });
}

// Diagnostics (include/rt_diag.h): registers and scratch of that instance — the tests assert the default instances
// never spill.
extern "C" int rt_diag_kernel_resources(int depth, int variant, int* vgprs, int* scratch_bytes) {
    if (depth < 0 || depth > RT_MAX_B || variant < 0 || variant > 5 || !vgprs || !scratch_bytes)
        return rt_fail(RT_EINVAL, "rt_diag_kernel_resources: bad arguments");
    const void* f = diag_kernel(depth, variant);
    if (!f) return rt_fail(RT_EINVAL, "rt_diag_kernel_resources: kernel not built");
    hipFuncAttributes a;
    RT_HIP(hipFuncGetAttributes(&a, f));
    *vgprs = a.numRegs;
    *scratch_bytes = (int)a.localSizeBytes;
    return RT_OK;
}

// Workgroups of the render kernel (depth, variant as above) the runtime places per CU with `lds_bytes` of
// dynamic LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor).
extern "C" int rt_diag_kernel_occupancy(int depth, int variant, int lds_bytes, int* blocks_per_cu) {
    if (depth < 0 || depth > RT_MAX_B || variant < 0 || variant > 5 || lds_bytes < 0 || !blocks_per_cu)
        return rt_fail(RT_EINVAL, "rt_diag_kernel_occupancy: bad arguments");
    const void* f = diag_kernel(depth, variant);
    if (!f) return rt_fail(RT_EINVAL, "rt_diag_kernel_occupancy: kernel not built");
    RT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, f, RT_WG_FAST, (size_t)lds_bytes));
    return RT_OK;
}
