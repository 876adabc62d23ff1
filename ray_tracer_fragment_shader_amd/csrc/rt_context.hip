// rt_context.hip — the context's lifetime, its A/B knobs, and the scene and motion upload (include/rt_api.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_ctx.hpp"
#include "rt_device.hpp"

using namespace rt;

namespace {

using namespace rtk;

// Eye-independent reciprocals of the division shortcuts (run by rt_set_scene): rcp_core of the checker
// square and of every triangle's den, with the compiler's own Newton steps (rt_device.hpp div_core).
__global__ __launch_bounds__(kThreads) void rt_scene_init_kernel(DevScene* __restrict__ g) {
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k == 0) g->rsquare = rcp_core(g->square);
    if (k < 2) g->tri[k].rden = g->tri[k].fast ? rcp_core(g->tri[k].den) : 0.0;
    const SceneArrays A = scene_arrays(g);
    if (k < g->n_tris) {
        DevTri* t = const_cast<DevTri*>(A.tri) + k;          // (this kernel writes the triangles)
        t->rden = t->fast ? rcp_core(t->den) : 0.0;
    }
}

}  // namespace

#if RT_COUNTERS
// Diagnostic build only (tools/counters.py): point the uploaded scene's event counters at `dev_buf`
// (kCntCount uint64 on the context's device); call after rt_set_scene.
extern "C" int rt_debug_counters(rt_ctx* c, void* dev_buf) {
    if (!c || !c->scene.set) return rt_fail(RT_EINVAL, "rt_debug_counters: no scene");
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipMemcpy(&c->scene.d_scene->counters, &dev_buf, sizeof(dev_buf), hipMemcpyHostToDevice));
    return RT_OK;
}
#endif

extern "C" int rt_device_count(int* count) {
    if (!count) return rt_fail(RT_EINVAL, "rt_device_count: null pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return rt_fail(RT_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return RT_OK;
}

extern "C" int rt_ctx_destroy(rt_ctx* c) {
    if (!c) return RT_OK;
    (void)hipSetDevice(c->device);
    rt_screen_release(c);
    if (c->frames.rs) (void)hipStreamSynchronize(c->frames.rs);
    if (c->frames.cs) (void)hipStreamSynchronize(c->frames.cs);
    if (c->scene.d_scene) (void)hipFree(c->scene.d_scene);
    if (c->scene.d_motion) (void)hipFree(c->scene.d_motion);
    if (c->windows.d_table) (void)hipFree(c->windows.d_table);
    view_release(c);
    sdma_destroy(c);
    if (c->frames.ev0) (void)hipEventDestroy(c->frames.ev0);
    if (c->frames.ev1) (void)hipEventDestroy(c->frames.ev1);
    if (c->sync.view_ev) (void)hipEventDestroy(c->sync.view_ev);
    for (int b = 0; b < rt_ctx::kSlots; ++b) {
        if (c->frames.rendered[b]) (void)hipEventDestroy(c->frames.rendered[b]);
        if (c->frames.copied[b]) (void)hipEventDestroy(c->frames.copied[b]);
    }
    if (c->frames.rs) (void)hipStreamDestroy(c->frames.rs);
    if (c->frames.cs) (void)hipStreamDestroy(c->frames.cs);
    for (void* p : c->frames.d_out)
        if (p) (void)hipFree(p);
    delete c;
    return RT_OK;
}

// The A/B knobs of a new context: every RT_* environment variable a context reads, its clamp and (rt_ctx::Knobs) its
// default.
static void knobs_from_env(rt_ctx::Knobs& k) {
    if (const char* e = getenv("RT_SCENE_IN_LDS")) k.use_lds = atoi(e) != 0;
    if (const char* e = getenv("RT_MIN_WAVES")) k.min_waves = atoi(e);
    if (const char* e = getenv("RT_WG_STAGING")) k.wg_staging = atoi(e) != 0;
    if (const char* e = getenv("RT_TILE_ORDER")) k.order_mode = atoi(e) == 1 ? 1 : 0;   // 1: bottom-to-top (A/B)
    if (const char* e = getenv("RT_COPY_MODE")) k.copy_mode = std::min(std::max(atoi(e), -1), 3);
    if (const char* e = getenv("RT_SDMA_SPLIT")) k.sd_split = std::min(std::max(atoi(e), 1), 2);
    if (const char* e = getenv("RT_SDMA_WRITER")) k.sd_writer_req = std::min(std::max(atoi(e), 0), 2);
    if (const char* e = getenv("RT_SDMA_WAIT_MS")) k.sd_wait_ms = std::max(atoi(e), 0);
    if (const char* e = getenv("RT_MOVING_ORDER")) k.moving_order = atoi(e) != 0;
    if (const char* e = getenv("RT_RECALIBRATE")) k.recalibrate = std::max(atoi(e), 0);
    if (const char* e = getenv("RT_COPY_BLOCKS")) k.copy_blocks = std::max(atoi(e), 0);
    if (const char* e = getenv("RT_COPY_KERNEL")) k.copy_kernel = std::min(std::max(atoi(e), -1), 1);
    if (const char* e = getenv("RT_CONE_CACHE")) k.cone_cache = atoi(e) != 0;
    if (const char* e = getenv("RT_LEVEL_MASKS")) k.level_masks = atoi(e) != 0;
    if (const char* e = getenv("RT_SKY_TILES")) k.sky_tiles = atoi(e) != 0;
    if (const char* e = getenv("RT_SKY_RUN_MAX")) k.sky_run_max = std::min(std::max(atoi(e), 0), 65535);   // 0: whole streaks
    if (const char* e = getenv("RT_TILE_CLASSES")) k.tile_classes = atoi(e) != 0;
    if (const char* e = getenv("RT_FLAT_TILES")) k.flat_tiles = atoi(e) != 0;
    if (const char* e = getenv("RT_ORDER_POLICY")) k.order_policy = std::min(std::max(atoi(e), 0), 1);
    if (const char* e = getenv("RT_ACHRO_OFF")) k.achro_off = atoi(e) != 0;
    if (const char* e = getenv("RT_ACCUM_MAX_PASSES")) k.accum_max_passes = std::min(std::max(atoi(e), 1), 65536);
    if (const char* e = getenv("RT_WINDOW_GRID_X")) k.window_grid_x = std::min(std::max(atoi(e), 1), 1 << 20);
}

extern "C" int rt_ctx_create(int device, rt_ctx** out) {
    if (!out) return rt_fail(RT_EINVAL, "rt_ctx_create: null out");
    *out = nullptr;
    int n = 0;
    int rc = rt_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n) return rt_fail(RT_EHIP, "rt_ctx_create: no HIP device " + std::to_string(device));
    RT_HIP(hipSetDevice(device));
    rt_ctx* c = new rt_ctx();
    c->device = device;
    knobs_from_env(c->knobs);
    if ((rc = view_create(c))) {
        rt_ctx_destroy(c);
        return rt_fail(rc, rc == RT_ENOMEM ? "rt_ctx_create: hipMalloc of the tile-row order failed"
                                           : "rt_ctx_create: stream/event creation failed");
    }
    bool ok = hipEventCreate(&c->frames.ev0) == hipSuccess && hipEventCreate(&c->frames.ev1) == hipSuccess &&
              hipEventCreateWithFlags(&c->sync.view_ev, hipEventDisableTiming) == hipSuccess &&
              hipStreamCreateWithFlags(&c->frames.rs, hipStreamDefault) == hipSuccess &&
              hipStreamCreateWithFlags(&c->frames.cs, hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; b < rt_ctx::kSlots && ok; ++b)
        ok = hipEventCreateWithFlags(&c->frames.rendered[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&c->frames.copied[b], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        rt_ctx_destroy(c);
        return rt_fail(RT_EHIP, "rt_ctx_create: stream/event creation failed");
    }
    *out = c;
    return RT_OK;
}

int rt_ctx_device(const rt_ctx* c) { return c ? c->device : -1; }

int rt_ctx_achromatic(const rt_ctx* c) { return c && c->scene.set && c->scene.achromatic ? 1 : 0; }

void rt_ctx_scene_id(const rt_ctx* c, uint64_t* gen, uint64_t* fingerprint) {
    *gen = c && c->scene.set ? c->scene.gen : 0;
    *fingerprint = c && c->scene.set ? c->scene.hash : 0;
}

// Builds the motion record of the uploaded scene for the displacements `disp` (3 per sphere) and uploads it.  The
// record changes, so work in flight on the device is waited for first (rt_set_scene's ordering rule).
static int motion_upload(rt_ctx* c, std::vector<double> disp) {
    std::vector<unsigned char> rec;
    const int n = (int)(c->scene.local_c.size() / 3);
    int rc = rt_build_motion(c->scene.blob, c->scene.local_c.data(), disp.data(), n, &rec);
    if (rc) return rc;
    RT_HIP(hipSetDevice(c->device));
    RT_HIP(hipDeviceSynchronize());
    if (rec.size() > c->scene.motion_cap) {
        if (c->scene.d_motion) RT_HIP(hipFree(c->scene.d_motion));
        c->scene.d_motion = nullptr;
        c->scene.motion_cap = 0;
        if (hipMalloc(&c->scene.d_motion, rec.size()) != hipSuccess)
            return rt_fail(RT_ENOMEM, "rt_set_motion: hipMalloc failed");
        c->scene.motion_cap = rec.size();
    }
    RT_HIP(hipMemcpy(c->scene.d_motion, rec.data(), rec.size(), hipMemcpyHostToDevice));
    c->scene.disp.swap(disp);
    return RT_OK;
}

static std::vector<double> scene_local_centres(const rt_scene* scene) {
    std::vector<double> v((size_t)3 * (size_t)scene->n_spheres);
    for (int k = 0; k < scene->n_spheres; ++k)
        for (int q = 0; q < 3; ++q) v[3 * k + q] = scene->spheres[k].center[q];
    return v;
}

extern "C" int rt_set_scene(rt_ctx* c, const rt_scene* scene) {
    if (!c) return rt_fail(RT_EINVAL, "rt_set_scene: null context");
    std::vector<unsigned char> blob;
    int rc = rt_build_dev_scene(scene, &blob);
    if (rc) return rc;
    // An unchanged scene (same flattened record, byte for byte) keeps the device copy, the per-eye data
    // and the tile-row order: rt_render calls this every frame.
    if (c->scene.set && blob == c->scene.blob) {
        // (the motion record is built from the scene-local centres: other centres that round to the same world centres
        // are a changed scene to it, and clear the motion as one)
        std::vector<double> lc = scene_local_centres(scene);
        if (memcmp(lc.data(), c->scene.local_c.data(), lc.size() * sizeof(double)) == 0) return RT_OK;
        c->scene.local_c.swap(lc);
        return motion_upload(c, std::vector<double>(c->scene.local_c.size(), 0.0));
    }
    int achromatic = 0;
    rc = rt_scene_achromatic(scene, &achromatic);
    if (rc) return rc;
    RT_HIP(hipSetDevice(c->device));
    // Renders still in flight on any stream of this device read d_scene: wait for them before it changes.
    RT_HIP(hipDeviceSynchronize());
    c->scene.set = false;
    if (blob.size() > c->scene.cap) {
        if (c->scene.d_scene) RT_HIP(hipFree(c->scene.d_scene));
        c->scene.d_scene = nullptr;
        c->scene.cap = 0;
        if (hipMalloc(&c->scene.d_scene, blob.size()) != hipSuccess)
            return rt_fail(RT_ENOMEM, "rt_set_scene: hipMalloc failed");
        c->scene.cap = blob.size();
    }
    RT_HIP(hipMemcpy(c->scene.d_scene, blob.data(), blob.size(), hipMemcpyHostToDevice));
    c->scene.bytes = (int)blob.size();
    const rt::DevScene* h = reinterpret_cast<const rt::DevScene*>(blob.data());
    hipLaunchKernelGGL(rt_scene_init_kernel, dim3((unsigned)((std::max(h->n_tris, 2) + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, nullptr, c->scene.d_scene);
    RT_HIP(hipGetLastError());
    RT_HIP(hipDeviceSynchronize());
    c->scene.lds_bytes = h->lds_bytes;
    c->scene.n_padded = h->n_padded;
    c->scene.n_stride = h->n_stride;
    c->scene.n_lights = h->n_lights;
    c->scene.transparent = h->transparent != 0 || h->n_meshes > 0;   // FULL kernel variants
    c->scene.tree = h->tree != 0;
    c->scene.achromatic = achromatic != 0;
    c->eye.valid = false;
    c->scene.set = true;
    c->scene.blob.swap(blob);
    c->scene.hash = rt_blob_fingerprint(c->scene.blob);
    ++c->scene.gen;
    c->scene.local_c = scene_local_centres(scene);
    return motion_upload(c, std::vector<double>(c->scene.local_c.size(), 0.0));   // a changed scene clears the motion
}

// ---- motion of the spheres (include/rt_api.h, ABI 10: new symbols only) ------------------------------------------
extern "C" int rt_set_motion(rt_ctx* c, const double* displacement, int n_spheres) {
    if (!c) return rt_fail(RT_EINVAL, "rt_set_motion: null context");
    if (!c->scene.set) return rt_fail(RT_EINVAL, "rt_set_motion: no scene set");
    const int n = (int)(c->scene.local_c.size() / 3);
    std::vector<double> disp(c->scene.local_c.size(), 0.0);
    if (displacement || n_spheres != 0) {                   // (NULL, 0) clears the motion
        if (!displacement) return rt_fail(RT_EINVAL, "rt_set_motion: null displacement");
        if (n_spheres != n) return rt_fail(RT_EINVAL, "rt_set_motion: n_spheres is not the uploaded scene's");
        for (size_t k = 0; k < disp.size(); ++k) {
            if (!std::isfinite(displacement[k])) return rt_fail(RT_EINVAL, "rt_set_motion: displacement must be finite");
            disp[k] = displacement[k];
        }
    }
    if (c->scene.d_motion && memcmp(disp.data(), c->scene.disp.data(), disp.size() * sizeof(double)) == 0) return RT_OK;
    return motion_upload(c, std::move(disp));
}

// ---- the list of windows (include/rt_api.h, ABI 10: new symbols only) ---------------------------------------------
// The table is built on the host (rt_group_plan.cpp rt_build_window_table, after rt_window_list_plan's checks) and
// uploaded whole into an allocation of its own; the old table is freed only once the new one holds the list, so a call
// that fails at any step — the checks, the allocation, the copy — leaves the previous list in force.
extern "C" int rt_set_windows(rt_ctx* c, int W, int H, const rt_window* wins, int n, int layout) {
    if (!c) return rt_fail(RT_EINVAL, "rt_set_windows: null context");
    RT_HIP(hipSetDevice(c->device));
    if (!wins && n == 0) {                                  // (NULL, 0) clears the list; the table's memory is kept
        RT_HIP(hipDeviceSynchronize());
        c->windows.set = false;
        c->windows.list.clear();
        c->windows.offset.clear();
        return RT_OK;
    }
    // The list in force again (it was valid when it was set) keeps the device copy and costs no check: the host
    // conveniences call this for every render.  The strides are the layout's, not the caller's.
    if (c->windows.set && wins && W == c->windows.width && H == c->windows.height && layout == c->windows.layout &&
        n >= 1 && (size_t)n == c->windows.list.size()) {
        bool same = true;
        for (int k = 0; k < n && same; ++k) {
            const rt_window& o = c->windows.list[k];
            same = wins[k].x0 == o.x0 && wins[k].y0 == o.y0 && wins[k].width == o.width && wins[k].height == o.height;
        }
        if (same) return RT_OK;
    }
    std::vector<unsigned char> table;
    std::vector<rt_window> list;
    uint32_t tiles[4];
    uint64_t elements = 0;
    const int rc = rt_build_window_table(W, H, wins, n, layout, &table, &list, tiles, &elements);
    if (rc) return rc;
    // Renders still in flight on any stream of this device read the old table: wait for them before it is freed.
    RT_HIP(hipDeviceSynchronize());
    unsigned char* d = nullptr;
    if (hipMalloc(&d, table.size()) != hipSuccess) return rt_fail(RT_ENOMEM, "rt_set_windows: hipMalloc failed");
    const hipError_t e_copy = hipMemcpy(d, table.data(), table.size(), hipMemcpyHostToDevice);
    if (e_copy != hipSuccess) {
        (void)hipFree(d);
        return rt_fail(RT_EHIP, std::string("rt_set_windows: ") + hipGetErrorString(e_copy));
    }
    if (c->windows.d_table) (void)hipFree(c->windows.d_table);
    c->windows.d_table = d;
    c->windows.cap = table.size();
    c->windows.width = W;
    c->windows.height = H;
    c->windows.layout = layout;
    c->windows.list.swap(list);
    c->windows.offset.resize((size_t)n);
    const rt::DevWindow* e = reinterpret_cast<const rt::DevWindow*>(table.data() + rt::window_entries_at(n));
    for (int k = 0; k < n; ++k) c->windows.offset[k] = e[k].base + ((int64_t)e[k].y0 * e[k].stride + e[k].x0);
    for (int s = 0; s < 4; ++s) c->windows.tiles[s] = tiles[s];
    c->windows.elements = elements;
    c->windows.set = true;
    return RT_OK;
}
