// rt_ctx.hpp — the context behind the C ABI's rt_ctx handle, for the device-side units only (not part of the ABI;
// rt_host.cpp, rt_screen.cpp and rt_group.cpp see the context through the accessors of rt_internal.hpp).
//
// Which unit holds what (the render, ray-list and sampled kernels are templates in rt_render.hpp and rt_sampled.hpp,
// instantiated per depth in rt_render_b<B>.hip, rt_adaptive.hip, rt_lens.hip and rt_lens_adaptive.hip):
//   rt_context.hip  the context's lifetime, its A/B knobs, scene and motion upload (rt_scene_init_kernel)
//   rt_plain.hip    the plain render path, render_dev_impl and its eight steps, and the view cache it owns: the
//                   dispatch-table kernels (rt_order / rowsum / iota / disp / run_plan / run_disp), rt_prepare_kernel
//   rt_diag.hip     the view diagnostics of include/rt_diag.h
//   rt_sampled.hip  adaptive supersampling (rt_classify_kernel), the lens family's device entry points, the
//                   adaptive lens render's, and the accumulating and converging renders' with their windowed forms
//                   (kernels: rt_accum.hip, rt_converge.hip, rt_accum_window.hip, rt_converge_window.hip)
//   rt_frames.hip   every call that renders into host memory: the context's device buffers, the ray sums, the packed
//                   and asynchronous frames, the pinned-memory registry, the copy kernel and the SDMA path
//   rt_rays.hip     the ray-list entry points (rt_intersect_kernel, rt_probe_math_kernel)
//   rt_gather.hip   multi-GPU: gathered row bands -> image order (rt_unshuffle_kernel, rt_unpack_kernel); no context
//
// The two records the kernels read — the scene record d_scene and the motion record d_motion — are built on the host
// (rt_host.cpp rt_build_dev_scene, rt_build_motion) and laid out by rt_layout.hpp alone: every unit above takes their
// array pointers from its scene_arrays() / motion_arrays() (the kernels through rt_device.hpp view_of).
//
// Each member struct of rt_ctx is written by one unit (named beside it); rt_context.hip creates and destroys them all.
#pragma once

#include <hip/hip_runtime.h>
#include <hsa/hsa.h>                           // the types of rt_ctx::Sdma only (the calls: rt_frames.hip)

#include <array>
#include <optional>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "rt_internal.hpp"

namespace rtk {
struct DispRec;                                // rt_render.hpp
struct RenderParams;
}  // namespace rtk

constexpr int kOrderMax = 8192;                // tile rows rt_order_kernel sorts (one workgroup, keys in LDS)
constexpr int kRecalibrate = 8;                // renders of a moving camera per re-timing of the tile rows
constexpr int kAccumMaxPasses = 4;             // passes per rt_accum_kernel launch (rt_ctx::Knobs::accum_max_passes)
constexpr uint8_t kClassTrace = 0, kClassSky = 1, kClassSphereFree = 2;   // rt_ctx::View::tile_class

// A grow-only device buffer.  reserve: room for `n` bytes, by free-then-malloc when it is too small (the caller orders
// that against the work that reads it); false, and an empty buffer, when the device is out of memory.  No destructor:
// the owner releases it with its device set.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t bytes = 0;
    bool reserve(size_t n) {
        if (n <= bytes) return true;
        release();
        if (hipMalloc(&p, n) == hipSuccess) return bytes = n, true;
        (void)hipGetLastError();
        p = nullptr;
        return false;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    T* get() const { return p; }
};

struct rt_ctx {
    int device = 0;

    // The uploaded scene (rt_context.hip).
    struct Scene {
        rt::DevScene* d_scene = nullptr;
        size_t cap = 0;
        int bytes = 0;
        int lds_bytes = 0;
        int n_padded = 0;
        int n_stride = 0;
        int n_lights = 0;
        bool set = false;
        bool transparent = false;              // some material is transparent: TRANSP kernel variants
        bool tree = false;                     // some material transmits and reflects: TREE kernel variants
        bool achromatic = false;               // R = G = B everywhere (rt_scene_achromatic): GRAY formats allowed
        std::vector<unsigned char> blob;       // host image of d_scene (rt_set_scene skips an unchanged scene)
        uint64_t gen = 0;
        uint64_t hash = 0;                     // FNV-1a of `blob` (rt_ctx_scene_id)
        // Motion blur (rt_set_motion, rt_render_motion_dev): the record d_motion (rt_layout.hpp motion_arrays) always
        // describes the uploaded scene — rt_set_scene builds it with no motion — from the scene-local centres the scene
        // was set with.
        rt::DevMotion* d_motion = nullptr;
        size_t motion_cap = 0;
        std::vector<double> local_c;           // rt_sphere::center of the uploaded scene, 3 per sphere
        std::vector<double> disp;              // the displacements in force, 3 per sphere (all 0: no motion)
    } scene;

    // The list of windows in force (rt_set_windows, rt_context.hip; read by rt_sampled.hip's list renders and
    // rt_frames.hip's host entry points).  rt_set_scene and rt_set_motion do not touch it.
    struct Windows {
        bool set = false;
        int width = 0, height = 0, layout = 0;  // the frame the list is of; RT_WINDOWS_IN_PLACE / RT_WINDOWS_PACKED
        std::vector<rt_window> list;            // the windows, each with its layout's stride
        std::vector<int64_t> offset;            // the element of each window's pixel (0, 0) (rt_window_list_plan)
        uint32_t tiles[4] = {0, 0, 0, 0};       // the launch's tile count at S = 1, 2, 4, 8
        uint64_t elements = 0;                  // per-pixel elements of a buffer (rt_window_list_plan)
        unsigned char* d_table = nullptr;       // rt_layout.hpp: four prefix columns, then the DevWindow entries
        size_t cap = 0;
    } windows;

    // The A/B knobs rt_ctx_create reads from the environment (rt_context.hip knobs_from_env; the measurements behind a
    // default stand where the knob is read).  Only order_mode changes later (rt_diag_tile_order).
    struct Knobs {
        int min_waves = 5;                     // >= 5: the launch bounds of depth <= 3, fast_min_waves / cull_min_waves (faster
                                               // than no bound: tools/ab.py); RT_MIN_WAVES=0 disables
        int use_lds = 0;                       // RT_SCENE_IN_LDS=1: header + exact records in LDS (A/B: tools/ab.py)
        int wg_staging = 0;                    // RT_WG_STAGING=1: LDS-staged 32-pixel row stores (A/B)
        // Where the packed host frames' device-to-host copy runs (rt_frames.hip render_packed_queue): RT_COPY_MODE
        // (1: rs, 0: cs, 2: the kernel stores straight into the pinned buffer, 3: SDMA), RT_COPY_KERNEL
        // (0: hipMemcpyAsync) and RT_COPY_BLOCKS override (A/B; -1 / 0: the defaults).
        int copy_mode = -1;
        int copy_kernel = -1;
        int copy_blocks = 0;                   // RT_COPY_BLOCKS: workgroups of the copy kernel (0: the defaults)
        int order_policy = 0;                  // RT_ORDER_POLICY: 0 tile rows longest first (r01-r04), 1 tiles longest first
        int order_mode = 0;                    // RT_TILE_ORDER, rt_diag_tile_order: 0 adaptive, 1 bottom-to-top
        int moving_order = 0;                  // RT_MOVING_ORDER=1: a moving camera keeps the last calibrated order ...
        int recalibrate = kRecalibrate;        // ... re-timed every RT_RECALIBRATE-th render (rt_plain.hip render_plan_view)
        int cone_cache = 1;                    // RT_CONE_CACHE=0: always compute the masks in the kernel (A/B)
        bool level_masks = true;               // RT_LEVEL_MASKS=0: the level masks computed in every render
        // Sky tiles (rt_render.hpp render_body): waves whose primary rays provably all miss store the miss constants
        // without tracing.  RT_SKY_TILES=0: every wave traces (A/B; the images are the same bytes).
        bool sky_tiles = true;
        int sky_run_max = 16;                  // RT_SKY_RUN_MAX: adjacent sky tiles per run (1: no run table, 0: whole streaks)
        // Sphere-free tiles (rt_cone.hpp tile_sphere_free): a fast-kernel view's calibration marks them in its dispatch
        // records and cached renders trace them without the sphere code.  RT_TILE_CLASSES=0: no record is marked (A/B;
        // the images are the same bytes).
        bool tile_classes = true;
        // Flat tiles (rt_device.hpp trace_flat): the sphere-free tiles all of whose primary rays hit the board, which
        // cached renders trace on the straight-line path.  RT_FLAT_TILES=0: no record is marked flat (A/B; the images
        // are the same bytes); RT_TILE_CLASSES=0 implies it.
        bool flat_tiles = true;
        bool achro_off = false;                // RT_ACHRO_OFF=1: the three-channel kernels for achromatic scenes (A/B)
        int sd_split = 2;                      // RT_SDMA_SPLIT: engines a frame's copy is split over (1, 2)
        int sd_writer_req = 0;                 // RT_SDMA_WRITER (A/B): 1 or 2 forces the writer, 0 tries 2 then 1
        int sd_wait_ms = 5000;                 // RT_SDMA_WAIT_MS: how often sdma_wait re-checks a slow render
        // RT_ACCUM_MAX_PASSES: the most passes one rt_accum_kernel launch runs (rt_sampled.hip accum_render_dev splits a
        // call; the images are the same bytes under every value).  A launch holds the CUs until its last pass is done, so
        // on a GPU shared with other work it should stay in the low milliseconds: a pass of the measured workload (c2
        // 1920 x 1080, depth 1, crane, one moving sphere, J = 16) takes 0.89 ms at S = 4 inside the loop, a launch of
        // kAccumMaxPasses = 4 of them 3.58 ms (profiles/accum/bench_accum.json; 0.89 ms at S = 2, 0.23 ms at S = 1; S = 8,
        // four times the rays, not measured).  A larger value saves little more: per launch the split costs one read
        // and one write of the sums (48 bytes per pixel).  Other scenes, depths and motions: not measured.
        int accum_max_passes = kAccumMaxPasses;
        // RT_WINDOW_GRID_X: the most tiles one row of the list kernels' grid holds (rt_sampled.hpp window_list_grid: a
        // list of more tiles folds into grid.y, the last row padded with waves that store nothing).  The images are the
        // same bytes under every value; the tests set a small one to run the fold on a small frame.  1 .. 2^20; a launch
        // has at most 65535 rows, so a list of more than 65535 times this many tiles gets longer rows than asked for
        // (rt_sampled.hip window_list_params).
        int window_grid_x = 1 << 20;
    } knobs;

    // The eye the per-eye records inside d_scene were prepared for (rt_plain.hip; rt_set_scene clears `valid`).
    struct Eye {
        double pos[3] = {0, 0, 0};
        bool valid = false;                    // the device *Prim arrays hold data for `pos`
        bool ever_captured = false;            // a render was captured into a hipGraph: replays may rewrite
                                               // the per-eye data, so every later render re-prepares it
    } eye;

    // The view cache (rt_plain.hip alone writes it; rt_diag.hip reads it).
    // Adaptive tile-row order (rt_order_kernel): the first render of a new (scene, camera, size, rows,
    // depth, outputs) view uses the identity order; the second render of the same view is a calibration
    // render that also times its tile rows; later renders dispatch the rows by decreasing time.  A render
    // of another camera with the same frame shape (size, rows, depth, outputs, scene) reuses the last
    // calibrated order and every kRecalibrate-th such render re-times the rows under it when RT_MOVING_ORDER=1; by
    // default (r06) it renders in identity order.  Any order is a permutation of the tile rows: images never depend
    // on it.
    using ViewKey = std::array<unsigned char, sizeof(rt_camera) + 6 * sizeof(int) + sizeof(rt_rows) + sizeof(uint64_t)>;
    struct View {
        // What the buffers below hold of the ONE calibrated view, `cal`.  No value: there is none, and a render takes
        // the identity order and computes its masks in the kernel.  A calibration render drops it when it starts
        // (render_plan_view) and render_build_dispatch assigns the next one once its table kernels are queued;
        // rt_diag_tile_order drops it too (view_forget).  Only cached renders — renders of exactly `key` — read the
        // masks, the classes and the run table; the diagnostics describe it.
        enum class Runs { none, pending, ready };
        struct Calibrated {
            ViewKey key{};
            size_t tiles = 0;
            // Primary cone masks (scenes with >= kPrimaryConeMin spheres, one-wave 8 x 8 tiles only): the calibration
            // render wrote each tile's mask and, behind the `tiles` masks, its sky verdict to cone_tile, and
            // rt_disp_kernel put both into the records of disp; cached renders read them instead of recomputing them.
            bool cones = false;
            // The culling kernels' level masks in lmask, this many per tile (rt_device.hpp LevelMasks; 0: none).  A
            // cached render reads them only when its own stride is this one.
            int lmask_stride = 0;
            // tile_class holds the view's tile classes (rt_class_kernel: a fast-kernel view with level masks), which
            // the table kernels put into the records unless RT_TILE_CLASSES=0; tile_flat holds which sphere-free tiles
            // are flat (rt_flat_kernel: such a view whose kernel instance reads the bit; in the records unless
            // RT_FLAT_TILES=0 or RT_TILE_CLASSES=0).  rt_diag_tile_classes and rt_diag_flat_tiles read the two arrays.
            bool classes = false, flat = false;
            // Runs of sky tiles (rt_run_plan_kernel): beside disp the calibration of a view in tile-row order builds
            // disp_run, one position per run of up to Knobs::sky_run_max adjacent sky tiles.  Its position count reaches
            // the host without a stall of the calibrating call: a copy into the pinned word h_run_n queued behind the
            // table kernels, then run_ev (pending); the next cached render waits for run_ev (long passed, as a rule) and
            // reads the count: ready, with run_n positions, run_w per grid row, or none (a failed wait, no sky tile).
            Runs runs = Runs::none;
            uint32_t run_n = 0;
            int run_w = 0, run_rows = 0;
            int run_built_max = 1;                 // the run maximum disp_run was built with
            int stale = 0;                         // renders of other cameras since (RT_MOVING_ORDER=1)
        };
        std::optional<Calibrated> cal;
        std::optional<ViewKey> seen;               // the last view rendered once in identity order: its next render calibrates
        struct Last {                              // the last cached render, whatever happened since (rt_diag_disp_count)
            int positions = 0, tiles = 0, run_max = 0;
        } last;

        // The buffers, grouped as they grow (view_create, view_release, rt_grow_view_bufs).  Ordering against renders on
        // other streams: rt_ctx::Sync.
        // kOrderMax entries each, created with the context: the row order (tile rows by decreasing calibrated time) and
        // the rows' times (rt_rowsum_kernel).
        DevBuf<int32_t> tile_rows;
        DevBuf<uint32_t> row_cost;
        // Per tile, all grown together to `tiles_cap` tiles: the view's dispatch table (rt_disp_kernel), the calibration
        // render's wave times, its cone masks and sky verdicts (2 per tile), the class and flat bytes, and the tile
        // order's radix-sort buffers.
        size_t tiles_cap = 0;
        DevBuf<rtk::DispRec> disp;
        DevBuf<uint32_t> tile_cost, sort_keys;
        DevBuf<uint64_t> cone_tile;
        DevBuf<uint8_t> tile_class, tile_flat;
        DevBuf<int32_t> sort_in, sort_out;
        DevBuf<void> sort_tmp;
        // ... and the run table's, all or none (without them every render reads the plain table): the table, the
        // per-position codes, their prefix sum (hipcub, run_tmp).
        DevBuf<rtk::DispRec> disp_run;
        DevBuf<uint32_t> run_code, run_num;
        DevBuf<void> run_tmp;
        DevBuf<uint64_t> lmask;                    // the level masks, a capacity of their own
        uint32_t* h_run_n = nullptr;               // pinned: the run table's position count
        hipEvent_t run_ev = nullptr;               // ... is in h_run_n
    } view;

    // Cross-stream ordering of the per-view state (rt_plain.hip render_order_streams, render_record_view): the per-eye
    // records inside d_scene (rt_prepare_kernel) and the view's buffers (View::row_cost, tile_rows, tile_cost,
    // cone_tile, disp, ...).  Every render reads the per-eye records; a render that prepares a new eye or calibrates
    // also writes.  A writer records view_ev on its stream after its last write; a render on another stream first
    // waits for view_ev on the GPU (read-after-write, write-after-write).  Renders are tracked by stream: a writer
    // drains the device first when renders were queued on a stream other than its own since the last drain
    // (write-after-read); same-stream renders are ordered by the stream, so one stream per context (the benchmark's
    // layout) never waits or drains.
    struct Sync {
        hipEvent_t view_ev = nullptr;
        hipStream_t view_st = nullptr;
        bool view_rec = false;                 // view_ev was recorded (on view_st)
        hipStream_t reader_st = nullptr;       // the stream of the renders queued since the last drain ...
        bool readers = false;                  // ... (any)
        bool readers_multi = false;            // ... on more than one stream
    } sync;

    // rt_render_packed_async frame t uses slot t % kSlots (device buffer 5 + slot): up to kSlots - 1 frames of
    // latency behind the one being queued
    static constexpr int kSlots = 3;

    // The host-buffer calls (rt_frames.hip: rt_render, rt_render_packed, rt_render_packed_async) run on the context's
    // own streams: renders on `rs` (blocking w.r.t. the null stream, like the null-stream renders it replaced), the
    // device-to-host copies on `cs`, so an asynchronous frame's copy overlaps the next frame's render.
    struct Frames {
        hipStream_t rs = nullptr, cs = nullptr;
        hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the render: rt_stats::kernel_ms
        hipEvent_t rendered[kSlots] = {};      // slot b's packed frame is in its device buffer
        hipEvent_t copied[kSlots] = {};        // slot b's packed frame is in its host buffer
        bool copied_rec[kSlots] = {};
        bool copied_cs[kSlots] = {};           // ... by a copy on the copy stream (else on the render stream)
        uint64_t ticket = 0;                   // rt_render_packed_async frames queued so far
        int last_copy_mode = -1;               // the mode the last packed frame took (rt_diag_copy_path)
        // rt_render's device buffers (grow-only, reused across calls): rgba32f, rgba8, rgb64f, raycount, sums,
        // packed slot 0, packed slot 1; then rt_render_adaptive's refined mask and workspace, rt_render_accum's sums, and
        // rt_render_converge's sums of squares, pass counts and active word (its sums are rt_render_accum's buffer)
        static constexpr int kBufRefined = 5 + kSlots, kBufAdaptive = 6 + kSlots, kBufAccum = 7 + kSlots;
        static constexpr int kBufAccum2 = 8 + kSlots, kBufCount = 9 + kSlots, kBufActive = 10 + kSlots;
        static constexpr int kBufs = 11 + kSlots;
        void* d_out[kBufs] = {};
        size_t out_cap[kBufs] = {};
    } frames;

    // copy_mode 3 (rt_frames.hip sdma_*): the frame leaves on a copy (SDMA) engine — no CUs taken from the next render.
    // Per slot, the render stream stores 0 into `dep` (hipStreamWriteValue64 on the HSA signal's value) once the frame
    // is in its device buffer; the SDMA copies, queued with `dep` as their dependency, then move it, each decrementing
    // its own completion signal done[slot][half] (one signal per engine copy, initialised to 1).
    struct Sdma {
        bool tried = false, ok = false;
        hsa_agent_t gpu{0}, cpu{0};
        uint32_t engine = 0, engine2 = 0;      // the two lowest free engines (engine2 = 0: only one)
        hsa_signal_t dep[kSlots] = {}, done[kSlots][2] = {};
        volatile hsa_signal_value_t* dep_ptr[kSlots] = {};
        hipEvent_t fired[kSlots] = {};         // recorded on rs right after slot b's sdma_fire
        bool pending[kSlots] = {};
        int copies[kSlots] = {};               // engine copies queued for slot b (1 or 2)
        int writer = 0;                        // sdma_fire: 1 stream write-value, 2 signal kernel
    } sdma;
};

#define RT_HIP(call)                                                                                  \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return rt_fail(RT_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- what crosses the unit boundaries ------------------------------------------------------------------------------
inline bool float_format(int f) { return f == RT_PIXEL_RGBA32F || f == RT_PIXEL_GRAY32F; }

// log2 of a supersampling factor in {1, 2, 4, 8}, or -1.
inline int ss_log2_of(int samples) {
    return samples == 1 ? 0 : samples == 2 ? 1 : samples == 4 ? 2 : samples == 8 ? 3 : -1;
}

// rt_plain.hip.  The view cache's buffers, event and pinned word made (rt_ctx_create, with the device set; RT_OK, RT_ENOMEM
// or RT_EHIP) and released (rt_ctx_destroy, likewise); the calibrated view and the view seen once forgotten, so that the next
// two renders calibrate afresh (rt_diag_tile_order); the device render behind rt_render_dev / rt_render_dev_packed, with
// ray counters beside a packed image (render_packed_queue); the checks every render makes on its context, camera, size,
// depth and row plan, and the rows this process renders; the front of the sampled _dev entry points.
int view_create(rt_ctx* c);
void view_release(rt_ctx* c);
void view_forget(rt_ctx* c);
// The calibrated view if it has cone masks and sky verdicts — what the view diagnostics describe — or nullptr.
inline const rt_ctx::View::Calibrated* view_with_cones(const rt_ctx* c) {
    return c->view.cal && c->view.cal->cones ? &*c->view.cal : nullptr;
}
int render_dev_impl(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows, int fmt_f, void* pf,
                    int fmt_8, void* p8, double* rgb64f, uint32_t* raycount, void* stream, int ss_log2 = -1);
int render_local_rows(const rt_ctx* c, const rt_camera* cam, int W, int H, int depth, const rt_rows* rows,
                      int* local_rows);
int sample_grid_front(rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples, int* s,
                      rtk::RenderParams* P);

// rt_sampled.hip.  The kinds of the lens family (depth of field, soft shadows, motion blur), the checks on the arguments
// a kind reads and the family's one device render, which the host entry points of rt_frames.hip call too.
enum LensKind { kLensDof = 0, kLensSoft = 1, kLensMotion = 2 };
int lens_arg_checks(LensKind kind, const char* who, double aperture, double light_size, double shutter);
int lens_render_dev(LensKind kind, const char* who, rt_ctx* c, const rt_camera* cam, int W, int H, int depth,
                    int samples, double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                    double* rgb64f, uint32_t* raycount2, void* stream);
// The check on `jitter` and the device render of the jittered render, as `who` (rt_frames.hip's host entry point too).
int jitter_arg_checks(const char* who, int jitter);
int jitter_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, int W, int H, int depth, int samples, int jitter,
                      uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                      double* rgb64f, uint32_t* raycount2, void* stream);
// The device render of the shutter render, as `who` (rt_frames.hip's host entry point too).
int shutter_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                       int depth, int samples, int jitter, uint32_t seed, double aperture, double light_size,
                       double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream);
// The device render of the accumulating render, as `who` (rt_frames.hip's host entry point too); the most passes of a call.
constexpr int kAccumCallPasses = 65536;
int accum_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                     int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes, double aperture,
                     double light_size, double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                     uint32_t* raycount2, void* stream, const rt_window* win = nullptr, bool list = false);
// The checks on the converging render's own arguments and its device render, as `who` (rt_frames.hip's host entry point too).
int converge_arg_checks(const char* who, int passes, uint32_t min_passes, double tolerance);
int converge_render_dev(const char* who, rt_ctx* c, const rt_camera* cam, const rt_camera_motion* motion, int W, int H,
                        int depth, int samples, int jitter, uint32_t seed, int passes, uint32_t min_passes,
                        double tolerance, double aperture, double light_size, double shutter, double* accum,
                        double* accum2, uint32_t* count, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                        uint32_t* raycount2, uint32_t* active, void* stream, const rt_window* win = nullptr,
                        bool list = false);
// `win` of the two above: nullptr runs the frame's kernels; a window (checked by window_arg_checks against the W x H
// frame) runs the windowed ones on buffers whose pointers point at window pixel (0, 0) (rt_render_accum_window_dev).
// `list` (with win = nullptr): the context's list of windows (rt_set_windows), which must be of the W x H frame, in one
// launch of the list kernels per launch group, on buffers laid out as rt_window_list_plan says.
int window_arg_checks(const char* who, const rt_window* win, int W, int H);

// rt_frames.hip.  Waits for the SDMA copies in flight and destroys the engine path's signals (rt_ctx_destroy, after
// the context's streams have drained).
void sdma_destroy(rt_ctx* c);
