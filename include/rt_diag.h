/*
 * rt_diag.h — diagnostics exported by librt_amd.so beside the drop-in boundary (rt_api.h).
 *
 * Not part of the reference's interface: these entry points exist so the parity tests can check the
 * device arithmetic the render kernel relies on, operand by operand, against the compiler's IEEE
 * sequences (and, on the host, against binary64 arithmetic as the reference's Point does it,
 * Hw4/MySdlApplication.cpp:174-175).
 */
#ifndef RT_DIAG_H
#define RT_DIAG_H

#include "rt_api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* op 0: for each of n vectors v (3 doubles, device memory) write 9 doubles (device memory):
 *   [0..2] v / |v| and [3] |v| with the compiler's sqrt and division (Point::normalize / length),
 *   [4..7] the same from the render kernel's fast path (unit), [8] its len_fast(v).
 * op 1: for each of n pairs (a, b) write 2 doubles: a / b (the compiler's IEEE division) and the render
 * kernel's division with a shared reciprocal (div_core(a, b, rcp_core(b)), used by the checker).
 * Asynchronous on `stream`.  RT_EINVAL for an unknown op or null buffers. */
int rt_probe_math_dev(int op, const double* in, int n, double* out, void* stream);

/* The scene agreement of a one-process-per-GPU group (rt_render_multi), without its collective, so the CPU tests
 * drive it from several processes.  rt_group_agree_due: 1 when a rank whose scene has `fingerprint` must vote
 * before its next frame (it differs from the last agreed one, or nothing was agreed yet).  rt_group_agree_vote:
 * this rank's vote {h, ~h, a, ~a}.  rt_group_agree_combine: acc = element-wise unsigned max(acc, other) — what the
 * group's ncclAllReduce(ncclMax) computes.  rt_group_agree_verdict: RT_OK when the combined votes of every rank
 * name one scene (fingerprint and achromatic flag), else RT_EINVAL. */
int rt_group_agree_due(uint64_t fingerprint, int agreed, uint64_t agreed_fingerprint);
void rt_group_agree_vote(uint64_t fingerprint, int achromatic, uint64_t vote[4]);
void rt_group_agree_combine(uint64_t acc[4], const uint64_t other[4]);
int rt_group_agree_verdict(const uint64_t reduced[4]);

/* Tile-row dispatch order of later rt_render_dev calls of this context: mode 0 (default) adaptive — the
 * first render of a new (scene, camera, size, row plan, depth) times its 8-row tile rows and later
 * renders dispatch them longest first; mode 1 bottom-to-top.  Images are identical either way (every
 * tile is traced once, by the same code).  RT_EINVAL for another mode. */
int rt_diag_tile_order(rt_ctx* ctx, int mode);

/* Registers per work-item (*vgprs) and private scratch bytes per work-item (*scratch_bytes) of the render
 * kernel instance rt_render_dev launches for `depth` (0..7) and scene kind `variant`: 0 spheres + board,
 * 1 >= 16 spheres (wave-culling variant), 2 meshes or transparent materials, 3 ray trees (whose node stack
 * lives in scratch by design), 4 / 5 the achromatic (one-channel) instances of 0 / 1 (depth <= 3; RT_EINVAL
 * for deeper ones).  Needs a HIP device.  RT_EINVAL for bad arguments. */
int rt_diag_kernel_resources(int depth, int variant, int* vgprs, int* scratch_bytes);

/* Workgroups per CU the HIP runtime allows the render kernel (depth, variant) with lds_bytes of dynamic LDS. */
int rt_diag_kernel_occupancy(int depth, int variant, int lds_bytes, int* blocks_per_cu);

/* Which render-kernel instance a frame runs: the library's one selector, called with the facts it decides on.  No
 * context, no device.  The scene kind (tree, transparent, n_padded spheres rounded up to 4, the stride n_stride of
 * its per-sphere arrays, achromatic, lds_bytes of its record), the context's knobs (use_lds: RT_SCENE_IN_LDS,
 * wg_staging: RT_WG_STAGING, min_waves: RT_MIN_WAVES, 5 by default, achro_off: RT_ACHRO_OFF), the depth (0..7), the
 * output mode (0 RGBA images, 1 packed GRAY / RGB formats, 2 supersampled) and level_mask (1: not the frame itself but
 * the launch that writes a fast scene's level masks behind its calibration render).  out[0..10]: the instance's
 * kernel template (0 rt_render_kernel, 1 rt_render_kernel_sg) and its template arguments
 * LDS, MINW, TRANSP, CULL, WG, TREE, PACKED, FIX64, ACHRO, SS; out[11] the launch's dynamic LDS bytes; out[12] the tile
 * width in pixels.  RT_EINVAL for bad arguments, and (out written) when the build has no such instance. */
int rt_diag_render_route(int tree, int transparent, int n_padded, int n_stride, int achromatic, int lds_bytes,
                         int use_lds, int wg_staging, int min_waves, int achro_off, int depth, int mode, int level_mask,
                         int out[13]);

/* How this context's last rt_render_packed / rt_render_packed_async frame reached host memory: *mode 0 the copy
 * kernel on the copy stream, 1 behind the render on the render stream (copy kernel, or hipMemcpyAsync for pageable
 * memory), 2 stored by the render straight into mapped pinned memory, 3 an SDMA engine, -1 no packed frame yet;
 * *writer how an SDMA frame's start is signalled (1 the stream's write-value operation, 2 a one-wave kernel, 0 the
 * engine is not set up).  RT_EINVAL for a null context. */
int rt_diag_copy_path(rt_ctx* ctx, int* mode, int* writer);

/* Sky tiles: 8 x 8 pixel tiles none of whose primary rays can hit anything — a proof from the tile's bounding cone
 * against the board's edges and the spheres' cones, made per wave by the render kernel, which then stores the miss
 * constants without tracing (RT_SKY_TILES=0 in the environment of rt_ctx_create turns the early-out off; the images
 * are the same bytes either way).  rt_diag_sky_tiles evaluates the kernel's verdict on the host, no device needed:
 * out[ty * tiles_x + tx] = 1 when tile (tx, ty) of the width x height frame (the rank's local rows when `rows` is
 * given) is proved, else 0; tiles_x = ceil(width / 8), tile rows = ceil(local rows / 8), n their product.  Scenes the
 * early-out does not cover (meshes, transparent materials, fewer than 8 or more than 64 spheres) give all zeros.
 * RT_EINVAL for bad arguments or another n. */
int rt_diag_sky_tiles(const rt_scene* scene, const rt_camera* cam, int width, int height, const rt_rows* rows,
                      uint8_t* out, size_t n);

/* The verdicts the waves themselves reached in this context's last calibration render (the second render of a
 * static view; later renders of that view read them from their dispatch records): *tiles the view's tile count,
 * *sky how many took the early-out.  Both 0 when no calibrated view holds verdicts.  Waits for the device. */
int rt_diag_sky_count(rt_ctx* ctx, int* tiles, int* sky);

/* Runs of sky tiles: a cached render of a calibrated static view sends one wave per run of up to RT_SKY_RUN_MAX
 * adjacent sky tiles of a tile row (read by rt_ctx_create; 1: one wave per tile, 0: whole streaks), from a
 * run-compacted dispatch table its calibration builds beside the plain one.  Images are the same bytes either way.
 * rt_diag_sky_run_plan evaluates the plan on the host, no device needed, with the function the device runs: for the
 * verdict grid sky[ty * tiles_x + tx] (nonzero: sky) and run_max >= 1, run[ty * tiles_x + tx] = 0 for a tile that is
 * a dispatch position of its own and traces, len >= 1 for the first tile of a run of len sky tiles, -1 for the run's
 * other tiles; *positions the dispatch positions in all.  RT_EINVAL for bad arguments.
 * rt_diag_disp_count: what the last cached render of this context's calibrated view launched — *positions its dispatch
 * positions, *tiles the view's tiles, *run_max the longest run its table may hold (1: the plain table, positions =
 * tiles).  All 0 before the first such render. */
int rt_diag_sky_run_plan(const uint8_t* sky, int tiles_x, int tiles_y, int run_max, int32_t* run, int* positions);
int rt_diag_disp_count(rt_ctx* ctx, int* positions, int* tiles, int* run_max);

/* Tile classes: the calibration of a static view of a fast-kernel scene (8 .. 15 padded spheres, opaque, no meshes) with
 * level masks marks every tracing tile whose primary cone mask and level masks keep no sphere as sphere-free, and the
 * cached renders of that view trace such a tile without the sphere code (RT_TILE_CLASSES=0 in the environment of
 * rt_ctx_create leaves every dispatch record unmarked; the images are the same bytes either way).
 * rt_diag_tile_class_plan evaluates the decision on the host, no device needed, with the function the device runs: for
 * `tiles` tiles with the cone masks cone[t], the sky verdicts sky[t] (nonzero: sky; null: none) and `slots` level masks
 * each, masks[t * slots + k] (null when slots = 0), of a scene of n_spheres <= 64 (padded) spheres, out[t] = 1 when
 * tile t is sphere-free — not sky, and no bit below n_spheres set in its cone mask or in any of its slots — else 0.
 * RT_EINVAL for bad arguments (null cone or out, tiles < 0, slots < 0, slots > 0 without masks, n_spheres outside
 * 0 .. 64).
 * rt_diag_tile_classes: the classes of this context's last calibrated view as its calibration decided them (whatever
 * RT_TILE_CLASSES says about carrying them in the records) — *tiles the view's tile count, *sky and *sphere_free how
 * many are in each class.  All 0 when the calibrated view holds no classes (culling-kernel scenes, views without level
 * masks, no calibrated view).  rt_diag_tile_class_grid copies the grid out, out[ty * tiles_x + tx] = 0 a tracing tile,
 * 1 sky, 2 sphere-free; RT_EINVAL unless n is that tile count.  Both wait for the device. */
int rt_diag_tile_class_plan(const uint64_t* cone, const uint8_t* sky, const uint64_t* masks, int tiles, int slots,
                            int n_spheres, uint8_t* out);
int rt_diag_tile_classes(rt_ctx* ctx, int* tiles, int* sky, int* sphere_free);
int rt_diag_tile_class_grid(rt_ctx* ctx, uint8_t* out, size_t n);

/* Flat tiles: among the sphere-free tiles of such a view, those whose 64 primary rays (lanes past the frame edge
 * clamped to the last pixel) all hit the board, seen from an eye that passes the board's origin skip.  Every such ray
 * is lit by every light and its reflected ray hits nothing, so the cached renders of the view trace these tiles on a
 * straight-line path (RT_FLAT_TILES=0 in the environment of rt_ctx_create leaves every record unmarked, and
 * RT_TILE_CLASSES=0 implies it; the images are the same bytes either way).  The verdict is made by the view's
 * calibration, for the views whose kernel instance reads it: plain renders of every depth and packed ones up to depth 1.
 * rt_diag_flat_tiles: *tiles the tile count of this context's last calibrated view, *flat how many its calibration found
 * flat (whatever RT_FLAT_TILES says about carrying them in the records).  Both 0 when the view holds no verdicts (no
 * tile classes, a supersampled view, a packed view beyond depth 1, no calibrated view).  rt_diag_flat_tile_grid copies
 * the grid out, out[ty * tiles_x + tx] = 1 flat, else 0; RT_EINVAL unless n is that tile count.  A flat tile reports as
 * sphere-free in rt_diag_tile_class_grid.  Both wait for the device.
 * rt_diag_disp_sky_word evaluates, on the host and with the function the device's table kernels run, the `sky` word of
 * a dispatch record: `run` what the word holds outside the classes (0 a tracing tile, 1 .. 65535 the run length of a sky
 * record), sphere_free and flat the tile's class (a sphere-free tile traces: run = 0).  The top bit marks sphere-free,
 * the bit below it flat; flat is set only beside sphere-free.  RT_EINVAL for a null word, run > 65535, or a sphere-free
 * tile with run != 0. */
int rt_diag_flat_tiles(rt_ctx* ctx, int* tiles, int* flat);
int rt_diag_disp_sky_word(uint32_t run, int sphere_free, int flat, uint32_t* word);
/* rt_diag_flat_gates evaluates, on the host and with the function the device runs, the wave-uniform gates of the flat
 * class for `scene` seen from eye[3]: *gates = 1 when the scene has its board and |eye.y| is within the board's
 * origin-skip limit (*skip_y, if not null: that limit, -1 where the skip is not proven); *hits_ok = the per-eye flag of
 * the hit points' bounding-sphere shortcut, as the device sets it for that eye.  No device needed.  RT_EINVAL for null
 * eye, gates or hits_ok, or a scene the builder rejects. */
int rt_diag_flat_gates(const rt_scene* scene, const double* eye, int* gates, int* hits_ok, double* skip_y);
int rt_diag_flat_tile_grid(rt_ctx* ctx, uint8_t* out, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* RT_DIAG_H */
