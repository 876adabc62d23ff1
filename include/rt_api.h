/*
 * rt_api.h — C ABI of the MI355X-native per-pixel ray tracer.
 *
 * This is the drop-in boundary for the reference's frame hand-off:
 *   draw()            Hw4/MySdlApplication.cpp:1541-1563  (builds lights + camera, calls L5)
 *   rayTraceScreen()  Hw4/MySdlApplication.cpp:1251-1324  (camera basis, per-pixel rays, GL emit)
 *   rayTraceRay()     Hw4/MySdlApplication.cpp:1184-1249  (closest hit, shadows, bounces)
 *   Shape/Triangle/CheckerBoard::intersection  MySdlApplication.cpp:611-823, 1084-1113
 * The reference has no plugin/FFI API: its seam is a C++ call made on the GL thread.
 * This header replaces that call with plain C types: the scene is a flat descriptor built from the
 * same inputs `loadScene` uses (MySdlApplication.cpp:1495-1539), pixels land in caller-owned buffers.
 *
 * Conventions
 *  - All geometry is IEEE binary64, exactly as the reference's `Point` (MySdlApplication.cpp:136-212).
 *  - Pixel (i, j) has j = 0 at the BOTTOM row (gluOrtho2D(0,W,0,H), MySdlApplication.cpp:1383) and is
 *    stored at index j*W + i of a full image.  A row-banded call (rt_rows) stores its rows densely in
 *    local order; rt_unshuffle_dev puts gathered bands back into image order.
 *  - Every entry point returns RT_OK (0) or a negative RT_E* code; rt_last_error() gives the text for
 *    the calling thread.  There is no silent fallback: without a HIP device every render call fails
 *    with RT_EHIP.
 *  - One rt_ctx per (thread, device).  A context owns the device copy of the scene; rt_render_dev is
 *    asynchronous on the caller's stream and does not allocate, so it may be captured in a hipGraph.
 *    A context's renders must be stream-ordered (one stream at a time): a render may update the
 *    context's per-camera data (sphere data for a new eye, the tile-row dispatch order).
 *  - hipGraph capture: a captured render is self-contained (it carries its own per-eye preparation and
 *    uses the identity tile-row order), so renders of other views between replays do not disturb it.
 *    rt_set_scene with a different scene invalidates captured graphs (the scene record may move).
 *  - Multi-GPU: rt_group + rt_render_multi split a frame's rows over GPUs and gather
 *    them to rank 0 over RCCL (one process driving several GPUs, or one process per GPU).
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 10

#define RT_OK            0
#define RT_EINVAL       -1   /* bad argument (null pointer, size, unsupported material, ...) */
#define RT_EHIP         -2   /* HIP runtime error or no device */
#define RT_ENOMEM       -3   /* allocation failed */
#define RT_EUNSUPPORTED -4   /* reference feature outside the GPU path (cylinder/cone stubs) */

#define RT_MAX_SPHERES 1024
#define RT_MAX_LIGHTS  16
#define RT_MAX_MESHES  64
#define RT_MAX_DEPTH   7     /* reference uses MAX_DEPTH = 5 (MySdlApplication.cpp:48) */

#define RT_MESH_TETRAHEDRON 1   /* Tetrahedron(p, edgeSize), MySdlApplication.cpp:863-900 */
#define RT_MESH_CUBE        2   /* Cube(p, edgeSize),        MySdlApplication.cpp:903-950 */

/* Material — MySdlApplication.cpp:272-307 (ambient, diffuse, specular, transparency, refraction). */
typedef struct rt_material {
    double ambient[3];
    double diffuse[3];
    double specular[3];
    double transparency[3];
    double refraction;
} rt_material;

/* Sphere(p, r) — MySdlApplication.cpp:846-860.  `center` is scene-local, exactly the `p` handed to the
 * reference constructor (e.g. convertStringCoordinate("d7")); the world centre is center + scene.position. */
typedef struct rt_sphere {
    double center[3];
    double radius;
} rt_sphere;

/* Light(color, position) — MySdlApplication.cpp:214-232.  World coordinates. */
typedef struct rt_light {
    double color[3];
    double position[3];
} rt_light;

/* A triangle-mesh composite of the reference: a Shape with a bounding sphere of radius
 * sqrt(3)*edge/2 around `position` and triangle sub-objects (tetrahedron: 4 triangles; cube: 6 Quads of
 * 2 triangles), material g_tetrahedronMaterial / g_cubeMaterial.  `position` is scene-local, the `p`
 * handed to the constructor.  g_scene child order: the mesh comes after `after_spheres` spheres (and
 * after every mesh listed before it). */
typedef struct rt_mesh {
    int32_t kind;                /* RT_MESH_TETRAHEDRON or RT_MESH_CUBE */
    int32_t after_spheres;
    double position[3];
    double edge;
} rt_mesh;

/* The reference's g_scene (MySdlApplication.cpp:590) flattened: a bounding sphere at `position` of
 * `radius`, then children in insertion order — the CheckerBoard first when present (initScene2 inserts
 * it first, MySdlApplication.cpp:1442-1443), then spheres and meshes in the order given (see rt_mesh). */
typedef struct rt_scene {
    double position[3];          /* g_scene position, BOARD_POSITION (MySdlApplication.cpp:42) */
    double radius;               /* g_scene radius sqrt(3)*BOARD_HALF_SIZE; <= 0 disables the cull */
    int32_t has_board;           /* CheckerBoard present */
    int32_t n_spheres;           /* <= RT_MAX_SPHERES */
    int32_t n_lights;            /* <= RT_MAX_LIGHTS */
    int32_t reserved0;
    double board_position[3];    /* CheckerBoard(p) argument (scene-local) */
    double board_half_size;      /* BOARD_HALF_SIZE (MySdlApplication.cpp:44) */
    double square_edge_size;     /* SQUARE_EDGE_SIZE (MySdlApplication.cpp:46) */
    double small_number;         /* SMALL_NUMBER (MySdlApplication.cpp:50) */
    double attenuation_factor;   /* ATTENUATION_FACTOR (MySdlApplication.cpp:35) */
    rt_material white_square;    /* g_whiteSquare (MySdlApplication.cpp:583) */
    rt_material black_square;    /* g_blackSquare (MySdlApplication.cpp:585) */
    rt_material sphere_material; /* g_sphereMaterial (MySdlApplication.cpp:586) */
    const rt_sphere* spheres;    /* host pointer, n_spheres entries */
    const rt_light* lights;      /* host pointer, n_lights entries (the per-frame `lights` vector) */
    rt_material tetrahedron_material;  /* g_tetrahedronMaterial (MySdlApplication.cpp:587) */
    rt_material cube_material;         /* g_cubeMaterial (MySdlApplication.cpp:588) */
    int32_t n_meshes;            /* <= RT_MAX_MESHES */
    int32_t reserved1;
    const rt_mesh* meshes;       /* host pointer, n_meshes entries */
} rt_scene;

/* Camera — rayTraceScreen's arguments (MySdlApplication.cpp:1251-1252, called at :1560).
 * Primary ray of pixel (i, j): Line(eye, sp) with
 *   sp = (look_at + (pitch*(double)(i + bottom_x))*right) + (pitch*(double)(j + bottom_y))*up'
 * where right = normalize((look_at-eye) x up), up' = normalize(right x (look_at-eye))
 * (MySdlApplication.cpp:1270-1279).  pitch = 1 is the reference's unit pixel step (:1315, :1321). */
typedef struct rt_camera {
    double eye[3];               /* CAMERA_POSITION (MySdlApplication.cpp:38) */
    double look_at[3];           /* LOOK_AT_VECTOR (MySdlApplication.cpp:39) */
    double up[3];                /* UP_VECTOR (MySdlApplication.cpp:40) */
    double pitch;                /* world units between adjacent pixel centres */
    int32_t bottom_x;            /* -W/2 (C integer division, MySdlApplication.cpp:1560) */
    int32_t bottom_y;            /* -H/2 */
} rt_camera;

/* Row banding for multi-GPU sharding: the image's rows are cut into bands of `band_height` rows and
 * band b goes to rank b % n_ranks.  A call renders only its rank's rows, densely, in increasing order.
 * `frames` > 1 renders that many frames of the same view in one call, frame-major: the rank's rows of
 * frame 0, then of frame 1, ... (each frame banded the same way), so an all-to-all can send frame f's
 * rows to rank f.  NULL rt_rows* (or n_ranks == 1 and frames <= 1) means one full image. */
typedef struct rt_rows {
    int32_t band_height;
    int32_t n_ranks;
    int32_t rank;
    int32_t frames;              /* 0 or 1: one frame */
} rt_rows;

/* Ray counts actually traced (SURVEY.md §8d rule): primary segments, reflected segments (levels 1..B,
 * only after a hit), shadow rays (one per light per hit). */
typedef struct rt_stats {
    uint64_t primary_rays;
    uint64_t reflect_rays;
    uint64_t shadow_rays;
    double kernel_ms;
} rt_stats;

/* Per-ray hit record, the observable part of the reference's Intersection (MySdlApplication.cpp:309-359). */
typedef struct rt_hit {
    double point[3];
    double normal[3];
    double reflected_end[3];     /* reflectedRay().endPoint() = point + r */
    double transmitted_end[3];   /* transmittedRay().endPoint() = point + t (t = 0 on total reflection) */
    int32_t hit;                 /* Intersection::intersects() */
    int32_t material;            /* 0 white square, 1 black square, 2 sphere, 3 tetrahedron, 4 cube, -1 none */
} rt_hit;

typedef struct rt_ctx rt_ctx;

/* ---- library / device ---------------------------------------------------------------------- */
int rt_abi_version(void);
const char* rt_last_error(void);
int rt_device_count(int* count);
int rt_ctx_create(int device, rt_ctx** out);
int rt_ctx_destroy(rt_ctx* ctx);

/* ---- scene (host side; no device needed) --------------------------------------------------- */
/* Fill constants and materials with the reference's globals (MySdlApplication.cpp:31-52, 583-590):
 * empty scene, board present at (0,0,0), no spheres, no lights. */
int rt_scene_init_reference(rt_scene* scene);
/* convertStringCoordinate (MySdlApplication.cpp:1326-1346): "b6" -> board-local point. */
int rt_convert_string_coordinate(const char* square, double out[3]);
/* Light placement used by loadScene (MySdlApplication.cpp:1511):
 * BOARD_POSITION + (0, 3.5*SQUARE_EDGE_SIZE, 0) + convertStringCoordinate(square). */
int rt_light_position_from_square(const char* square, double out[3]);
/* loadScene (MySdlApplication.cpp:1495-1539) over boardMap entries (square -> type; types as the
 * reference enum {LIGHT, TETRAHEDRON, CUBE, SPHERE, CYLINDER, CONE}, MySdlApplication.cpp:16).
 * Duplicate squares keep the last type (boardMap[tmp] = type, :1467), entries are visited in
 * std::map<string> order, the last light wins.  Spheres go to sphere_buf (capacity sphere_cap),
 * tetrahedra and cubes to mesh_buf (capacity mesh_cap) in child order, the light (white,
 * g_lightColor) to *light.  Returns RT_EUNSUPPORTED if a cylinder or cone is present (their reference
 * implementations are stubs: MySdlApplication.cpp:1000-1020, 457-458); everything else is still filled. */
int rt_load_scene(const char* const* squares, const int32_t* types, int n, rt_scene* scene,
                  rt_sphere* sphere_buf, int sphere_cap, rt_mesh* mesh_buf, int mesh_cap, rt_light* light);
/* draw()'s camera (MySdlApplication.cpp:1556-1560) for a W x H window at the given pitch. */
int rt_camera_init_reference(rt_camera* cam, int width, int height, double pitch);
/* Number of rows a rank renders under `rows` (NULL = all rows), over all its frames. */
int rt_local_rows(int height, const rt_rows* rows, int* out);
/* Image row of local row `local_row` under `rows`: frame * height + row within the frame. */
int rt_global_row(int height, const rt_rows* rows, int local_row, int* out);

/* ---- device path ---------------------------------------------------------------------------- */
/* Validate and upload the scene (scene + spheres + lights are copied; caller keeps ownership).
 * A scene identical to the uploaded one (same flattened record) is a no-op: no device work, the per-eye
 * data and tile-row order are kept (rt_render calls this every frame).  A changed scene first waits for
 * all work on the context's device (renders in flight on any stream read the old record), then uploads
 * synchronously. */
int rt_set_scene(rt_ctx* ctx, const rt_scene* scene);

/* Render this rank's rows of a width x height frame with `depth` bounces (rayTraceRay's `depth`).
 * Device pointers, each nullable, each local_rows*width pixels:
 *   rgba32f: float4 (r,g,b,1) unclamped, rgba8: clamp(c,0,1)*255 rounded (RGBA8 = floor(v*255+0.5)),
 *   rgb64f: 3 doubles (the reference's double colour, for bit-exact parity),
 *   raycount: per pixel packed (primary+reflect) | shadow << 16.
 * `stream` is a hipStream_t (NULL = default stream).  Asynchronous; no allocation. */
int rt_render_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth,
                  const rt_rows* rows, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                  uint32_t* raycount, void* stream);

/* ---- supersampled rendering (ABI 8) -------------------------------------------------------------- */
/* S x S samples per pixel (S = `samples` in {1, 2, 4, 8}) on a regular grid, summed in the render kernel, so only
 * the width x height output pixels are written.  This is NOT the app's jittered, adaptive rayTraceScreen
 * (rt_render_screen is): the samples are fixed, and every one of them is a pixel of the existing contract.
 *  1. Sample-grid camera cam_s (rt_camera_supersample): eye, look_at and up of `cam`; pitch_s = cam.pitch / S
 *     (exact: S is a power of two); bottom_x_s = S * cam.bottom_x, bottom_y_s = S * cam.bottom_y (RT_EINVAL when
 *     a product overflows int32).  For odd W this is not the camera rt_camera_init_reference(S * W, ...) makes:
 *     -S * (W / 2) differs from -(S * W) / 2.
 *  2. Sample (a, b) of pixel (i, j), 0 <= a, b < S, has the colour rt_render_dev gives pixel (S i + a, S j + b) of
 *     the S W x S H frame of cam_s: rayTraceRay on the primary ray of the camera comment above.  The samples of a
 *     pixel cover its cell [i, i + 1) x [j, j + 1) in pitch units, starting at the one-sample render's point.
 *  3. Per channel, in FP64, the samples are summed as a fixed pairwise tree: first along a, v[a] <- v[2a] + v[2a+1]
 *     repeated log2 S times, then the same along b, then one multiplication by 1.0 / (S * S) (exact).  The order is
 *     part of the contract: another order differs in the last bits.
 *  4. rgb64f is that value; rgba32f its (float) with alpha 1; rgba8 floor(clamp(c, 0, 1) * 255 + 0.5) of it.
 *     raycount2 holds two uint32 per pixel: primary + reflected segments, then shadow rays, each summed over the
 *     pixel's samples (the packed 16 + 16-bit word of rt_render_dev would overflow).
 *  5. The reference yields NaN colours in some ray-tree scenes.  A channel with a NaN sample is NaN; which NaN
 *     (sign, payload) is unspecified.  rgba8 of a NaN is 0, as in rt_render_dev.
 *  6. samples = 1 writes the images rt_render_dev writes (the counters still as two words).
 * Host only: *out = cam_s (out may be cam).  RT_EINVAL for samples outside {1, 2, 4, 8} or int32 overflow. */
int rt_camera_supersample(const rt_camera* cam, int samples, rt_camera* out);
/* The supersampled render of this rank's rows.  Device pointers, each nullable, local_rows * width pixels;
 * asynchronous on `stream`, no allocation: the rules of rt_render_dev (view calibration and hipGraph capture
 * included, applied to the sample grid).  `rows` with frames <= 1 is honoured (bands are cut in output rows);
 * frames > 1 with samples > 1 fails with RT_EINVAL, as does samples outside {1, 2, 4, 8}. */
int rt_render_ss_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples,
                     const rt_rows* rows, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                     void* stream);
/* Synchronous host-buffer convenience, as rt_render (full frame).  *stats: primary_rays = width * height * S * S,
 * reflect_rays and shadow_rays from the summed counters. */
int rt_render_ss(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height, int depth,
                 int samples, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- adaptive supersampling (ABI 9) -------------------------------------------------------------- */
/* The S x S samples of rt_render_ss_dev only where the one-sample image has contrast; one sample elsewhere.
 * Deterministic (not the app's rand()-driven rayTraceScreen chain: rt_render_screen is), and defined entirely by
 * outputs of the calls above.  For a full width x height frame, S = `samples` in {1, 2, 4, 8} and T = `threshold`
 * in {-1, .., 255}:
 *  1. Base frame.  B is the frame rt_render_dev(cam, width, height, depth) writes; q its RGBA8 image,
 *     floor(clamp(c, 0, 1) * 255 + 0.5) with NaN -> 0.  B(i, j) is sample (0, 0) of pixel (i, j) of the
 *     supersampled render, bit for bit.
 *  2. Criterion.  Pixel (i, j) is REFINED iff some in-frame 4-neighbour n in {(i +- 1, j), (i, j +- 1)} and some
 *     channel c in {r, g, b} has |q_c(i, j) - q_c(n)| > T, in integer arithmetic.  It always reads the base bytes,
 *     never a refined value.  T = 255 refines nothing; T = -1 refines every pixel that has an in-frame neighbour
 *     (every pixel of any frame larger than 1 x 1); a 1 x 1 frame refines nothing.
 *  3. Value.  A refined pixel has exactly the value rt_render_ss_dev(cam, width, height, depth, S) gives it (the
 *     fixed pairwise tree along a, then along b, times 1 / (S S)); an unrefined pixel has exactly B(i, j).
 *     rgb64f, rgba32f and rgba8 derive from that value as in rt_render_ss_dev.  raycount2 holds two uint32 per
 *     pixel: the base sample's counters for an unrefined pixel, the sums over the S x S samples for a refined one.
 *     NaN rules as in rt_render_ss_dev.
 *  4. `refined`: a nullable uint8 image, width x height, 1 for a refined pixel and 0 otherwise.
 *  5. Pins that follow: T = 255 writes the images rt_render_dev writes; T = -1 (frames larger than 1 x 1) writes
 *     the images rt_render_ss_dev writes.  There is NO shortcut for either: both run the same passes as any other
 *     T.  S = 1 writes the base images, and `refined` still reports the criterion.
 * Full frames only: a row band's criterion would need rows its rank does not render, so there is no rt_rows.
 * rt_render_multi, the packed and asynchronous host paths and the drop-in draw() render one sample per pixel. */
/* Host only: the bytes of device workspace rt_render_adaptive_dev needs for a width x height frame (the work list
 * and its counter, and room for the base RGBA8 image).  RT_EINVAL for samples outside {1, 2, 4, 8} or a bad size. */
int rt_adaptive_workspace_bytes(int width, int height, int samples, size_t* bytes);
/* Device pointers, each output nullable, width * height pixels; `workspace`: workspace_bytes >=
 * rt_adaptive_workspace_bytes(...) of device memory, 16-byte aligned, owned by the caller and used by one call at a
 * time (its first uint32 holds the number of refined pixels once the call's work is done).  Asynchronous on
 * `stream`, no allocation and no host synchronisation, so it may be captured in a hipGraph like rt_render_dev; the
 * base pass follows rt_render_dev's view-calibration and capture rules.  Three passes: the base render into the
 * caller's outputs; a classification pass that writes `refined` and compacts the refined pixels into a work list
 * (whose order is unspecified and influences no output); a refine pass over the list, S x S lanes per pixel reduced
 * in the wave, which overwrites the refined pixels in every requested output.
 * RT_EINVAL (rt_last_error names the argument) for `samples` outside {1, 2, 4, 8}, `threshold` outside -1 .. 255, a
 * null, misaligned or too small `workspace`, and when the sample-grid camera overflows int32. */
int rt_render_adaptive_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples,
                           int threshold, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                           uint8_t* refined, void* workspace, size_t workspace_bytes, void* stream);
/* Synchronous host-buffer convenience, as rt_render_ss (the workspace is the context's).  *n_refined (nullable): the
 * number of refined pixels n.  *stats from the summed raycount2: primary_rays = (width * height - n) + n * S * S. */
int rt_render_adaptive(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height, int depth,
                       int samples, int threshold, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint8_t* refined,
                       rt_stats* stats, uint64_t* n_refined);

/* ---- depth of field (ABI 10) ---------------------------------------------------------------------- */
/* A thin-lens render: the S x S samples of a pixel start at S x S points of a square lens around the eye, so
 * geometry in the focal plane is sharp (and anti-aliased as in rt_render_ss_dev) and geometry off it is blurred.
 * Deterministic, and defined entirely by rt_trace_rays_dev on rays this text spells out.  For a full
 * width x height frame, S = `samples` in {1, 2, 4, 8} and A = `aperture`, finite and >= 0, the half-width in world
 * units of a square lens centred at the eye, in the plane spanned by right and up':
 *  1. Sample-grid camera.  cam_s = rt_camera_supersample(cam, S); right and up' are its basis from the camera
 *     comment above (the same vectors the render kernels use; they are `cam`'s too).
 *  2. Sample (a, b) of pixel (i, j), 0 <= a, b < S, is the ray Line(e(a, b), sp_s(S i + a, S j + b)): sp_s is the
 *     primary-ray end point of cam_s, and the ray starts at
 *         e(a, b) = (eye + (A * t_a) * right) + (A * t_b) * up',   t_a = (double)(2 a + 1 - S) / (double)S
 *     (an exact quotient: S is a power of two), each parenthesis one IEEE operation per component, in exactly this
 *     order.  The lens point is paired with the sub-pixel point of the same (a, b).
 *  3. The colour and the counters of a sample are what rt_trace_rays_dev gives that ray:
 *     rayTraceRay(scene, lights, Line(start, end), colour, depth).
 *  4. Reduction and outputs follow rt_render_ss_dev rules 3-5 exactly: the fixed pairwise tree along a, then along
 *     b, then * 1 / (S S); rgb64f, rgba32f and rgba8 derive from the reduced value; raycount2 holds two uint32 per
 *     pixel, summed over the samples; a channel with a NaN sample is NaN (sign and payload unspecified), its rgba8 0.
 *  5. Focal plane: the plane through look_at spanned by right and up'.  All S x S rays of a pixel pass through its
 *     points of that plane, so geometry there is sharp.
 *  6. rt_camera_focus(cam, ratio, out) moves the focal plane without changing the view: look_at'[c] = eye[c] +
 *     ratio * (look_at[c] - eye[c]), pitch' = ratio * pitch, everything else copied; ratio == 1.0 copies `cam`
 *     unchanged bit for bit.  Host only; RT_EINVAL for a ratio that is <= 0 or not finite; out may be cam.
 *  7. Pins that follow, with NO shortcut in the implementation: A = 0 writes the images and counters
 *     rt_render_ss_dev writes; S = 1 writes the images rt_render_dev writes for any A (t = 0; the counters are still
 *     two words).  Both pins assume an eye with no -0.0 component: eye + (+-0) is the eye only then.  Both cases run
 *     the same kernel as any other A.
 *  8. Full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host synchronisation, so the
 *     call may be captured in a hipGraph.  It has no per-view state: it does not calibrate and neither reads nor
 *     writes the context's cone or level masks or its tile order, which stay intact for later rt_render_dev calls.
 *  9. RT_EINVAL (rt_last_error names the argument) for `samples` outside {1, 2, 4, 8}, an `aperture` that is
 *     negative, NaN or infinite, a bad frame size (the sample frame S width x S height holds at most 2^31 samples),
 *     and an int32 overflow of the sample-grid camera.
 * 10. The lens is a regular square grid: jittered (here: rt_render_jitter_dev has them) or disc-shaped lenses are not
 *     offered.  rt_render_multi, the
 *     packed and asynchronous host paths and the drop-in draw() render through a pinhole.
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, A = 8, RGBA32F + RGBA8, tools/bench_dof.py): S = 2 124 us and
 * S = 4 503 us per frame, 1.42 x and 1.44 x rt_render_ss_dev at the same S, and 3.9 x and 3.0 x faster than the same
 * rays through rt_trace_rays_dev with the reduction in further passes.  Other scenes and depths: not measured. */
int rt_camera_focus(const rt_camera* cam, double ratio, rt_camera* out);
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_dof_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples,
                      double aperture, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                      void* stream);
/* Synchronous host-buffer convenience, as rt_render_ss.  *stats: primary_rays = width * height * S * S, reflect_rays
 * and shadow_rays from the summed counters. */
int rt_render_dof(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height, int depth,
                  int samples, double aperture, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- soft shadows (ABI 10: new symbols only) -------------------------------------------------------- */
/* Square area lights: the S x S samples of a pixel see every light at S x S points of a square panel, so shadow
 * edges become penumbrae.  Deterministic, and defined entirely by rt_set_scene and rt_trace_rays_dev on scenes and
 * rays this text spells out.  For a full width x height frame, S = `samples` in {1, 2, 4, 8}, A = `aperture` and
 * R = `light_size`, both finite and >= 0:
 *  1. Rays.  Exactly rt_render_dof_dev rules 1-2: sample (a, b) of pixel (i, j) is the ray
 *     Line(e(a, b), sp_s(S i + a, S j + b)), with e(a, b) on the square lens of half-width A.
 *  2. Lights of a sample.  Every light i of the uploaded scene is a square panel of half-width R centred at the
 *     light's position L_i, in the world xz-plane (parallel to the reference's board, whose normal is (0, -1, 0)).
 *     Sample (a, b) sees light i at
 *         (L_i.x + (R * t_a), L_i.y, L_i.z + (R * t_b)),   t_a = (double)(2 a + 1 - S) / (double)S
 *     (an exact quotient), each parenthesis and each sum one IEEE operation.  Colours are unchanged, one R serves all
 *     lights, and the light point is paired with the lens point and the sub-pixel point of the same (a, b).
 *  3. Value.  The colour and the counters of a sample are what rt_trace_rays_dev gives its ray after rt_set_scene of
 *     the scene with the lights of rule 2: rayTraceRay(scene_ab, lights_ab, Line(start, end), colour, depth).
 *  4. Reduction and outputs follow rt_render_ss_dev rules 3-5 exactly: the fixed pairwise tree along a, then along
 *     b, then * 1 / (S S); rgb64f, rgba32f and rgba8 derive from the reduced value; raycount2 holds two uint32 per
 *     pixel, summed over the samples; a channel with a NaN sample is NaN (sign and payload unspecified), its rgba8 0.
 *  5. Pins that follow, with NO shortcut in the implementation (all run the same kernel as any other R): R = 0
 *     writes the images and counters rt_render_dof_dev writes, for any A; A = 0 and R = 0 writes what
 *     rt_render_ss_dev writes; S = 1 writes the images rt_render_dev writes for any A and R (t = 0; the counters are
 *     still two words).  The pins assume that no light has a -0.0 x or z component (L + (+-0) is L only then), as
 *     the lens pins assume for the eye.
 *  6. Full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host synchronisation, so the
 *     call may be captured in a hipGraph.  No per-view state, as rt_render_dof_dev rule 8.  The displaced lights are
 *     formed in the kernel: the call neither writes nor re-uploads the context's scene record, and later
 *     rt_render_dev, rt_render_dof_dev and other calls on the context give exactly what they gave before.
 *  7. RT_EINVAL (rt_last_error names the argument) for `samples` outside {1, 2, 4, 8}, an `aperture` or a
 *     `light_size` that is negative, NaN or infinite, a bad frame size (the sample frame S width x S height holds at
 *     most 2^31 samples), and an int32 overflow of the sample-grid camera.  A rejected call writes no pixel.
 *  8. Not offered: per-light sizes, disc-shaped or jittered panels, and a pairing of light, lens and sub-pixel
 *     points other than by (a, b).  A penumbra is therefore a ramp of at most S * S steps, the same in every pixel
 *     (rt_render_jitter_dev turns the steps into noise).
 *     rt_render_multi, the packed and asynchronous host paths and the drop-in draw() keep point lights.
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, R = 40, A = 0, RGBA32F + RGBA8, tools/bench_soft.py): S = 2 130 us
 * and S = 4 525 us per frame, 1.07 x and 1.08 x rt_render_dof_dev at the same S and A (the price of a shadow test
 * without the point light's cone filter), 1.53 x rt_render_ss_dev, and 3.9 x and 3.1 x faster than S x S calls of
 * rt_trace_rays_dev on pre-uploaded displaced scenes with the reduction in further passes (5.3 x and 4.5 x with the
 * rt_set_scene uploads).  Other scenes and depths: not measured. */
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_soft_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples,
                       double aperture, double light_size, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                       uint32_t* raycount2, void* stream);
/* Synchronous host-buffer convenience, as rt_render_ss.  *stats: primary_rays = width * height * S * S, reflect_rays
 * and shadow_rays from the summed counters. */
int rt_render_soft(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height, int depth,
                   int samples, double aperture, double light_size, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                   rt_stats* stats);

/* ---- motion blur (ABI 10: new symbols only) --------------------------------------------------------- */
/* Moving spheres: the S x S samples of a pixel see the scene at S x S shutter times, so a moving sphere, its shadow and
 * its reflections are blurred along its path.  Deterministic, and defined entirely by rt_set_scene and
 * rt_trace_rays_dev on scenes and rays this text spells out.  For a full width x height frame, S = `samples` in
 * {1, 2, 4, 8}, A = `aperture` and R = `light_size`, both finite and >= 0, F = `shutter`, finite and in [0, 1], and the
 * displacements d_k of rt_set_motion (d[3 k + c]: half-extent of sphere k's motion during the exposure, scene-local):
 *  1. Rays and lights.  Exactly rt_render_soft_dev rules 1-2: the lens point, the sub-pixel point and the light point
 *     of the same (a, b).
 *  2. Time of a sample.  Sample (a, b) has the time index n = a + S b and the time
 *         sigma = F * u_n,   u_n = (double)(2 n + 1 - S S) / (double)(S S)
 *     (an exact quotient; sigma is one multiplication): S S distinct times per pixel, symmetric about 0, |sigma| < 1.
 *  3. Spheres of a sample.  Sphere k has the scene-local centre center[c] + (sigma * d_k[c]) per component: one
 *     multiplication, then one addition.  Radii, board, meshes, lights (apart from rule 1), materials and the bounding
 *     sphere are unchanged.
 *  4. Value.  The colour and the counters of a sample are what rt_trace_rays_dev gives its ray after rt_set_scene of
 *     the scene of rules 1 and 3 (which forms the world centre as that value + scene.position, one more addition).
 *  5. Reduction and outputs follow rt_render_ss_dev rules 3-5 exactly.
 *  6. Pins that follow, with NO shortcut in the implementation (all run the same kernel): F = 0 writes the images and
 *     counters rt_render_soft_dev writes, for any A and R; so do all d = 0, and a context with no motion set.  With
 *     R = 0 as well the output is rt_render_dof_dev's, with A = R = 0 rt_render_ss_dev's; S = 1 (sigma = 0) writes the
 *     images rt_render_dev writes.  The pins assume that no sphere centre has a -0.0 component.
 *  7. rt_set_motion copies the displacements and builds the device record the kernel reads (the swept spheres' filter
 *     records and bounding proof).  n_spheres must equal the uploaded scene's, else RT_EINVAL; (NULL, 0) clears the
 *     motion.  A CHANGED rt_set_scene also clears it; an identical scene (a no-op in rt_set_scene) keeps it.  It
 *     follows rt_set_scene's ordering rule: a changed motion first waits for all work on the context's device.  It may
 *     allocate, so it is not capturable.  The context's scene record is read, never written: every other call on the
 *     context gives exactly what it gave before.
 *  8. rt_render_motion_dev: full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host
 *     synchronisation, so the call may be captured in a hipGraph.  No per-view state; it neither reads nor writes the
 *     cone masks, the level masks or the tile order.
 *  9. RT_EINVAL (rt_last_error names the argument) for `samples` outside {1, 2, 4, 8}, an `aperture` or a `light_size`
 *     that is negative, NaN or infinite, a `shutter` that is negative, above 1, NaN or infinite, a non-finite
 *     displacement, a wrong n_spheres, a bad frame size, and an int32 overflow of the sample-grid camera.  A rejected
 *     call writes no pixel.
 * 10. Not offered: moving meshes, board, lights or camera; curved or accelerated paths; jittered times; a pairing of
 *     time with (a, b) other than rule 2.  A streak is therefore a sum of at most S S copies, the same in every pixel
 *     (rt_render_jitter_dev jitters the times; rt_render_shutter_dev moves the camera).
 *     rt_render_multi, the packed and asynchronous host paths and the drop-in draw() stay frozen in time.
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, one sphere moving by |d| = 40, F = 1, A = R = 0, RGBA32F + RGBA8,
 * tools/bench_motion.py): S = 2 139 us and S = 4 565 us per frame, 1.05 x and 1.06 x rt_render_soft_dev at the same S
 * (the price of per-lane sphere centres and swept filter records), 1.9 x and 1.8 x rt_render_ss_dev, and 3.6 x and
 * 2.9 x faster than S x S calls of rt_trace_rays_dev on pre-uploaded displaced scenes with the reduction in further
 * passes (5.4 x and 4.6 x with the rt_set_scene uploads).  Other scenes, depths and motions: not measured. */
int rt_set_motion(rt_ctx* ctx, const double* displacement, int n_spheres);
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_motion_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples,
                         double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                         double* rgb64f, uint32_t* raycount2, void* stream);
/* Synchronous host-buffer convenience, as rt_render_soft: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the frame.  *stats as rt_render_soft. */
int rt_render_motion(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam, int width,
                     int height, int depth, int samples, double aperture, double light_size, double shutter,
                     float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- adaptive sampling of the lens, soft-shadow and motion-blur renders (ABI 10: new symbols only) ------------- */
/* Two levels of rt_render_motion_dev: every pixel gets S_lo x S_lo samples, and the pixels whose coarse samples disagree
 * or that stand on a contrast edge of the coarse frame get S_hi x S_hi.  Deterministic, and defined entirely by
 * rt_render_motion_dev.  For a full width x height frame, S_lo = `samples_lo` <= S_hi = `samples_hi`, both in
 * {1, 2, 4, 8}, T = `threshold` in {-1, .., 255}, and A, R, F and the displacements as for rt_render_motion_dev:
 *  1. Coarse frame.  C is the frame rt_render_motion_dev(cam, width, height, depth, S_lo, A, R, F) writes; c(a, b),
 *     0 <= a, b < S_lo, are a pixel's samples before the reduction; q(v) is the RGBA8 byte of a colour value,
 *     floor(clamp(v, 0, 1) * 255 + 0.5) of the FP64 value, NaN -> 0.
 *  2. Criterion.  Pixel (i, j) is REFINED iff (a) or (b):
 *     (a) spread: for some channel, the maximum over (a, b) of q(c(a, b)) minus the minimum over (a, b) is > T;
 *     (b) contrast: rule 2 of rt_render_adaptive_dev on the bytes q(C): some in-frame 4-neighbour differs by more than
 *         T in some channel.
 *     Both read coarse data only, never a refined value.  T = -1 refines every pixel, a 1 x 1 frame included ((a) holds:
 *     rt_render_adaptive_dev refines nothing there); T = 255 refines nothing; with S_lo = 1, (a) never holds for T >= 0.
 *  3. Value.  A refined pixel has exactly the value and the two counters rt_render_motion_dev(.., S_hi, A, R, F) gives
 *     it, an unrefined pixel exactly those of C.  The outputs derive from that value as in rt_render_ss_dev rules 3-5.
 *     `refined`: a nullable uint8 image, width x height, 1 for a refined pixel and 0 otherwise.
 *  4. Pins that follow, with NO shortcut in the implementation (the same three passes run for every argument): T = 255
 *     writes C; T = -1 writes the S_hi frame; S_lo = S_hi writes that frame for every T; F = 0, R = 0 and A = 0 reduce
 *     the frame to rt_render_soft_dev's, rt_render_dof_dev's and rt_render_ss_dev's as for rt_render_motion_dev; and
 *     A = R = F = 0, S_lo = 1, T >= 0 on a frame larger than 1 x 1 writes exactly what rt_render_adaptive_dev(S_hi, T)
 *     writes, `refined` included.
 *  5. rt_render_lens_adaptive_dev: full frames only.  Asynchronous on `stream`, no allocation and no host
 *     synchronisation, so the call may be captured in a hipGraph.  No per-view state: it reads the scene and motion
 *     records and never writes them, and the cone masks, the level masks and the tile order stay intact.  Three passes:
 *     the coarse render into the caller's outputs, which also leaves one spread byte per pixel in the workspace; a
 *     classification pass that writes `refined` and compacts the refined pixels into a work list (whose order is
 *     unspecified and influences no output); a refine pass over the list, S_hi x S_hi lanes per pixel reduced in the
 *     wave, which overwrites the refined pixels in every requested output.
 *     `workspace`: workspace_bytes >= rt_lens_adaptive_workspace_bytes(...) of device memory, 16-byte aligned, owned by
 *     the caller and used by one call at a time.  It holds the counter, the work list, the spread bytes and room for
 *     the coarse RGBA8 image (used when `rgba8` is null); its first uint32 holds the number of refined pixels once the
 *     call's work is done.
 *  6. RT_EINVAL (rt_last_error names the argument), and no pixel written, for a sample count outside {1, 2, 4, 8},
 *     S_lo > S_hi, a `threshold` outside -1 .. 255, rt_render_motion_dev's checks of A, R and F, a null, misaligned or
 *     too small `workspace`, and an int32 overflow of either sample-grid camera.
 *  7. Not offered: row bands, multi-GPU and the packed or asynchronous host paths; more than two levels; a dilation of
 *     the mask; jittered samples; a threshold per effect. */
/* Host only: the bytes of device workspace rt_render_lens_adaptive_dev needs for a width x height frame.  RT_EINVAL for
 * a null pointer or a bad size. */
int rt_lens_adaptive_workspace_bytes(int width, int height, size_t* bytes);
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_lens_adaptive_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples_lo,
                                int samples_hi, int threshold, double aperture, double light_size, double shutter,
                                float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, uint8_t* refined,
                                void* workspace, size_t workspace_bytes, void* stream);
/* Synchronous host-buffer convenience, as rt_render_motion: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the frame with the context's own workspace.  *n_refined (nullable): the
 * number of refined pixels n.  *stats from the summed raycount2: primary_rays = (width * height - n) * S_lo * S_lo +
 * n * S_hi * S_hi. */
int rt_render_lens_adaptive(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                            int width, int height, int depth, int samples_lo, int samples_hi, int threshold,
                            double aperture, double light_size, double shutter, float* rgba32f, uint8_t* rgba8,
                            double* rgb64f, uint8_t* refined, rt_stats* stats, uint64_t* n_refined);

/* ---- jittered sampling of the lens, soft-shadow and motion-blur renders (ABI 10: new symbols only) ------------- */
/* Stratified jittered sampling: rt_render_motion_dev with each of the S x S samples of a pixel moved, in every one of
 * its seven dimensions, to one of J sub-positions of its stratum, chosen by a hash of the sample and a seed.  The regular
 * grid's banding (a penumbra of S S steps, a streak of S S copies, the same in every pixel) becomes noise at the same ray
 * count.  Jitter is QUANTISED: every jittered position is a point of the regular grid J times finer than the sample
 * grid, so every quotient below is exact and J = 1 is the existing render.  Deterministic, and defined entirely by
 * rt_set_scene and rt_trace_rays_dev on scenes and rays this text spells out.  For a full width x height frame,
 * S = `samples` in {1, 2, 4, 8}, J = `jitter` in {1, 2, 4, 8, 16}, `seed` any uint32, and A, R, F and the displacements as
 * for rt_render_motion_dev:
 *  1. Hash.  fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16, all uint32 and
 *     wrapping.  Sample (a, b) of pixel (i, j) has the sample-grid coordinates (I, Jr) = (S i + a, S j + b) and the index
 *     q = Jr * (S * width) + I (below 2^31: the size check); its word is w = fmix32(fmix32(q) ^ seed).
 *     fmix32(0) = 0, fmix32(1) = 0x514e28b7, fmix32(fmix32(5) ^ 7) = 0xe80274bd.
 *  2. Levels.  Dimension d in 0 .. 6 takes nibble d of w: k_d = ((w >> 4 d) & 15) >> (4 - log2 J), in 0 .. J - 1.
 *     d = 0, 1: sub-pixel x, y; 2, 3: lens x, y; 4, 5: light x, z; 6: time.  J = 1 gives k_d = 0 for every d.
 *  3. Ray end.  The fine camera cam_f has eye, look_at and up of `cam`, pitch_f = cam.pitch / (S J) (exact) and
 *     bottom_f = S J bottom.  The ray ends at the primary-ray end point of cam_f (the camera comment's formula) for the
 *     fine pixel (J I + k_0, J Jr + k_1).
 *  4. Ray start.  e = (eye + (A * t_x) * right) + (A * t_y) * up',  t_x = (double)(2 (J a + k_2) + 1 - S J) / (double)(S J),
 *     t_y likewise from b and k_3; the operation order of rt_render_dof_dev rule 2.
 *  5. Lights.  (L.x + (R * g_x), L.y, L.z + (R * g_z)), g_x and g_z by the formula of t_x from (a, k_4) and (b, k_5).
 *  6. Time.  sigma = F * u,  u = (double)(2 (J n + k_6) + 1 - S S J) / (double)(S S J),  n = a + S b; sphere centres
 *     follow rt_render_motion_dev rule 3.  |t|, |g|, |u| < 1 as on the regular grid.
 *  7. Value.  The colour and the counters of a sample are what rt_trace_rays_dev gives its ray after rt_set_scene of the
 *     scene of rules 5 and 6.  Reduction and outputs follow rt_render_ss_dev rules 3-5 exactly.
 *  8. Pins that follow, with NO shortcut in the implementation (all run the same kernel): J = 1 with any seed writes
 *     exactly what rt_render_motion_dev writes, images and counters; with A = R = F = 0, sample (a, b) of pixel (i, j) is
 *     pixel (J I + k_0, J Jr + k_1) of the S J width x S J height frame rt_render_dev renders with cam_f; equal arguments
 *     give equal bytes, call after call and under graph replay.
 *  9. rt_render_jitter_dev: full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host
 *     synchronisation, so the call may be captured in a hipGraph.  No per-view state; the scene and motion records are
 *     read, never written.
 * 10. RT_EINVAL (rt_last_error names the argument) for rt_render_motion_dev's checks, a `jitter` outside
 *     {1, 2, 4, 8, 16}, and an int32 overflow of the fine camera: of S J bottom_x or S J bottom_y, of S J width or
 *     S J height, or of a fine pixel's coordinate plus bottom_f.  A rejected call writes no pixel.
 * 11. Not offered: jitter in rt_render_lens_adaptive_dev, rt_render_adaptive_dev and rt_render_ss_dev; disc lenses;
 *     blue-noise or low-discrepancy sequences; a seed per effect; the rand()-driven jitter of the app (rt_render_screen
 *     stays the faithful one).
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, R = 40, one sphere moving by |d| = 40, F = 1, A = 0, RGBA32F + RGBA8,
 * tools/bench_jitter.py, profiles/jitter/bench_jitter.json): S = 2 147.5 us at J = 1 and 149.7 us at J = 16 per frame
 * against 139.6 us for rt_render_motion_dev (1.06 x and 1.07 x); S = 4 600.5 us and 602.7 us against 570.9 us (1.05 x and
 * 1.06 x).  The cost is the kernel's own per-lane work, present at J = 1; the lanes' separate light points and times at
 * J = 16 add 1.5 % and 0.4 %.  Other scenes, depths, apertures and motions: not measured. */
/* Host only: levels[d] = k_d of sample (I, Jr), 0 <= I < S width, of a width-pixel-wide frame, by the functions the
 * kernel calls.  RT_EINVAL for a null pointer, samples or jitter outside their sets, and a sample outside a frame of at
 * most 2^31 samples. */
int rt_jitter_sample(int width, int samples, int jitter, uint32_t seed, int I, int Jr, int32_t levels[7]);
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_jitter_dev(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, int samples, int jitter,
                         uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f,
                         uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream);
/* Synchronous host-buffer convenience, as rt_render_motion: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the frame.  *stats as rt_render_motion. */
int rt_render_jitter(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam, int width,
                     int height, int depth, int samples, int jitter, uint32_t seed, double aperture, double light_size,
                     double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- camera motion blur: a moving eye and look-at point (ABI 10: new symbols only) ------------------------------ */
/* rt_render_jitter_dev with the camera itself moving during the exposure: a pan, a dolly, a crane or an orbit streaks
 * the whole frame the way a moving sphere streaks its own image.  Every sample has the camera of its own shutter time,
 * eye, look-at point and basis.  Deterministic, and defined entirely by rt_set_scene and rt_trace_rays_dev on scenes and
 * rays this text spells out.  For a full width x height frame, S, J, `seed`, A, R, F and the displacements as for
 * rt_render_jitter_dev, and `motion` the half-extents of the camera's move during the exposure, in world units:
 *  1. Everything of rt_render_jitter_dev holds unchanged: the hash, the levels k_0 .. k_6, the fine camera's pitch_f and
 *     bottom_f, the lens quotients t, the light quotients g, the time sigma = F * u with k_6, the sphere centres, the
 *     reduction tree and the outputs.  J = 1 gives the regular grid of rt_render_motion_dev.
 *  2. Camera of a sample.  A sample at time sigma has the camera
 *         eye_s[c] = eye[c] + (sigma * motion.eye[c]),   look_s[c] = look_at[c] + (sigma * motion.look_at[c])
 *     per component: one multiplication, then one addition; up, pitch and bottom are `cam`'s.  Its basis is the camera
 *     comment's formula on those values in the reference's operation order (MySdlApplication.cpp:1270-1277,
 *     Point::normalize :174-175): LD = look_s - eye_s, right_s = normalize(LD x up), up'_s = normalize(right_s x LD);
 *     normalize(v): l = sqrt(v.x v.x + v.y v.y + v.z v.z), summed left to right, then three IEEE divisions by l;
 *     a x b = (a.y b.z - b.y a.z, a.z b.x - a.x b.z, a.x b.y - a.y b.x).  rt_camera_at returns exactly this camera: eye
 *     and look_at moved, everything else copied (`out` may be `cam`; motion NULL: no move); RT_EINVAL for a null
 *     pointer, a non-finite sigma or a non-finite displacement.
 *  3. Ray.  It ends at (look_s + (pitch_f * (double)(fi + bottom_fx)) * right_s) + (pitch_f * (double)(fj + bottom_fy)) *
 *     up'_s, (fi, fj) = (J I + k_0, J Jr + k_1), and starts at (eye_s + (A * t_x) * right_s) + (A * t_y) * up'_s: rules 3
 *     and 4 of rt_render_jitter_dev with the sample's own camera.
 *  4. Value.  The colour and the counters of a sample are what rt_trace_rays_dev gives that ray on the scene of
 *     rt_render_jitter_dev rules 5 and 6.
 *  5. Pins that follow, with NO shortcut in the implementation (one kernel runs for every argument): motion NULL or all
 *     zero writes exactly what rt_render_jitter_dev writes, images and counters — with J = 1 rt_render_motion_dev's
 *     output, and down the chain rt_render_soft_dev's, rt_render_dof_dev's, rt_render_ss_dev's and rt_render_dev's; so
 *     does F = 0 with any motion.  The pins assume that no eye or look_at component is -0.0.  With J = 1, A = R = 0
 *     and frozen spheres, sample (a, b) of pixel (i, j) is pixel (S i + a, S j + b) of the S width x S height frame
 *     rt_render_dev renders with rt_camera_supersample(rt_camera_at(cam, motion, sigma_n), S), n = a + S b.
 *  6. rt_render_shutter_dev: full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host
 *     synchronisation, so the call may be captured in a hipGraph.  No per-view state; the scene and motion records are
 *     read, never written, and the cone masks, the level masks and the tile order stay intact.  The camera motion is an
 *     argument of the call, not state of the context.
 *  7. RT_EINVAL (rt_last_error names the argument) for every check of rt_render_jitter_dev, a non-finite displacement in
 *     `motion`, and a camera at sigma in {-F, 0, +F} whose right or up' is not finite (a view direction parallel to up
 *     at an end or the middle of the exposure).  A rejected call writes no pixel.  A basis that degenerates strictly
 *     between those times is the caller's responsibility: the sample's value is still rule 4's.
 *  8. Not offered: a moving up, curved or accelerated paths, moving lights, board and meshes, camera motion in
 *     rt_render_lens_adaptive_dev, a shutter per effect.  rt_render_multi, the packed and asynchronous host paths and the
 *     drop-in draw() keep a frozen camera.
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, R = 40, one sphere moving by |d| = 40, F = 1, A = 0, RGBA32F + RGBA8,
 * tools/bench_shutter.py, profiles/shutter/bench_shutter.json; against rt_render_jitter_dev with the same arguments in
 * the same run): a zero motion costs 1.20 x at every size (S = 2: 179.0 us at J = 1 and 181.3 us at J = 16 against 148.2 us
 * and 150.5 us; S = 4: 728.5 us and 731.2 us against 604.2 us and 607.2 us), a crane of |eye move| = 40 1.32 x - 1.35 x
 * (S = 2: 195.4 us and 203.5 us; S = 4: 811.9 us and 818.1 us).  The 20 % are the issue slots of the 141 FP64 instructions
 * of the per-lane basis (two IEEE square roots, six IEEE divisions) on a kernel that is FP64-issue bound and executes
 * about 700 per sample at this depth; the crane's further 9 - 12 % come with fewer rays, not more (likely the wave-level
 * sphere culling, which widens with the spread of a wave's ray origins; not measured).  profiles/shutter/README.md has
 * the counts.  Other scenes, depths, apertures and motions: not measured. */
typedef struct rt_camera_motion {   /* half-extents of the camera's move during the exposure, world units */
    double eye[3];
    double look_at[3];
} rt_camera_motion;
/* Host only: the camera of rule 2 at time sigma. */
int rt_camera_at(const rt_camera* cam, const rt_camera_motion* motion, double sigma, rt_camera* out);
/* Device pointers, each output nullable, width * height pixels. */
int rt_render_shutter_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width, int height,
                          int depth, int samples, int jitter, uint32_t seed, double aperture, double light_size,
                          double shutter, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                          void* stream);
/* Synchronous host-buffer convenience, as rt_render_jitter: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the frame.  *stats as rt_render_jitter. */
int rt_render_shutter(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                      const rt_camera_motion* motion, int width, int height, int depth, int samples, int jitter,
                      uint32_t seed, double aperture, double light_size, double shutter, float* rgba32f,
                      uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- progressive accumulation: many jittered passes summed in the kernel (ABI 10: new symbols only) -------------- */
/* rt_render_shutter_dev takes at most 8 x 8 samples per pixel at one of 16 sub-positions per dimension: one noisy
 * estimate.  rt_render_accum_dev adds the frames of K consecutive seeds to a caller-owned sum, in a fixed order, and
 * writes the mean of all passes so far: 256 or 1024 samples per pixel in one call, or a preview that sharpens call after
 * call.  Every value is a fixed-order sum of frames rt_render_shutter_dev defines.  For n0 = `first_pass`, K = `passes`
 * >= 1, and every other argument as for rt_render_shutter_dev:
 *  1. Pass.  Pass p, n0 <= p < n0 + K, has the value v_p: what rt_render_shutter_dev writes to rgb64f with the same
 *     arguments and the seed (seed + p) mod 2^32 (after the reduction tree and the product with 1 / (S S)); its counters
 *     are that frame's raycount2.
 *  2. Sum.  Per channel, in FP64, one IEEE addition per pass, left to right:
 *       n0 = 0: `accum` is NOT READ (it may be uninitialised); acc = v_0, then acc = acc + v_p for p = 1 .. K - 1;
 *       n0 > 0: acc = accum, then acc = acc + v_p for p = n0 .. n0 + K - 1;
 *     accum <- acc.  The order is part of the contract: summing the call's passes first and adding that sum to `accum`
 *     is another value (on the oracle it differs in 30 of 209 pixels for n0 = 2, K = 3 of the tests' case).
 *  3. Mean and outputs.  m = acc / (double)(n0 + K), one IEEE division per channel — not a product with a reciprocal,
 *     which differs (26 and 37 of 209 pixels at K = 3 and K = 7 of the tests' case).  rgb64f is m; rgba32f and rgba8 derive from m by
 *     rt_render_ss_dev rule 4; raycount2 is the sum of the K passes' counters of THIS call only, uint32 and wrapping.  A
 *     channel with a NaN pass stays NaN in `accum` from then on (which NaN: unspecified); its rgba8 byte is 0.
 *  4. Pins that follow, with NO shortcut in the implementation (one kernel runs for every argument): n0 = 0, K = 1 writes
 *     exactly the images and counters of rt_render_shutter_dev with `seed`, and `accum` equals its rgb64f — so every pin
 *     of the chain holds through it (rt_render_jitter_dev, _motion_dev, _soft_dev, _dof_dev, _ss_dev, and the plain frame
 *     at S = J = 1).  A call (0, a) followed by a call (a, b) on the same `accum` leaves the same bytes in `accum` and
 *     in every image as one call (0, a + b), and the two calls' counters sum to the one call's.  Equal arguments and an
 *     equal `accum` give equal bytes, call after call and under graph replay.
 *  5. rt_render_accum_dev: full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host
 *     synchronisation, so the call may be captured in a hipGraph.  No per-view state; the scene and motion records are
 *     read, never written.  The host may split a call into several launches of at most L passes each, so that one
 *     launch on a shared GPU stays short; L is 4 (below) unless RT_ACCUM_MAX_PASSES (read by rt_ctx_create, 1 .. 65536)
 *     says otherwise.  Rule 2 makes the split invisible: the images are the same bytes under every value.
 *  6. RT_EINVAL (rt_last_error names the argument), with no byte of `accum` or of any image written, for every check of
 *     rt_render_shutter_dev, a null `accum`, `passes` < 1 or above 65536, and `first_pass + passes` above 2^31.
 *  7. Not offered: accumulation for rt_render_lens_adaptive_dev; rt_rows (a rectangle of the frame, and with it a
 *     split over GPUs or tiles, is rt_render_accum_window_dev below); the packed and group paths; weights other than 1.  Jitter is quantised, so the mean converges to the regular grid
 *     S J times finer per dimension, not to the continuous integral.  A per-pixel variance and stopping rule is a call
 *     of its own: rt_render_converge_dev (below), which sums in this call's order.
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, R = 40, one sphere moving by |d| = 40, F = 1, A = 0, crane of
 * |eye move| = 40, J = 16, RGBA32F + RGBA8, tools/bench_accum.py, profiles/accum/bench_accum.json; one
 * rt_render_shutter_dev frame in the same run: 54 us at S = 1, 204 us at S = 2, 817 us at S = 4): one call of K passes
 * takes 229 us (K = 4) and 906 us (K = 16) at S = 1, 888 us and 3508 us at S = 2 — 1.05 x - 1.09 x the single frame per
 * pass; against K rt_render_shutter_dev calls into rgb64f with a separate FP64 accumulation per pass and one division
 * and conversion at the end it is 0.49 x and 0.65 x at S = 1, 0.84 x and 0.95 x at S = 2, and against K calls of one pass
 * each 0.81 x - 0.86 x; all three give the same bytes.  S = 4, K = 4, one launch: 3.58 ms, which is why L = 4.  The
 * per-pass excess is the loop's own: the kernel arguments outlive the register file across the trace (64 scalar
 * registers kept in vector lanes in the depth-1 opaque instance) and the running sums wait in LDS; profiles/accum/
 * README.md has the counts.  Other scenes, depths and motions: not measured. */
/* Device pointers; `accum`: width * height * 3 doubles, required; each output nullable, width * height pixels. */
int rt_render_accum_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width, int height,
                        int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes,
                        double aperture, double light_size, double shutter, double* accum, float* rgba32f,
                        uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream);
/* Synchronous host-buffer convenience, as rt_render_shutter: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the passes.  `accum` is a host buffer of width * height * 3 doubles, read
 * when first_pass > 0 and written on success.  *stats as rt_render_shutter, over all passes of the call. */
int rt_render_accum(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                    const rt_camera_motion* motion, int width, int height, int depth, int samples, int jitter,
                    uint32_t seed, uint32_t first_pass, int passes, double aperture, double light_size, double shutter,
                    double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats);

/* ---- converging accumulation: a pixel stops once its standard error is low (ABI 10: new symbols only) ------------ */
/* rt_render_accum_dev gives every pixel the same K passes, though most pixels of a frame never change from pass to pass
 * and the rest stays noisy for dozens.  rt_render_converge_dev accumulates in rt_render_accum_dev's fixed order, keeps a
 * per-pixel sum of squares and pass count beside the sum, and stops giving a pixel passes once the estimated standard
 * error of its mean is at most a tolerance in every channel: a budget of 64 or 256 passes that only the noisy pixels use.
 * Every argument is as for rt_render_accum_dev, except that `first_pass` is gone and that `passes` = K >= 1 is a budget
 * per pixel and call, `min_passes` = M and `tolerance` = E.
 *  State.  Three caller-owned device buffers hold the state (acc, sq, n) of a pixel: `accum`, 3 doubles per pixel;
 *     `accum2`, 3 doubles per pixel, the sums of squares; `count`, one uint32 per pixel.  All three are required.  A new
 *     sum starts from a zeroed `count`; where n = 0, `accum` and `accum2` are NOT READ (they may be uninitialised).
 *     Every pixel is independent of every other.
 *  1. Pass.  v_p is what rt_render_shutter_dev writes to rgb64f for this pixel with the seed (seed + p) mod 2^32; its
 *     counters are that frame's raycount2 words for the pixel.  The pass a pixel receives next is the pass with the
 *     number of its own n: a pixel's passes are always 0, 1, 2, ..., without a gap, whatever happens to other pixels.
 *  2. Step, up to K times per call: if stopped(acc, sq, n), end.  Otherwise v = v_n and, per channel, in FP64, one IEEE
 *     operation per operator, no contraction:
 *       n = 0: acc = v, sq = v * v;
 *       n > 0: acc = acc + v, sq = sq + (v * v) — one multiplication, then one addition; a fused multiply-add gives
 *              other bits (on the oracle 90 of 627 channel values differ after 6 passes of the tests' main case);
 *     then n = n + 1.
 *  3. Stop rule.  stopped(acc, sq, n) is true iff n = 2^31, or n >= M and no channel has d > lim, where
 *       d = sq - (acc * acc) / (double)n            (a multiplication, a division, a subtraction),
 *       lim = (E * E) * ((double)n * (double)(n - 1))   (three multiplications):
 *     the estimated standard error of the mean is at most E.  A NaN d does not hold a pixel back (the comparison is
 *     false).  The rule is evaluated before every pass, at the start of a call too, so a pixel that was stopped under a
 *     loose E resumes, with its next pass, when a later call gives a smaller E or a larger M.
 *  4. Outputs, written for every pixel whether or not it received a pass in this call: the state is written back;
 *     m = acc / (double)n, one IEEE division (n >= 1 after any call); rgb64f, rgba32f and rgba8 derive from m by
 *     rt_render_ss_dev rule 4; raycount2 holds the sums of the counters of the passes the pixel received in THIS call
 *     (0, 0 for a pixel that received none); `active`, a nullable device uint32, holds the number of pixels for which
 *     stopped() is false on the final state.
 *  5. Pins that follow, with NO shortcut in the implementation (one kernel runs for every argument).  With M > K and a
 *     zeroed `count`: `accum`, every image and raycount2 hold exactly the bytes of rt_render_accum_dev(first_pass 0,
 *     passes K), `count` = K everywhere and `active` = width * height — so K = 1 is rt_render_shutter_dev and every pin
 *     of the chain holds through it.  For any arguments a pixel with count n has in `accum` exactly what
 *     rt_render_accum_dev(0, n) leaves there.  A call of a passes followed by a call of b passes, with equal M and E,
 *     leaves the same bytes in all three state buffers and in every image as one call of a + b, and the two calls'
 *     counters sum to the one call's; the host's split into launches of at most L passes (rt_render_accum_dev rule 5,
 *     RT_ACCUM_MAX_PASSES) is invisible for the same reason.  Equal arguments and equal state give equal bytes, call
 *     after call and under graph replay.
 *  6. Full frames only (no rt_rows).  Asynchronous on `stream`, no allocation and no host synchronisation; capturable
 *     in a hipGraph: one stream, a straight line of nodes, the reset of `active` a memset node of the call.  No per-view
 *     state; the scene and motion records are read, never written.
 *  7. RT_EINVAL (rt_last_error names the argument), with no byte written, for every check of rt_render_shutter_dev, a
 *     null `accum`, `accum2` or `count`, `passes` outside 1 .. 65536, `min_passes` outside 2 .. 2^31, and a `tolerance`
 *     that is negative, NaN or infinite.
 *  8. Not offered: a relative or perceptual tolerance; a tolerance per channel; compaction of the live tiles into a
 *     work list; a stopping rule in rt_render_lens_adaptive_dev; rt_rows (a rectangle of the frame is
 *     rt_render_converge_window_dev below); the packed and group paths.
 * One wave keeps its 8 x 8 tile of the sample grid for the whole launch, as in rt_render_accum_dev, and leaves its pass
 * loop as soon as all of its pixels have stopped; a wave whose pixels had all stopped before the launch traces nothing.
 * The lanes of a stopped pixel in a live wave trace and discard.
 * Measured: MI355X, c2 1920 x 1080 output, depth 1, the scene of rt_render_accum_dev's figures, J = 16, K = 64, M = 4,
 * RGBA32F + RGBA8, tools/bench_converge.py, profiles/converge/bench_converge.json; rt_render_accum_dev(0, 64) in the
 * same run: 3.63 ms at S = 1, 14.05 ms at S = 2. With M = 65, so that nothing stops, the call takes 4.20 ms and 15.81
 * ms, 1.16 x and 1.13 x: the price of the second sum and of the rule (at S = 2 8 % per launch: 7.5 % more vector
 * instructions, 52 instead of 24 bytes of state per pixel; and 0.7 ms in the last launch, where every wave adds to
 * `active`). From a zeroed count it takes 3.34 ms (E = 1 / 255) and 3.23 ms (4 / 255) at S = 1, 10.57 ms and 8.42 ms
 * at S = 2: 0.92 x, 0.89 x, 0.75 x and 0.60 x rt_render_accum_dev, while tracing 0.51, 0.48, 0.46 and 0.35 of the
 * wave-passes (0.42, 0.36, 0.39, 0.25 of the pixel-passes); the gap is stopped lanes in live waves, the waves of all
 * 16 launches that only load their state and leave, and the live waves being the costly ones of the frame. The RMS
 * difference to a 256-pass mean doubles against the full budget (0.0134 against 0.0072 at S = 2, E = 1 / 255): with M
 * = 4 a pixel whose first four passes agree stops at once. profiles/converge/README.md has the records. Other scenes,
 * depths and motions: not measured. */
/* Device pointers; `accum`, `accum2`: width * height * 3 doubles, `count`: width * height uint32, all required; each
 * output and `active` nullable. */
int rt_render_converge_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width, int height,
                           int depth, int samples, int jitter, uint32_t seed, int passes, uint32_t min_passes,
                           double tolerance, double aperture, double light_size, double shutter, double* accum,
                           double* accum2, uint32_t* count, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                           uint32_t* raycount2, uint32_t* active, void* stream);
/* Synchronous host-buffer convenience, as rt_render_accum: rt_set_scene(scene), rt_set_motion(displacement,
 * scene->n_spheres) (NULL: no motion), then the passes.  `accum`, `accum2` and `count` are host arrays, read and written
 * on success.  *n_active (nullable): what `active` holds.  *stats as rt_render_accum, over the passes this call traced:
 * its primary rays are S S times the growth of the sum of `count`. */
int rt_render_converge(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                       const rt_camera_motion* motion, int width, int height, int depth, int samples, int jitter,
                       uint32_t seed, int passes, uint32_t min_passes, double tolerance, double aperture,
                       double light_size, double shutter, double* accum, double* accum2, uint32_t* count,
                       float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats, uint64_t* n_active);

/* ---- windows of the accumulating and converging renders (ABI 10: new symbols only) ------------------------------- */
/* rt_render_accum_dev and rt_render_converge_dev render whole frames, and a camera shifted to a region does not give
 * the region's bytes under jitter: the sample key is Jr (S width) + I in the coordinates of the frame being rendered.
 * The window calls render one rectangle of the width x height frame with the frame's own bytes — what a rank of a
 * multi-GPU split or a tile of a frame whose FP64 state does not fit at once owns, or the region a viewer refines.
 * Every argument is as for the un-windowed call; `win` says which pixels, and how the buffers are laid out. */
typedef struct rt_window {      /* a rectangle of the width x height output frame, in output pixels, j = 0 at the bottom */
    int32_t x0, y0;             /* frame pixel of window pixel (0, 0) */
    int32_t width, height;      /* >= 1; x0 + width <= frame width, y0 + height <= frame height */
    int32_t stride;             /* >= width: window pixel (i, j) is element j * stride + i of every per-pixel buffer */
} rt_window;
/* Every buffer pointer points at window pixel (0, 0).  An element is the buffer's own per-pixel unit: 3 doubles for
 * `accum`, `accum2` and rgb64f, one uint32 for `count`, 4 floats for rgba32f, 4 bytes for rgba8, 2 uint32 for raycount2;
 * one stride serves all buffers.  stride = win.width is a dense window; stride = the frame's width with the pointers
 * offset to the window's origin is a window in place inside full-frame buffers.
 *  1. Value.  For every window pixel (i, j) the state (`accum`; for converge also `accum2` and `count`), the mean, the
 *     three images and the counters are exactly what the un-windowed call with the same arguments writes for frame
 *     pixel (x0 + i, y0 + j).  In particular the sample key is the full frame's: rt_jitter_sample(S width, ...,
 *     I = S (x0 + i) + a, Jr = S (y0 + j) + b) with the FRAME's width, not the window's.
 *  2. Nothing else is touched.  Elements outside the window are neither read nor written: the gap between the rows when
 *     stride > win.width, and everything outside an in-place window.
 *  3. `active` (converge) holds the number of the WINDOW's pixels that are not stopped on the final state.
 *  4. Whole-frame pin.  With win = {0, 0, width, height, width} every byte equals the un-windowed call's.  There is no
 *     shortcut in either direction: the un-windowed entry points run the kernels they always ran, the window calls run
 *     theirs for every window.  A state written by either call can be continued by the other.
 *  5. Tiling pin.  Windows that partition the frame, rendered in any order into full-frame buffers (stride = width,
 *     pointers offset to each window's origin), leave the bytes of one un-windowed call in every buffer, and their
 *     `active` values sum to its `active`.  The split-call rules hold per window: (0, a) then (a, b) equals (0, a + b);
 *     the host's launch split (RT_ACCUM_MAX_PASSES) stays invisible; a loosely stopped window resumes under a smaller E.
 *     One pass from pass 0 on a window is that rectangle of rt_render_shutter_dev's frame, so the window calls give
 *     windows of every sampled render of the chain.
 *  6. No alignment rule: any x0, y0, width and height.  Waves tile the window from its own origin, so a wave holds other
 *     pixels than the full frame's waves do; a lane's value does not depend on the other lanes' rays
 *     (rt_render_converge_dev), so the bytes are the same.
 *  7. RT_EINVAL (rt_last_error names `window`), with no byte written, for a null `win`, a negative x0 or y0, a width or
 *     height below 1, a window that leaves the frame, stride < win.width, and every check of the un-windowed call.
 *  8. Asynchronous on `stream`, no allocation and no host synchronisation; capturable in a hipGraph, the reset of
 *     `active` a memset node of the call.  No per-view state.
 *  9. Not offered: windows of rt_render_lens_adaptive_dev; rt_rows; the packed and group paths.  A list of windows in
 *     one launch is rt_render_accum_windows_dev and rt_render_converge_windows_dev (below).
 * The kernels are rt_accum_kernel and rt_converge_kernel with the lane's sample formed from the window's sample origin;
 * the host folds the window into five words and moves the pointers, and every instance keeps its parent's waves per
 * SIMD (profiles/window/resource_usage.txt).
 * Measured (MI355X, c2 1920 x 1080 output, depth 1, the scene of rt_render_accum_dev's figures, J = 16, accum (0, 16) and
 * converge K = 64, M = 4, E = 1 / 255, RGBA32F + RGBA8, tools/bench_window.py, profiles/window/bench_window.json, every
 * leg's bytes checked equal first; the un-windowed calls in the same run: 0.91 and 3.34 ms at S = 1, 3.53 and 10.56 ms at
 * S = 2): the whole-frame window takes 1.014 x and 1.005 x (S = 1), 1.011 x and 1.008 x (S = 2) the un-windowed call, above
 * the spreads at S = 2 only.  The frame as 2 / 4 / 8 strips of whole rows, one call each: 1.17 x / 1.47 x / 1.70 x (accum)
 * and 1.20 x / 1.60 x / 1.74 x (converge) at S = 1, 1.05 x / 1.14 x / 1.25 x and 1.07 x / 1.20 x / 1.34 x at S = 2; as 4 x 4
 * tiles 2.57 x, 3.02 x, 1.40 x, 1.71 x: 22 - 47 us of ramp and drain per extra launch.  A 960 x 540 window at (3, 5) is not
 * slower than one at (8, 8) (0.94 x - 0.99 x).  profiles/window/README.md has the records.  Other scenes, depths and
 * motions: not measured. */
int rt_render_accum_window_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width, int height,
                               const rt_window* win, int depth, int samples, int jitter, uint32_t seed,
                               uint32_t first_pass, int passes, double aperture, double light_size, double shutter,
                               double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f, uint32_t* raycount2,
                               void* stream);
int rt_render_converge_window_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width,
                                  int height, const rt_window* win, int depth, int samples, int jitter, uint32_t seed,
                                  int passes, uint32_t min_passes, double tolerance, double aperture, double light_size,
                                  double shutter, double* accum, double* accum2, uint32_t* count, float* rgba32f,
                                  uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, uint32_t* active, void* stream);
/* Synchronous host-buffer conveniences, as rt_render_accum and rt_render_converge: the host arrays are addressed with
 * the window's stride as the device buffers are, and only the window's rows move (the state up, everything back).
 * *n_active and *stats are the window's. */
int rt_render_accum_window(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                           const rt_camera_motion* motion, int width, int height, const rt_window* win, int depth,
                           int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes, double aperture,
                           double light_size, double shutter, double* accum, float* rgba32f, uint8_t* rgba8,
                           double* rgb64f, rt_stats* stats);
int rt_render_converge_window(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                              const rt_camera_motion* motion, int width, int height, const rt_window* win, int depth,
                              int samples, int jitter, uint32_t seed, int passes, uint32_t min_passes, double tolerance,
                              double aperture, double light_size, double shutter, double* accum, double* accum2,
                              uint32_t* count, float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats,
                              uint64_t* n_active);

/* ---- lists of windows of the accumulating and converging renders (ABI 10: new symbols only) ------------------------ */
/* A window call is one launch per rectangle and per launch group, and each launch pays its ramp and drain: a rank that
 * owns dozens of disjoint bands, a tile loop or a viewer refining several regions pays it per rectangle.  The list calls
 * render any set of DISJOINT windows of one frame with one launch per launch group, every pixel with the bytes of the
 * un-windowed frame.  The list lives in the context (rt_set_windows, as the motion does: rt_set_motion); the render calls
 * take exactly the un-windowed calls' arguments. */
#define RT_MAX_WINDOWS      4096
#define RT_WINDOWS_IN_PLACE 0   /* every window inside full-frame buffers: stride = frame width               */
#define RT_WINDOWS_PACKED   1   /* every window dense (stride = its width), one after the other in list order */
/* rt_window_list_plan: a pure host function (no context, no GPU) that validates a list and gives the numbers everything
 * else uses.  wins[k].stride is ignored on input: the layout decides it.
 *   offset[k]      the element index of window k's pixel (0, 0) in every per-pixel buffer (an element: rt_window above).
 *                  IN_PLACE: y0 width + x0, the stride is `width`.  PACKED: the sum of the areas of windows 0 .. k - 1,
 *                  the stride is wins[k].width.
 *   *elements      the per-pixel elements the buffers must hold.  IN_PLACE: width height.  PACKED: the sum of the areas.
 *   first_tile[k]  the number of 8 x 8-sample tiles of windows 0 .. k - 1 at `samples` = S: window k has
 *                  ceil(S w / 8) ceil(S h / 8) of them; first_tile[n] is the launch's tile count.
 * Any output pointer may be null.  RT_EINVAL (rt_last_error names the argument), with nothing written, for n < 1 or
 * n > RT_MAX_WINDOWS (`n`), an unknown `layout`, `samples` not 1, 2, 4 or 8, a bad frame size (`width`, `height`), a
 * null `wins`, a window that fails the single-window checks of rule 7 of the window calls (`window`, with its index) and
 * two windows that share a frame pixel (`window`, with both indices).  Windows that touch along an edge are disjoint.
 * Disjoint windows make both layouts' footprints disjoint: that is the whole aliasing rule. */
int rt_window_list_plan(int width, int height, int samples, const rt_window* wins, int n, int layout,
                        uint32_t* first_tile /* n + 1 */, int64_t* offset /* n */, uint64_t* elements);
/* rt_set_windows: validates the list with rt_window_list_plan, copies it into the context and uploads one device table
 * (per window: its rectangle, stride and element base, and its tile prefix for each of S = 1, 2, 4, 8, so the table does
 * not depend on S).  Synchronous: work in flight on the device is waited for first, and this is the only allocation of
 * the list calls.  n = 0 with wins = NULL clears the list.  rt_set_scene and rt_set_motion do not touch the list.  A
 * failed call leaves the previous list in force. */
int rt_set_windows(rt_ctx* ctx, int width, int height, const rt_window* wins, int n, int layout);
/* The list renders: rt_render_accum_dev's and rt_render_converge_dev's arguments, unchanged.
 *  1. Value.  For every pixel of every window of the list, rule 1 of the window calls: the bytes of the un-windowed call
 *     for that frame pixel, under the full frame's sample key.  The buffers hold `elements` elements laid out as the plan
 *     says: window k's pixel (i, j) is element offset[k] + j stride_k + i of every per-pixel buffer.
 *  2. Nothing else is touched: elements that belong to no window are neither read nor written.
 *  3. `active` (converge) is the count over all windows of the list.
 *  4. The order of the list changes nothing but the PACKED offsets.  The list {0, 0, width, height} gives the bytes of
 *     the single-window call on the whole frame and of the un-windowed call.
 *  5. As per window today: (0, a) then (a, b) equals (0, a + b); the host's launch split (RT_ACCUM_MAX_PASSES) is
 *     invisible; a loosely stopped list resumes under a smaller E; a state written by the un-windowed or the
 *     single-window calls is continued by a list call (IN_PLACE, or PACKED after moving the rows) and the other way round.
 *  6. One launch per launch group of at most RT_ACCUM_MAX_PASSES passes, whatever n is.  The grid is one-dimensional over
 *     first_tile[n] tiles (folded into grid.y above 2^20 tiles); a wave finds its window by a wave-uniform binary search
 *     of the prefix column (at most 12 steps), loads that entry once and from there runs the single-window kernel's body.
 *  7. RT_EINVAL (rt_last_error names `window`), with no byte written, when no list is set or `width`, `height` are not
 *     the list's frame; and for every check of the un-windowed call.
 *  8. Asynchronous on `stream`, no allocation and no host synchronisation; capturable in a hipGraph, the reset of
 *     `active` a memset node of the call.  A captured graph holds the table's address and the tile count of the list in
 *     force at capture: after rt_set_windows, re-capture.
 *  9. Not offered: a list produced on the device (the table's layout does not preclude it: prefixes and entries are plain
 *     device arrays); overlapping windows; lists for rt_render_lens_adaptive_dev; rt_rows; the packed and group paths.
 * Every instance keeps its parent's waves per SIMD and adds no scratch (profiles/window_list/resource_usage.txt).
 * Measured (MI355X, the window calls' c2 frames and arguments, accum (0, 16) and converge K = 64, M = 4, E = 1 / 255 at
 * S = 1 and S = 2, tools/bench_window_list.py, profiles/window_list/bench_window_list.json, every leg's bytes checked
 * equal first): one list call against one window call per rectangle takes 0.43 x / 0.36 x / 0.75 x / 0.62 x for 4 x 4 tiles
 * (accum S = 1, converge S = 1, accum S = 2, converge S = 2), 0.62 x / 0.60 x / 0.85 x / 0.79 x for 8 strips and
 * 0.125 x / 0.128 x / 0.28 x / 0.25 x for rank 0's 17 bands of 8 rows at 8 ranks, above the spreads in every cell.  Against
 * the un-windowed call the 4 x 4 tiles cost 1.108 x / 1.100 x / 1.056 x / 1.055 x and the 8 strips 1.061 x / 1.054 x /
 * 1.063 x / 1.056 x.  The list of the one whole-frame window costs 1.041 x / 1.036 x / 1.041 x / 1.040 x the window call on it:
 * not within the spreads; 1.6 % of it is in the kernel's own traced time (profiles/window_list/kernel_trace_accum_s1.csv),
 * the rest was not separated.  4096 windows of
 * 8 x 8 pixels cost 1.035 x / 1.025 x / 1.025 x / 1.025 x the one window of their region.  profiles/window_list/README.md
 * has the records.  Other scenes, depths and motions: not measured. */
int rt_render_accum_windows_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width, int height,
                                int depth, int samples, int jitter, uint32_t seed, uint32_t first_pass, int passes,
                                double aperture, double light_size, double shutter, double* accum, float* rgba32f,
                                uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, void* stream);
int rt_render_converge_windows_dev(rt_ctx* ctx, const rt_camera* cam, const rt_camera_motion* motion, int width,
                                   int height, int depth, int samples, int jitter, uint32_t seed, int passes,
                                   uint32_t min_passes, double tolerance, double aperture, double light_size,
                                   double shutter, double* accum, double* accum2, uint32_t* count, float* rgba32f,
                                   uint8_t* rgba8, double* rgb64f, uint32_t* raycount2, uint32_t* active, void* stream);
/* Synchronous host-buffer conveniences, as rt_render_accum and rt_render_converge with the list after their arguments:
 * rt_set_scene, rt_set_motion and rt_set_windows(width, height, wins, n, layout), then the render.  The host arrays are
 * laid out as the plan says, as the context's device buffers are, and only the windows' rows move (the state up,
 * everything back).  *n_active and *stats are the list's.  The list stays set in the context. */
int rt_render_accum_windows(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                            const rt_camera_motion* motion, int width, int height, int depth, int samples, int jitter,
                            uint32_t seed, uint32_t first_pass, int passes, double aperture, double light_size,
                            double shutter, double* accum, float* rgba32f, uint8_t* rgba8, double* rgb64f,
                            rt_stats* stats, const rt_window* wins, int n, int layout);
int rt_render_converge_windows(rt_ctx* ctx, const rt_scene* scene, const double* displacement, const rt_camera* cam,
                               const rt_camera_motion* motion, int width, int height, int depth, int samples, int jitter,
                               uint32_t seed, int passes, uint32_t min_passes, double tolerance, double aperture,
                               double light_size, double shutter, double* accum, double* accum2, uint32_t* count,
                               float* rgba32f, uint8_t* rgba8, double* rgb64f, rt_stats* stats, uint64_t* n_active,
                               const rt_window* wins, int n, int layout);

/* ---- packed pixel formats (ABI 5)--------------------------------------------------------------- */
/* What a frame's bytes look like in a buffer.  Rows are dense (W * bytes per pixel), j = 0 at the bottom.
 * GRAY formats hold the R channel only and are accepted only for an ACHROMATIC scene (rt_scene_achromatic):
 * there R = G = B bit for bit, since every colour term of rayTraceRay (:1223-1226, :1241-1246) is a
 * component-wise product or sum of equal components, so the packed frame expands back to exactly the RGBA
 * frame.  They cut the bytes of a frame over PCIe (rt_render_packed: glDrawPixels(..., GL_LUMINANCE, ...))
 * and over xGMI (rt_render_multi's gather: 1 B/px instead of 4). */
#define RT_PIXEL_RGBA32F 0      /* float4 (r, g, b, 1), 16 B/px (the rgba32f image of rt_render_dev) */
#define RT_PIXEL_GRAY32F 1      /* float r, 4 B/px (achromatic scenes) */
#define RT_PIXEL_RGBA8   2      /* 4 B/px (the rgba8 image of rt_render_dev) */
#define RT_PIXEL_RGB8    3      /* 3 B/px, glDrawPixels(GL_RGB) / PPM order */
#define RT_PIXEL_GRAY8   4      /* 1 B/px: the R byte of RGBA8 (achromatic scenes) */
int rt_pixel_bytes(int format, int* bytes);
/* *out = 1 when the scene is achromatic: every material term the scene's objects use (ambient, diffuse,
 * specular, transparency of the board squares when the board is present, of the sphere material when there
 * are spheres, of the tetrahedron / cube materials when such meshes are present) and every light colour has
 * three equal components (MySdlApplication.cpp:577, 583-588: the app's board, spheres and tetrahedron are; its
 * red cube is not).  Host only.  (The renders use the same test, with no transparent material, to run one-channel
 * kernel instances whose three channels are bitwise equal by construction.) */
int rt_scene_achromatic(const rt_scene* scene, int* out);
/* rt_render_dev with the float image in `float_format` (RT_PIXEL_RGBA32F / GRAY32F) and the byte image in
 * `byte_format` (RT_PIXEL_RGBA8 / RGB8 / GRAY8); each image nullable.  Same rules as rt_render_dev. */
int rt_render_dev_packed(rt_ctx* ctx, const rt_camera* cam, int width, int height, int depth, const rt_rows* rows,
                         int float_format, void* float_pixels, int byte_format, void* byte_pixels, void* stream);
/* Host-buffer frames in one format (draw()'s replacement with fewer PCIe bytes).  rt_render_packed is
 * synchronous (stats nullable, as rt_render): the render and a copy kernel that writes the frame over PCIe
 * into host_pixels, back to back on the context's render stream.  rt_render_packed_async queues the render
 * on the render stream and the frame's device-to-host copy behind it — on an SDMA engine when host_pixels is
 * page-locked (rt_host_alloc; the render stream starts the engine's copy, no CU is taken from the next render),
 * else a copy kernel on the context's copy stream — and returns at once with a ticket: the copy of frame t runs
 * beside the render of frame t+1 (three device buffers: up to two frames may be waited for behind the one being
 * queued); rt_ctx_wait(ctx, t) returns when frame t's pixels are in host_pixels (ticket 0: everything queued).
 * host_pixels must stay valid until then.  RT_COPY_MODE (read at rt_ctx_create) overrides the path for both calls:
 * 0 copy kernel on the copy stream, 1 behind the render, 3 SDMA engine. */
int rt_render_packed(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height, int depth,
                     int format, void* host_pixels, rt_stats* stats);
int rt_render_packed_async(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height,
                           int depth, int format, void* host_pixels, uint64_t* ticket);
int rt_ctx_wait(rt_ctx* ctx, uint64_t ticket);
/* Pinned (page-locked) host memory for host-buffer frames (hipHostMalloc / hipHostFree). */
int rt_host_alloc(size_t bytes, void** out);
int rt_host_free(void* p);

/* ---- reference-faithful rayTraceScreen ------------------------------- */
/* rayTraceScreen (MySdlApplication.cpp:1251-1324) exactly as the app runs it: the incremental unit-step
 * screen walk from (bottom_x, bottom_y) (cam->pitch is not used: the reference steps by the unit vectors
 * right and up'), every sample jittered by 0.5 * randomUnit() (:1148-1169, rand() arguments evaluated
 * right to left), up to 16 samples per pixel with the reference's convergence test (:1294-1311), and the
 * average colour carried from pixel to pixel (:1283).  The carry-over and the shared rand() stream make
 * the frame a serial chain; the samples are traced on the GPU in speculative chunks (each pixel's sample
 * count is predicted and a window of stream positions around the prediction is traced; the host resolves the
 * chain in order, with the continuation of the chain already queued, and restarts it where the actual stream
 * position leaves a window), so the result is the reference's, bit for bit.  The context keeps the chunks'
 * buffers between calls (≈ 14 MB of mapped host memory and a stream per buffer set, three sets in the default
 * pipeline; freed by rt_ctx_destroy); concurrent calls on one context are allowed (each beyond the first
 * allocates its own).
 * rand_kind: RT_RAND_GLIBC (glibc rand(), the reference built on Linux) or RT_RAND_MSVC (the MSVC CRT
 * LCG, the reference's own Visual Studio build); seed as given to srand (the app never calls srand: 1).
 * Host outputs, each nullable, width*height pixels, j = 0 bottom: rgb64f (the colour passed to
 * glColor3d, :1312), rgba8 (floor(clamp(c,0,1)*255+0.5)), samples (samples traced per pixel, 2..16);
 * *rand_calls = rand() calls made.  Synchronous. */
#define RT_RAND_GLIBC 0
#define RT_RAND_MSVC  1
int rt_render_screen(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height,
                     int depth, int rand_kind, uint32_t seed, double* rgb64f, uint8_t* rgba8,
                     uint8_t* samples, uint64_t* rand_calls);

/* Synchronous host-buffer convenience for draw() (MySdlApplication.cpp:1541-1563): uploads `scene` (a
 * no-op when unchanged), renders into device buffers the context keeps between calls, copies back, fills
 * *stats (ray counts summed on the device + kernel time).  Any output pointer may be NULL.  Tile-row order:
 * the first render of a view uses the identity order, the second times its tile rows, later renders
 * of the view dispatch the longest rows first (images are identical either way). */
int rt_render(rt_ctx* ctx, const rt_scene* scene, const rt_camera* cam, int width, int height,
              int depth, const rt_rows* rows, float* rgba32f, uint8_t* rgba8, double* rgb64f,
              rt_stats* stats);

/* Arbitrary rays (Line(start, end)) through the uploaded scene on the device:
 * rt_intersect_dev = g_scene.intersection (MySdlApplication.cpp:724-823) -> rt_hit per ray;
 * rt_trace_rays_dev = rayTraceRay(scene, lights, ray, color, depth) -> 3 doubles per ray. */
int rt_intersect_dev(rt_ctx* ctx, const double* starts, const double* ends, int n, rt_hit* hits,
                     void* stream);
int rt_trace_rays_dev(rt_ctx* ctx, const double* starts, const double* ends, int n, int depth,
                      double* rgb64f, uint32_t* raycount, void* stream);

/* Put gathered bands back into image order: `gathered` holds n_ranks slabs, slab r = rank r's local
 * rows (rt_local_rows rows each, slabs padded to `slab_rows` rows), `image` is height x width.
 * elem_bytes in {1,2,4,8,16,24,32}: bytes per pixel. */
int rt_unshuffle_dev(const void* gathered, void* image, int width, int height, int elem_bytes,
                     int band_height, int n_ranks, int slab_rows, void* stream);
/* rt_unshuffle_dev from packed slabs in src_format into an image in dst_format: equal formats (a plain
 * unshuffle), GRAY8 -> RGBA8, RGB8 -> RGBA8, GRAY32F -> RGBA32F (RT_PIXEL_*). */
int rt_unpack_dev(const void* gathered, void* image, int width, int height, int src_format, int dst_format,
                  int band_height, int n_ranks, int slab_rows, void* stream);

/* ---- multi-GPU: one frame's rows split over GPUs, gathered to rank 0 ---- */
/* A group of ranks: rank r renders the round-robin row bands b = r (mod n_ranks) of every frame into its
 * slab; rt_render_multi gathers the slabs to rank 0 (ncclSend / ncclRecv over xGMI) and puts the rows in
 * image order there (rt_unshuffle_dev).  Slabs and rank 0's gather buffer are double-buffered and every rank
 * renders and sends on the group's own streams, so frame f's gather overlaps frame f+1's render.
 * Each rank renders its context's scene: call rt_set_scene on every context with the same scene. */
#define RT_TRANSPORT_AUTO -1    /* RCCL when the contexts are on distinct devices, else COPY */
#define RT_TRANSPORT_RCCL  0    /* RCCL send/recv (one communicator rank per context) */
#define RT_TRANSPORT_COPY  1    /* hipMemcpyPeerAsync to rank 0 (contexts may share a device) */
#define RT_OUT_RGBA32F 1
#define RT_OUT_RGBA8   2
#define RT_COMM_ID_BYTES 128
typedef struct rt_group rt_group;
/* Bands for n_ranks: band_height 0 = auto (largest height <= 16 that gives every rank the same rows, e.g.
 * 15 for 1080 rows over 8 ranks; else 8).  *slab_rows_out (nullable) = the most rows any rank renders. */
int rt_band_plan(int height, int n_ranks, int band_height, int* band_out, int* slab_rows_out);
/* What one rank of a row-banded frame moves (host only, no device: the plan rt_render_multi follows).
 * kind 0 = the RGBA32F image, 1 = the RGBA8 image (RT_OUT_RGBA32F / RT_OUT_RGBA8). */
typedef struct rt_group_plan {
    int32_t n_ranks, rank;
    int32_t band_height;         /* rt_band_plan */
    int32_t slab_rows;           /* the most rows any rank renders */
    int32_t rank_rows;           /* rows this rank renders (rt_local_rows) */
    int32_t wire[2];             /* RT_PIXEL_* the kind travels in (GRAY for achromatic scenes), -1: not requested */
    int32_t elem_bytes[2];       /* bytes per pixel of wire[k] */
    uint64_t slab_bytes[2];      /* this rank's slab per kind: slab_rows x width x elem_bytes */
    uint64_t send_bytes[2];      /* bytes this rank sends rank 0 per frame (0 on rank 0: its slab is unpacked in place) */
    uint64_t gather_bytes[2];    /* rank 0: its gather buffer per kind (one slab-sized slot per renderer) */
    uint64_t payload_bytes;      /* rank 0: bytes received from the other ranks per frame, all kinds */
    int32_t renderers;           /* ranks that render bands: n_ranks, or n_ranks - 1 when rank 0 only assembles */
    int32_t root_renders;        /* 1: rank 0 renders bands too; 0: bands go to ranks 1 .. n - 1 (rt_group_root_renders) */
} rt_group_plan;
/* The plan of `rank` for a width x height frame (band_height 0 = auto, `outputs` as rt_render_multi, achromatic =
 * rt_scene_achromatic of the group's scene).  The band plan is over the renderers (rt_rows {band_height, renderers,
 * rank - (root_renders ? 0 : 1)}); rank 0 then receives every renderer's slab but its own. */
int rt_group_plan_frame(int width, int height, int n_ranks, int rank, int band_height, int outputs, int achromatic,
                        rt_group_plan* out);
/* Whether rank 0 of an n-rank group renders bands (1) or only receives and assembles the frame (0).  Rank 0 unpacks
 * the whole image (an HBM-bound 33 MB of RGBA8 stores at 4K) and receives every peer's slab besides, so from 4 ranks
 * on its bands go to the others (DESIGN.md §7 has the measurements); RT_GROUP_ROOT_RENDERS=0|1 overrides (every
 * rank of a group must see the same setting). */
int rt_group_root_renders(int n_ranks);
/* Rank 0's receive from `peer` (1 .. n_ranks - 1) for image `kind`: byte offset into rank 0's gather buffer and
 * byte count (equal to that peer's send_bytes[kind]). */
int rt_group_plan_recv(const rt_group_plan* plan, int width, int height, int peer, int kind, uint64_t* offset,
                       uint64_t* bytes);
/* FNV-1a 64 of the scene's flattened device record: what the ranks of a one-process-per-GPU group compare. */
int rt_scene_fingerprint(const rt_scene* scene, uint64_t* out);
/* One process driving n GPUs: ctxs[q] is rank q (ctxs[0] receives the image); distinct contexts, each on
 * its device (ncclCommInitAll over the contexts' devices for RT_TRANSPORT_RCCL). */
int rt_group_create(rt_ctx* const* ctxs, int n, int transport, rt_group** out);
/* One process per GPU (a torchrun-style launch): rank 0 makes the id, the launcher hands the same
 * RT_COMM_ID_BYTES bytes to every rank, each rank passes its own context (ncclCommInitRank). */
int rt_comm_unique_id(uint8_t* id);
int rt_group_create_rank(rt_ctx* ctx, int n_ranks, int rank, const uint8_t* id, rt_group** out);
int rt_group_destroy(rt_group* group);
/* *n_ranks: ranks of the group; *n_local: ranks driven by this process; *first_rank: the first of them;
 * *transport: RT_TRANSPORT_RCCL or RT_TRANSPORT_COPY.  Each pointer nullable. */
int rt_group_info(const rt_group* group, int* n_ranks, int* n_local, int* first_rank, int* transport);
/* One frame over the whole group.  Every rank calls it with the same camera, size, depth, band_height
 * (0 = auto) and `outputs` (RT_OUT_RGBA32F | RT_OUT_RGBA8: the images rank 0 receives).  On rank 0, rgba32f /
 * rgba8 are device images (width x height, j = 0 bottom) on rank 0's device for the requested outputs,
 * assembled in order on `stream` (a hipStream_t of that device; NULL = default stream); other ranks' pointers
 * are ignored.  Asynchronous: rank 0's image is complete when `stream` reaches this call's work.
 * What travels (the wire formats, rt_group_stats): for an achromatic scene (rt_scene_achromatic, decided by
 * each rank from its own context's scene — they are the same scene) GRAY8 for RGBA8 and GRAY32F for RGBA32F,
 * otherwise RGB8 and RGBA32F; rank 0 expands them into its images (rt_unpack_dev), byte for byte the images a
 * single rt_render_dev writes.  Every rank changes its scene (rt_set_scene) between the same frames; in a
 * one-process-per-GPU group the first frame after a rank's scene differs from the one the group last agreed on
 * all-reduces a fingerprint of the scene over the group (blocking, once per scene) and fails with RT_EINVAL on
 * every rank when they differ.  A scene change on some ranks only (the others still holding the agreed scene) is a
 * contract violation: those ranks enter the all-reduce while the others post their sends, and the group HANGS. */
int rt_render_multi(rt_group* group, const rt_camera* cam, int width, int height, int depth, int band_height,
                    int outputs, float* rgba32f, uint8_t* rgba8, void* stream);
/* Wait for the group's own render and gather streams (e.g. before timing on a rank > 0). */
int rt_group_synchronize(rt_group* group);
/* Per-phase timing of rt_render_multi (HIP events on the group's streams), for this process's ranks. */
typedef struct rt_group_stats {
    int32_t frames;              /* frames timed since rt_group_timing(group, 1) (the last <= 64 are averaged) */
    int32_t wire_float;          /* RT_PIXEL_* sent for RT_OUT_RGBA32F, -1: not requested (last frame) */
    int32_t wire_byte;           /* RT_PIXEL_* sent for RT_OUT_RGBA8, -1: not requested (last frame) */
    int32_t ranks_timed;         /* this process's ranks the means are over */
    uint64_t payload_bytes;      /* bytes rank 0 receives from the other ranks per frame (last frame) */
    double render_ms;            /* mean rt_render_dev launch on a rendering rank's render stream */
    double gather_ms;            /* mean send (rank > 0) / receive of every peer's slab (rank 0), from the
                                    point the rank's own render is done (it includes waiting for peers) */
    double assemble_ms;          /* rank 0: unshuffle + expand into the images (0 elsewhere) */
    double frame_ms;             /* rank 0: its render's start to the assembled image (0 elsewhere) */
} rt_group_stats;
/* enable = 1: start recording per-phase events from the next frame on (and clear earlier ones); 0: stop. */
int rt_group_timing(rt_group* group, int enable);
/* Synchronizes the group's streams, then fills *stats from the recorded frames. */
int rt_group_get_stats(rt_group* group, rt_group_stats* stats);

/* ---- output (host) -------------------------------------------------------------------------- */
/* writePpmScreenshot format (Hw4/ppm.cpp:15-25): "P6 W H 255\n" then RGB rows top-down, from an
 * RGBA8 (or RGB8 when channels == 3, GRAY8 when channels == 1) bottom-up image as glReadPixels returns it. */
int rt_write_ppm(const char* path, const uint8_t* pixels, int width, int height, int channels);

#ifdef __cplusplus
}
#endif

#endif /* RT_API_H */
