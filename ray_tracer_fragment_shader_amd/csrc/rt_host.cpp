// rt_host.cpp — host half of the C ABI (include/rt_api.h): scene construction the way the reference
// app builds g_scene, camera, row banding, device-scene flattening, PPM output.  No HIP calls here.
//
// Citations are into /root/reference/Hw4/MySdlApplication.cpp unless a file is named.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../include/rt_api.h"
#include "../../include/rt_diag.h"
#include "rt_cone.hpp"
#include "rt_internal.hpp"
#include "rt_jitter.hpp"
#include "rt_layout.hpp"

namespace {

thread_local std::string g_last_error;

// Host mirror of the reference Point (:136-212) with the same operation order.
struct HP {
    double x, y, z;
};
inline HP hp(double x, double y, double z) { return HP{x, y, z}; }
inline HP hp(const double* v) { return HP{v[0], v[1], v[2]}; }
inline HP operator+(HP a, HP b) { return hp(a.x + b.x, a.y + b.y, a.z + b.z); }
inline HP operator-(HP a, HP b) { return hp(a.x - b.x, a.y - b.y, a.z - b.z); }
inline HP operator*(double s, HP a) { return hp(s * a.x, s * a.y, s * a.z); }
inline double dot(HP a, HP b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline HP cross(HP a, HP b) { return hp(a.y * b.z - b.y * a.z, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline double length(HP a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
inline HP normalize(HP a) {
    double l = length(a);
    return hp(a.x / l, a.y / l, a.z / l);
}
inline void put(double* d, HP a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; }

// Reference constants (:31-52).
const double kWhite[3] = {1.0, 1.0, 1.0};
const double kBlack[3] = {0.0, 0.0, 0.0};
const double kRed[3] = {1.0, 0.0, 0.0};
const double kBoardPosition[3] = {0, 0, -160};
const double kBoardEdge = 320.0;
const double kBoardHalf = kBoardEdge / 2;
const unsigned kNumSquares = 8;
const double kSquareEdge = kBoardEdge / kNumSquares;
const double kSmall = .0001;
const double kAttenuation = 100000;
const double kCamera[3] = {0, 100, 200};
const double kLookAt[3] = {0, 0, -160};
const double kUp[3] = {0, 1, 0};

void set_material(rt_material* m, HP a, HP d, HP s, HP t, double r) {
    put(m->ambient, a);
    put(m->diffuse, d);
    put(m->specular, s);
    put(m->transparency, t);
    m->refraction = r;
}

// The kernel divides by a triangle's den with a shared reciprocal (rt_device.hpp div_const) only when
// |den| is in [2^-200, 2^200]: with |A| in [2^-500, 2^500] the IEEE sequence's scale steps are identities.
int32_t const_quotient_ok(double den) {
    return std::fabs(den) >= 0x1p-200 && std::fabs(den) <= 0x1p+200 ? 1 : 0;
}

bool valid_square(const char* sq) { return sq && sq[0] != 0 && sq[1] != 0; }

bool all_zero(const double v[3]) { return v[0] == 0 && v[1] == 0 && v[2] == 0; }

}  // namespace

int rt_fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

extern "C" int rt_abi_version(void) { return RT_ABI_VERSION; }

extern "C" const char* rt_last_error(void) { return g_last_error.c_str(); }

extern "C" int rt_scene_init_reference(rt_scene* s) {
    if (!s) return rt_fail(RT_EINVAL, "rt_scene_init_reference: null scene");
    memset(s, 0, sizeof(*s));
    put(s->position, hp(kBoardPosition));
    s->radius = std::sqrt((double)3) * kBoardHalf;                              // :590
    s->has_board = 1;
    s->board_half_size = kBoardHalf;
    s->square_edge_size = kSquareEdge;
    s->small_number = kSmall;
    s->attenuation_factor = kAttenuation;
    HP white = hp(kWhite), black = hp(kBlack);
    set_material(&s->white_square, .1 * white, .5 * white, white, black, 1);    // :583
    set_material(&s->black_square, black, .1 * white, black, black, 1);         // :585
    set_material(&s->sphere_material, black, .1 * white, white, black, 1);      // :586
    set_material(&s->tetrahedron_material, black, black, .1 * white, white, 2.0 / 3.0);  // :587
    HP red = hp(kRed);
    set_material(&s->cube_material, .1 * red, .4 * red, red, black, 1);         // :588
    return RT_OK;
}

extern "C" int rt_convert_string_coordinate(const char* sq, double out[3]) {   // :1326-1346
    if (!valid_square(sq) || !out) return rt_fail(RT_EINVAL, "rt_convert_string_coordinate: need 2 chars");
    HP first = hp(-kBoardEdge / 2, 0.0, kBoardEdge / 2);
    HP row = hp(0.0, 0.0, -(double(sq[0] - 'a') + .5) * kSquareEdge);
    HP col = hp((double(sq[1] - '0' - 1) + .5) * kSquareEdge, 0.0, 0.0);
    HP height = hp(0.0, 1.5 * kSquareEdge, 0.0);
    put(out, first + row + col + height);
    return RT_OK;
}

extern "C" int rt_light_position_from_square(const char* sq, double out[3]) {  // :1511
    double c[3];
    int rc = rt_convert_string_coordinate(sq, c);
    if (rc) return rc;
    put(out, hp(kBoardPosition) + hp(0.0, 3.5 * kSquareEdge, 0.0) + hp(c));
    return RT_OK;
}

extern "C" int rt_load_scene(const char* const* squares, const int32_t* types, int n, rt_scene* scene,
                             rt_sphere* sphere_buf, int sphere_cap, rt_mesh* mesh_buf, int mesh_cap, rt_light* light) {
    if (!scene || n < 0 || (n > 0 && (!squares || !types))) return rt_fail(RT_EINVAL, "rt_load_scene: bad args");
    std::map<std::string, int> board_map;                                       // boardMap (:595)
    for (int k = 0; k < n; ++k) {
        if (!valid_square(squares[k])) return rt_fail(RT_EINVAL, "rt_load_scene: bad square");
        if (types[k] < 0 || types[k] > 5) return rt_fail(RT_EINVAL, "rt_load_scene: bad object type");
        board_map[std::string(squares[k])] = types[k];                          // :1467
    }
    rt_scene_init_reference(scene);
    int ns = 0, nm = 0;
    bool unsupported = false;
    double lpos[3] = {0.0, 0.0, 0.0};                                           // g_lightPosition (:573)
    for (const auto& kv : board_map) {                                          // :1503-1538
        const char* sq = kv.first.c_str();
        switch (kv.second) {
            case 0:                                                             // LIGHT (:1510-1513)
                rt_light_position_from_square(sq, lpos);
                break;
            case 1:                                                             // TETRAHEDRON (:1514-1517)
            case 2: {                                                           // CUBE (:1518-1522)
                if (nm >= mesh_cap || !mesh_buf) return rt_fail(RT_EINVAL, "rt_load_scene: mesh_buf too small");
                rt_mesh& m = mesh_buf[nm++];
                m.kind = kv.second == 1 ? RT_MESH_TETRAHEDRON : RT_MESH_CUBE;
                m.after_spheres = ns;
                rt_convert_string_coordinate(sq, m.position);
                m.edge = kSquareEdge;
                break;
            }
            case 3: {                                                           // SPHERE (:1523-1527)
                if (ns >= sphere_cap || !sphere_buf) return rt_fail(RT_EINVAL, "rt_load_scene: sphere_buf too small");
                rt_convert_string_coordinate(sq, sphere_buf[ns].center);
                sphere_buf[ns].radius = kSquareEdge / 2;
                ++ns;
                break;
            }
            default:                                                            // CYLINDER / CONE: stubs
                unsupported = true;
                break;
        }
    }
    scene->n_spheres = ns;
    scene->spheres = sphere_buf;
    scene->n_meshes = nm;
    scene->meshes = mesh_buf;
    if (light) {
        put(light->color, hp(kWhite));                                          // g_lightColor (:577)
        put(light->position, hp(lpos));
        scene->n_lights = 1;                                                    // draw() pushes one light (:1552-1554)
        scene->lights = light;
    }
    if (unsupported)
        return rt_fail(RT_EUNSUPPORTED,
                       "rt_load_scene: cylinder/cone are stubs in the reference (MySdlApplication.cpp:1000-1020, 457-458)");
    return RT_OK;
}

extern "C" int rt_camera_init_reference(rt_camera* cam, int width, int height, double pitch) {
    if (!cam || width <= 0 || height <= 0) return rt_fail(RT_EINVAL, "rt_camera_init_reference: bad args");
    memset(cam, 0, sizeof(*cam));
    put(cam->eye, hp(kCamera));
    put(cam->look_at, hp(kLookAt));
    put(cam->up, hp(kUp));
    cam->bottom_x = -width / 2;                                                 // :1560
    cam->bottom_y = -height / 2;
    cam->pitch = pitch;
    return RT_OK;
}

// The sample-grid camera of a supersampled render (rt_api.h): pixel (S i + a, S j + b) of this camera's frame is
// sample (a, b) of pixel (i, j) of `cam`'s.
extern "C" int rt_camera_supersample(const rt_camera* cam, int samples, rt_camera* out) {
    if (!cam || !out) return rt_fail(RT_EINVAL, "rt_camera_supersample: null pointer");
    if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
        return rt_fail(RT_EINVAL, "rt_camera_supersample: samples must be 1, 2, 4 or 8");
    const long long bx = (long long)cam->bottom_x * samples, by = (long long)cam->bottom_y * samples;
    if (bx < INT32_MIN || bx > INT32_MAX || by < INT32_MIN || by > INT32_MAX)
        return rt_fail(RT_EINVAL, "rt_camera_supersample: samples * bottom_x / bottom_y overflows int32");
    rt_camera c = *cam;                                                         // (out may alias cam)
    c.pitch = cam->pitch / (double)samples;                                     // exact: a power of two
    c.bottom_x = (int32_t)bx;
    c.bottom_y = (int32_t)by;
    *out = c;
    return RT_OK;
}

// The camera of rt_render_dof_dev with its focal plane (the plane through look_at spanned by right and up') moved to
// `ratio` times its distance from the eye: the pitch scales with it, so every pixel's primary ray keeps its
// direction (up to rounding) and the pinhole view is the same.
extern "C" int rt_camera_focus(const rt_camera* cam, double ratio, rt_camera* out) {
    if (!cam || !out) return rt_fail(RT_EINVAL, "rt_camera_focus: null pointer");
    if (!(ratio > 0.0) || !std::isfinite(ratio))
        return rt_fail(RT_EINVAL, "rt_camera_focus: ratio must be finite and > 0");
    rt_camera c = *cam;                                                         // (out may alias cam)
    if (ratio != 1.0) {                                                         // 1.0: unchanged bit for bit
        for (int q = 0; q < 3; ++q) c.look_at[q] = cam->eye[q] + ratio * (cam->look_at[q] - cam->eye[q]);
        c.pitch = ratio * cam->pitch;
    }
    *out = c;
    return RT_OK;
}

// The camera of the shutter render (rt_api.h) at time sigma: eye and look_at moved by sigma times the motion's
// half-extents, one multiplication and one addition per component; everything else copied.  motion = NULL: no move.
extern "C" int rt_camera_at(const rt_camera* cam, const rt_camera_motion* motion, double sigma, rt_camera* out) {
    if (!cam || !out) return rt_fail(RT_EINVAL, "rt_camera_at: null pointer");
    if (!std::isfinite(sigma)) return rt_fail(RT_EINVAL, "rt_camera_at: sigma must be finite");
    rt_camera c = *cam;                                                         // (out may alias cam)
    if (motion) {
        for (int q = 0; q < 3; ++q)
            if (!std::isfinite(motion->eye[q]) || !std::isfinite(motion->look_at[q]))
                return rt_fail(RT_EINVAL, "rt_camera_at: non-finite displacement (motion)");
        for (int q = 0; q < 3; ++q) {
            c.eye[q] = cam->eye[q] + (sigma * motion->eye[q]);
            c.look_at[q] = cam->look_at[q] + (sigma * motion->look_at[q]);
        }
    }
    *out = c;
    return RT_OK;
}

// The seven levels of sample (I, Jr) of the jittered render's S width-wide sample frame, by the kernel's own functions
// (rt_jitter.hpp).
extern "C" int rt_jitter_sample(int width, int samples, int jitter, uint32_t seed, int I, int Jr, int32_t levels[7]) {
    if (!levels) return rt_fail(RT_EINVAL, "rt_jitter_sample: null pointer");
    if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
        return rt_fail(RT_EINVAL, "rt_jitter_sample: samples must be 1, 2, 4 or 8");
    const int jl = rtj::jitter_log2_of(jitter);
    if (jl < 0) return rt_fail(RT_EINVAL, "rt_jitter_sample: jitter must be 1, 2, 4, 8 or 16");
    const long long sw = (long long)width * samples;
    if (width <= 0 || sw > INT32_MAX) return rt_fail(RT_EINVAL, "rt_jitter_sample: bad image size (width)");
    if (I < 0 || I >= sw || Jr < 0 || (long long)Jr * sw + I >= (1LL << 31))
        return rt_fail(RT_EINVAL, "rt_jitter_sample: sample (I, Jr) outside a frame of at most 2^31 samples");
    const uint32_t w = rtj::jitter_word((uint32_t)Jr * (uint32_t)sw + (uint32_t)I, seed);
    for (int d = 0; d < 7; ++d) levels[d] = rtj::jitter_level(w, d, jl);
    return RT_OK;
}

extern "C" int rt_adaptive_workspace_bytes(int width, int height, int samples, size_t* bytes) {
    if (!bytes) return rt_fail(RT_EINVAL, "rt_adaptive_workspace_bytes: null pointer");
    *bytes = 0;
    if (samples != 1 && samples != 2 && samples != 4 && samples != 8)
        return rt_fail(RT_EINVAL, "rt_adaptive_workspace_bytes: samples must be 1, 2, 4 or 8");
    if (width <= 0 || height <= 0 || (long long)width * height > (1LL << 31))
        return rt_fail(RT_EINVAL, "rt_adaptive_workspace_bytes: bad image size");
    *bytes = rt_adaptive_layout((size_t)width * (size_t)height).bytes;
    return RT_OK;
}

extern "C" int rt_lens_adaptive_workspace_bytes(int width, int height, size_t* bytes) {
    if (!bytes) return rt_fail(RT_EINVAL, "rt_lens_adaptive_workspace_bytes: null pointer");
    *bytes = 0;
    if (width <= 0 || height <= 0 || (long long)width * height > (1LL << 31))
        return rt_fail(RT_EINVAL, "rt_lens_adaptive_workspace_bytes: bad image size");
    *bytes = rt_lens_adaptive_layout((size_t)width * (size_t)height).bytes;
    return RT_OK;
}

namespace {

int frames_of(const rt_rows* r) { return (r && r->frames > 1) ? r->frames : 1; }

// Rows of one frame that the rank renders.
int frame_local_rows(int height, const rt_rows* r) {
    if (!r || r->n_ranks <= 1) return height;
    const int hb = r->band_height, G = r->n_ranks;
    const int full_bands = height / hb, tail = height % hb;
    int n = (full_bands / G) * hb;
    if (r->rank < full_bands % G) n += hb;                                      // bands 0..extra-1 of the last round
    if (tail && (full_bands % G) == r->rank) n += tail;                         // the partial last band
    return n;
}

}  // namespace

extern "C" int rt_local_rows(int height, const rt_rows* r, int* out) {
    if (!out || height < 0) return rt_fail(RT_EINVAL, "rt_local_rows: bad args");
    if (r && (r->frames < 0 || r->n_ranks < 1)) return rt_fail(RT_EINVAL, "rt_local_rows: bad frames / ranks");
    if (r && r->n_ranks > 1 && (r->band_height <= 0 || r->rank < 0 || r->rank >= r->n_ranks))
        return rt_fail(RT_EINVAL, "rt_local_rows: bad band geometry");
    if (r && r->n_ranks == 1 && r->rank != 0) return rt_fail(RT_EINVAL, "rt_local_rows: bad rank");
    *out = frame_local_rows(height, r) * frames_of(r);
    return RT_OK;
}

extern "C" int rt_global_row(int height, const rt_rows* r, int local_row, int* out) {
    int nl = 0;
    int rc = rt_local_rows(height, r, &nl);
    if (rc) return rc;
    if (!out || local_row < 0 || local_row >= nl) return rt_fail(RT_EINVAL, "rt_global_row: row out of range");
    const int per = frame_local_rows(height, r);
    const int f = local_row / per, lr = local_row % per;
    int j = lr;
    if (r && r->n_ranks > 1) {
        const int hb = r->band_height;
        j = ((lr / hb) * r->n_ranks + r->rank) * hb + lr % hb;
    }
    *out = f * height + j;
    return RT_OK;
}

// Row bands of the multi-GPU group (rt_group.cpp).
extern "C" int rt_pixel_bytes(int format, int* bytes) {
    if (!bytes) return rt_fail(RT_EINVAL, "rt_pixel_bytes: null pointer");
    switch (format) {
        case RT_PIXEL_RGBA32F: *bytes = 16; return RT_OK;
        case RT_PIXEL_GRAY32F: *bytes = 4; return RT_OK;
        case RT_PIXEL_RGBA8: *bytes = 4; return RT_OK;
        case RT_PIXEL_RGB8: *bytes = 3; return RT_OK;
        case RT_PIXEL_GRAY8: *bytes = 1; return RT_OK;
        default: *bytes = 0; return rt_fail(RT_EINVAL, "rt_pixel_bytes: unknown pixel format");
    }
}

extern "C" int rt_band_plan(int height, int n_ranks, int band_height, int* band_out, int* slab_rows_out) {
    if (height <= 0 || n_ranks <= 0 || band_height < 0 || !band_out)
        return rt_fail(RT_EINVAL, "rt_band_plan: bad arguments");
    int hb = band_height;
    if (hb == 0) {
        // The render's tile height (8 rows): every 8 x 8 tile of a rank's slab is then 8 consecutive image rows, which
        // the per-wave primary cone culling needs (a tile straddling two bands tests every sphere).  Ranks differ by
        // at most one band (c4 at 8 ranks: 272 against 264 rows).  r02-r05 chose the largest height <= 16 giving
        // every rank the same rows (15 for 2160 rows over 8 ranks): its straddling tiles made every rank's band set
        // 10% slower (tools/c4_gap_probe.py part 2: 30.4 -> 27.5 us per 1/8 frame serial).
        hb = 8;
    }
    if (n_ranks == 1) hb = std::max(hb, 1);
    int slab = 0;
    for (int q = 0; q < n_ranks; ++q) {
        rt_rows r = {hb, n_ranks, q, 1};
        int nl = 0;
        int rc = rt_local_rows(height, &r, &nl);
        if (rc) return rc;
        slab = std::max(slab, nl);
    }
    *band_out = hb;
    if (slab_rows_out) *slab_rows_out = slab;
    return RT_OK;
}

void rt_camera_basis(const rt_camera* cam, double right[3], double upp[3]) {
    HP ld = hp(cam->look_at) - hp(cam->eye);                                    // :1270
    HP r = normalize(cross(ld, hp(cam->up)));                                   // :1271-1273
    HP u = normalize(cross(r, ld));                                             // :1276-1277
    put(right, r);
    put(upp, u);
}

// ---- the scene record and the motion record (rt_layout.hpp): rt_build_dev_scene's steps, in its order ------------------
namespace {

const double kInf = std::numeric_limits<double>::infinity();

// The builders fill the arrays rt_layout.hpp's layout functions hand out as const.
template <class T>
T* writable(const T* p) { return const_cast<T*>(p); }

// The checks on an rt_scene.  n_tris: the triangles its meshes flatten to.
int check_scene(const rt_scene* s, int* n_tris) {
    if (!s) return rt_fail(RT_EINVAL, "rt_set_scene: null scene");
    if (s->n_spheres < 0 || s->n_spheres > RT_MAX_SPHERES)
        return rt_fail(RT_EINVAL, "rt_set_scene: n_spheres out of range [0, " + std::to_string(RT_MAX_SPHERES) + "]");
    if (s->n_lights < 0 || s->n_lights > RT_MAX_LIGHTS)
        return rt_fail(RT_EINVAL, "rt_set_scene: n_lights out of range [0, " + std::to_string(RT_MAX_LIGHTS) + "]");
    if (s->n_spheres > 0 && !s->spheres) return rt_fail(RT_EINVAL, "rt_set_scene: null spheres");
    if (s->n_lights > 0 && !s->lights) return rt_fail(RT_EINVAL, "rt_set_scene: null lights");
    if (!(s->small_number >= 0) || !(s->square_edge_size != 0))
        return rt_fail(RT_EINVAL, "rt_set_scene: bad constants");
    // The kernel's checker divides by the square size with a shared reciprocal (rt_device.hpp
    // material_of), exact for sizes in this (generous) range.
    if (!(std::fabs(s->square_edge_size) >= 0x1p-400 && std::fabs(s->square_edge_size) <= 0x1p+400))
        return rt_fail(RT_EUNSUPPORTED, "rt_set_scene: square_edge_size outside [2^-400, 2^400]");
    if (s->n_meshes < 0 || s->n_meshes > RT_MAX_MESHES || (s->n_meshes > 0 && !s->meshes))
        return rt_fail(RT_EINVAL, "rt_set_scene: bad meshes");
    *n_tris = 0;
    for (int m = 0; m < s->n_meshes; ++m) {
        const rt_mesh& M = s->meshes[m];
        if (M.kind != RT_MESH_TETRAHEDRON && M.kind != RT_MESH_CUBE) return rt_fail(RT_EINVAL, "rt_set_scene: bad mesh kind");
        if (M.after_spheres < 0 || M.after_spheres > s->n_spheres || (m > 0 && M.after_spheres < s->meshes[m - 1].after_spheres))
            return rt_fail(RT_EINVAL, "rt_set_scene: mesh after_spheres must be non-decreasing in [0, n_spheres]");
        *n_tris += M.kind == RT_MESH_TETRAHEDRON ? 4 : 12;
    }
    return RT_OK;
}

// The header's constants: counts, bounding sphere, the reference's constants, lights, and the fields later steps or
// the device decide at their "not yet" values.  bc: g_scene's _position + offset (:739).
void put_header(const rt_scene* s, HP bc, int n_tris, rt::DevScene* d) {
    d->n_spheres = s->n_spheres;
    d->n_padded = rt::padded_spheres(s->n_spheres);
    d->n_stride = rt::sphere_stride(d->n_padded);    // array stride (rt_layout.hpp)
    d->lds_bytes = rt::lds_bytes_for(s->n_spheres);
    d->n_meshes = s->n_meshes;
    d->n_tris = n_tris;
    d->eye[0] = d->eye[1] = d->eye[2] = std::numeric_limits<double>::quiet_NaN();
    put(d->bc, bc);
    d->br2 = s->radius * s->radius;                                             // :750
    d->bound_on = s->radius > 0;                                                // :747 (g_scene is not _amSphere)
    // origins with |o - bc|^2 < (R-1)^2 provably pass the cull (proof at rt_device.hpp bound_pass_dp: |s| >= 1, which
    // clears the reference's |s| < SMALL_NUMBER test only while SMALL_NUMBER < 1 — kept below 0.5 for the rounding)
    d->inner2 = s->radius > 2 && s->small_number < 0.5 ? (s->radius - 1) * (s->radius - 1) : -1.0;
    d->eps = s->small_number;
    d->att = s->attenuation_factor;
    put(d->coff, bc);                                                           // CheckerBoard's positionOffset
    d->half = s->board_half_size;
    d->square = s->square_edge_size;
    d->self_eps2 = 0.25 * s->small_number * s->small_number;
    d->hits_inside = 0;                  // prove_hits_inside, once every object's extent is known
    d->hits_lim2 = -1.0;
    d->counters = nullptr;
    d->hits_ok = 0;                      // per eye, rt_prepare_kernel
    d->n_lights = s->n_lights;
    for (int k = 0; k < s->n_lights; ++k) {
        for (int q = 0; q < 3; ++q) {
            d->light[k].pos[q] = s->lights[k].position[q];
            d->light[k].col[q] = s->lights[k].color[q];
        }
    }
}

// The five DevMat records, and the two verdicts that choose the kernel variant.
void put_materials(const rt_scene* s, rt::DevScene* d) {
    const rt_material* mats[5] = {&s->white_square, &s->black_square, &s->sphere_material, &s->tetrahedron_material,
                                  &s->cube_material};
    // rayTraceRay (:1230-1247) spawns a transmitted ray when transparency != 0 and |transparency| > eps, a
    // reflected ray when opacity = 1 - transparency != 0.  A material that does both makes every hit on it
    // a branch of a ray tree: such scenes run the trace_tree kernels (depth-first, per-lane node stack);
    // the others follow one continuation per hit.
    bool used[5] = {true, true, s->n_spheres > 0, false, false};
    for (int m = 0; m < s->n_meshes; ++m) used[s->meshes[m].kind == RT_MESH_TETRAHEDRON ? 3 : 4] = true;
    bool any_transparent = false, tree = false;
    for (int m = 0; m < 5; ++m) {
        const rt_material* M = mats[m];
        rt::DevMat& dm = d->mat[m];
        HP T = hp(M->transparency);
        HP opacity = hp(1.0, 1.0, 1.0) - T;                                     // :1236
        bool zeroT = T.x == 0 && T.y == 0 && T.z == 0;
        bool transmit = !zeroT && length(T) > s->small_number;                  // :1238
        bool reflect = !(opacity.x == 0 && opacity.y == 0 && opacity.z == 0);   // :1243
        if (used[m] && transmit && reflect) tree = true;
        if (used[m] && !zeroT) any_transparent = true;
        for (int q = 0; q < 3; ++q) {
            dm.amb[q] = M->ambient[q];
            dm.diff[q] = M->diffuse[q];
            dm.spec[q] = M->specular[q];
        }
        put(dm.w, transmit ? T : opacity);
        put(dm.wt, T);
        put(dm.wo, opacity);
        dm.refr = M->refraction;
        dm.transmit = transmit ? 1 : 0;
        dm.transparent = zeroT ? 0 : 1;
        dm.reflect = reflect ? 1 : 0;
    }
    d->transparent = any_transparent ? 1 : 0;
    d->tree = tree ? 1 : 0;
}

// The record of Triangle(pos, m, v0, v1, v2) after its ctor (:406-433), world vertex 0 = pos + v0, in *T, whose
// `degenerate` is left to the caller (the board keeps it 0.0 and decides by the return values of its two triangles;
// the meshes store it).  Returns whether the ctor found the triangle degenerate: it then never intersects (:633-637).
bool tri_record(HP pos, HP v0, HP v1, HP v2, double eps, rt::DevTri* T) {
    HP u = v1 - v0, v = v2 - v0;                                                // :413-414
    HP n = cross(u, v);                                                         // :415
    bool degenerate = length(n) < eps;                                          // :418
    n = normalize(n);                                                           // :422
    double uv = dot(u, v), uu = dot(u, u), vv = dot(v, v);                     // :424-426
    double den = uv * uv - uu * vv;                                             // :428
    if (std::fabs(den) < eps) degenerate = true;                                // :430
    put(T->v0, pos + v0);                                                       // :640-641
    put(T->u, u);
    put(T->v, v);
    put(T->n, n);
    T->uv = uv;
    T->uu = uu;
    T->vv = vv;
    T->den = den;
    // den < 0: A > |den| 2^-1070 proves A/den < 0 (nonzero), so the kernel may skip the division.
    // Otherwise disable the shortcut.
    T->thr = (den < 0 && std::fabs(den) >= 1024.0) ? std::ldexp(std::fabs(den), -1070) : kInf;
    T->fast = const_quotient_ok(den);
    return degenerate;
}

// The board: its two triangles, the shared-plane check, and the two shortcuts with their proofs.
int put_board(const rt_scene* s, HP bc, rt::DevScene* d) {
    d->has_board = 0;
    if (s->has_board) {
        // CheckerBoard(p) -> _boundingSquare = Quad(p, Material(), P1..P4) (:1064-1069) ->
        // Triangle(zero, m, P1,P2,P3), Triangle(zero, m, P1,P3,P4) (:840-841).
        const double h = s->board_half_size;
        const HP P[4] = {hp(-h, 0, -h), hp(h, 0, -h), hp(h, 0, h), hp(-h, 0, h)};
        const int idx[2][3] = {{0, 1, 2}, {0, 2, 3}};
        const HP quad_pos = hp(s->board_position) + bc;                         // Quad: _position + offset
        const HP tri_pos = hp(0.0, 0.0, 0.0) + quad_pos;                        // Triangle: zero + offset (:640)
        bool degenerate[2];
        for (int t = 0; t < 2; ++t)
            degenerate[t] = tri_record(tri_pos, P[idx[t][0]], P[idx[t][1]], P[idx[t][2]], s->small_number, &d->tri[t]);
        // The kernel shares the plane step of the two triangles; the reference board always satisfies
        // this (same vertex 0, same normal).  A degenerate board never intersects (:633-637).
        if (!degenerate[0] && !degenerate[1]) {
            if (memcmp(d->tri[0].v0, d->tri[1].v0, sizeof(d->tri[0].v0)) != 0 ||
                memcmp(d->tri[0].n, d->tri[1].n, sizeof(d->tri[0].n)) != 0)
                return rt_fail(RT_EUNSUPPORTED, "rt_set_scene: board triangles do not share a plane");
            d->has_board = 1;
        } else if (degenerate[0] != degenerate[1]) {
            return rt_fail(RT_EUNSUPPORTED, "rt_set_scene: half-degenerate board");
        }
    }
    // Board self-test skip (rt_device.hpp board_skip): with the board normal exactly (0, +-1, 0), a ray that
    // starts at a board hit point q has |n . (v0 - q)| <= 2^-50 (3 |p0.y| + 5 |v0.y| + 1), p0 the origin of
    // the ray that hit; below eps^2 / 2 its m = num / nd (|nd| >= eps) is below eps: a certain miss.
    d->board_skip_y = -1.0;
    if (d->has_board && d->tri[0].n[0] == 0.0 && d->tri[0].n[2] == 0.0 && std::fabs(d->tri[0].n[1]) == 1.0 &&
        s->small_number > 0) {
        const double eps2 = s->small_number * s->small_number;
        const double y = (eps2 / 2 / 0x1p-50 - 5 * std::fabs(d->tri[0].v0[1]) - 1) / 3;
        if (y > 0 && std::isfinite(y)) d->board_skip_y = y;
    }
    // Board decided by position (rt_device.hpp board_hit): the reference's CheckerBoard exactly — normal (0, -1, 0),
    // T1 = (P1, P2, P3) with u = (L, 0, 0), v = (L, 0, L), T2 = (P1, P3, P4) with u = (L, 0, L), v = (0, 0, L) — and an
    // integer side L <= 2^12, so uu, uv, vv and den are exact.  Margin delta = L 2^-19, range far = 2^24 L (proof at
    // board_hit).
    d->board_fast = 0;
    d->board_lo = d->board_hi = d->board_out = kInf;
    d->board_far = -1.0;
    if (d->has_board) {
        const rt::DevTri &T1 = d->tri[0], &T2 = d->tri[1];
        const double L = 2 * s->board_half_size;
        auto is3 = [](const double* a, double x, double y, double z) { return a[0] == x && a[1] == y && a[2] == z; };
        const bool shape = L >= 1 && L <= 4096 && L == std::floor(L) && is3(T1.n, 0, -1, 0) && is3(T2.n, 0, -1, 0) &&
                           is3(T1.u, L, 0, 0) && is3(T1.v, L, 0, L) && is3(T2.u, L, 0, L) && is3(T2.v, 0, 0, L) &&
                           is3(T1.v0, T2.v0[0], T2.v0[1], T2.v0[2]) && T1.uu == L * L && T1.uv == L * L &&
                           T1.vv == 2 * L * L && T2.uu == 2 * L * L && T2.uv == L * L && T2.vv == L * L &&
                           T1.den == -(L * L * L * L) && T2.den == -(L * L * L * L);
        if (shape) {
            const double delta = std::ldexp(L, -19);
            d->board_fast = 1;
            d->board_lo = delta;
            d->board_hi = L - delta;
            d->board_out = L + delta;
            d->board_far = std::ldexp(L, 24);
        }
    }
    return RT_OK;
}

// FP32 filter image of a sphere (rt_device.hpp sphere_reject32): centre relative to bc, and
// rm = r2 + 4K sC^2 + K r2 rounded up, sC = max|c_i - bc_i|.  rel: centre - bound centre; r2: the squared radius the
// filter is to cover (the sphere's own, or its swept sphere's in the motion record).
rt::DevSphereF filter_record(HP rel, double r2) {
    const double sC = std::max(std::fabs(rel.x), std::max(std::fabs(rel.y), std::fabs(rel.z)));
    const double K = (double)rt::kFilterK;
    const double rm = r2 + 4 * K * sC * sC + K * r2;
    rt::DevSphereF f;
    f.cx = (float)rel.x;
    f.cy = (float)rel.y;
    f.cz = (float)rel.z;
    f.rm = (float)rm;
    if ((double)f.rm < rm) f.rm = std::nextafter(f.rm, std::numeric_limits<float>::infinity());
    return f;
}

// The spheres and their filter records, then the padding up to the stride.
void put_spheres(const rt_scene* s, HP bc, int ns, rt::DevSphere* sph, rt::DevSphereF* sphf) {
    for (int k = 0; k < s->n_spheres; ++k) {
        HP c = hp(s->spheres[k].center) + bc;                                   // sphere: _position + offset
        put(sph[k].c, c);
        sph[k].r2 = s->spheres[k].radius * s->spheres[k].radius;                // :750
        sphf[k] = filter_record(c - bc, sph[k].r2);
    }
    for (int k = s->n_spheres; k < ns; ++k) {                                   // padding: never a hit
        sph[k].r2 = -kInf;
        sphf[k].rm = -std::numeric_limits<float>::infinity();
    }
}

// Shadow-ray cone filter (rt_device.hpp occluded): a shadow ray Line(p, L) lies on a line through the
// light L, so it can meet sphere k only if |u . v_k| >= cos(phi_k), v_k = unit(C_k - L),
// sin(phi_k) = r / |C_k - L|.  Stored: f32(v_k) and c_k = cos(phi_k) - 2^-16 rounded down; a light
// inside or near a sphere (|C - L| <= r (1 + 2^-20) or |C - L| <= 2^-14 (1 + |L| + |C|)) gets c = -inf
// (always tested), padding spheres c = +inf (never).
void put_light_cones(const rt_scene* s, int ns, const rt::DevSphere* sph, rt::DevSphereLightF* lightf) {
    for (int i = 0; i < s->n_lights; ++i) {
        const HP L = hp(s->lights[i].position);
        const double aL = std::max(std::fabs(L.x), std::max(std::fabs(L.y), std::fabs(L.z)));
        for (int k = 0; k < ns; ++k) {
            rt::DevSphereLightF& f = lightf[i * ns + k];
            f.vx = f.vy = f.vz = 0.0f;
            if (k >= s->n_spheres) {
                f.c = std::numeric_limits<float>::infinity();
                continue;
            }
            const HP C = hp(sph[k].c);
            const HP v = C - L;
            const double D = length(v), r = std::fabs(s->spheres[k].radius);
            const double aC = std::max(std::fabs(C.x), std::max(std::fabs(C.y), std::fabs(C.z)));
            if (!(D > r * (1.0 + 0x1p-20) && D > 0x1p-14 * (1.0 + aL + aC))) {
                f.c = -std::numeric_limits<float>::infinity();
                continue;
            }
            const double sn = r / D;
            const double c = std::sqrt(std::max(0.0, 1.0 - sn * sn)) - 0x1p-16;
            f.vx = (float)(v.x / D);
            f.vy = (float)(v.y / D);
            f.vz = (float)(v.z / D);
            float cf = (float)c;
            if ((double)cf > c) cf = std::nextafter(cf, -std::numeric_limits<float>::infinity());
            f.c = cf;
        }
    }
}

// Meshes (Tetrahedron :863-900, Cube :903-950): Shape(p, m, sqrt(3)*edge/2, false) with Triangle /
// Quad sub-objects at zero position.  World vertex 0 of a triangle: tetrahedron (zero + (p + bc)) + v0,
// cube (zero + (zero + (p + bc))) + v0 — the chain of `_position + positionOffset` additions (:739, :640).
void put_meshes(const rt_scene* s, HP bc, rt::DevMesh* dmesh, rt::DevTri* dtri) {
    const HP zero = hp(0.0, 0.0, 0.0);
    int t_next = 0;
    for (int m = 0; m < s->n_meshes; ++m) {
        const rt_mesh& M = s->meshes[m];
        rt::DevMesh& DM = dmesh[m];
        const HP mpos = hp(M.position) + bc;                                    // Shape: _position + offset
        const double radius = std::sqrt((double)3) * M.edge / 2;
        put(DM.bc, mpos);
        DM.br2 = radius * radius;
        DM.inner2 = radius > 2 && s->small_number < 0.5 ? (radius - 1) * (radius - 1) : -1.0;   // (as g_scene's)
        DM.tri0 = t_next;
        DM.child = (s->has_board ? 1 : 0) + M.after_spheres + m;
        const double h = M.edge / 2;
        std::vector<std::array<HP, 3>> tris;
        HP tpos;
        if (M.kind == RT_MESH_TETRAHEDRON) {
            DM.mat = 3;
            DM.per_face = 1;
            DM.nfaces = 4;
            tris = {{hp(-h, -h, -h), hp(h, -h, -h), hp(-h, -h, h)},                 // bottom
                    {hp(-h, -h, -h), hp(-h, -h, h), hp(-h, h, -h)},                 // back
                    {hp(-h, -h, -h), hp(-h, h, -h), hp(-h, -h, h)},                 // left
                    {hp(-h, -h, h), hp(h, -h, -h), hp(-h, h, -h)}};                 // front
            tpos = zero + mpos;
        } else {
            DM.mat = 4;
            DM.per_face = 2;
            DM.nfaces = 6;
            const HP q[6][4] = {{hp(-h, h, -h), hp(h, h, -h), hp(h, h, h), hp(-h, h, h)},        // top
                                {hp(-h, -h, -h), hp(h, -h, -h), hp(h, -h, h), hp(-h, -h, h)},    // bottom
                                {hp(-h, -h, -h), hp(-h, h, -h), hp(-h, h, h), hp(-h, -h, h)},    // left
                                {hp(h, -h, -h), hp(h, h, -h), hp(h, h, h), hp(h, -h, h)},        // right
                                {hp(-h, -h, -h), hp(h, -h, -h), hp(h, h, -h), hp(-h, h, -h)},    // back
                                {hp(-h, -h, h), hp(h, -h, h), hp(h, h, h), hp(-h, h, h)}};       // front
            for (int f = 0; f < 6; ++f) {                                       // Quad: T(p1,p2,p3), T(p1,p3,p4)
                tris.push_back({q[f][0], q[f][1], q[f][2]});
                tris.push_back({q[f][0], q[f][2], q[f][3]});
            }
            tpos = zero + (zero + mpos);
        }
        for (const auto& tv : tris) {
            rt::DevTri& T = dtri[t_next++];
            T.degenerate = tri_record(tpos, tv[0], tv[1], tv[2], s->small_number, &T) ? 1.0 : 0.0;
        }
    }
}

// The hits_inside limit.  Hit points carry rounding that grows with their ray's origin o (D = |o - bc|): a sphere hit's
// |q - C|^2 = r^2 + err(disc), err(disc) <= 2^-49 D^2 (the sqrt keeps it below 2^-50 D^2 / r in |q - C|),
// and p0 + s u or p0 + m d adds <= 2^-51 (D + |bc| + far).  dev(D) = 2^-44 (D + |bc| + far + 1 + D^2 / rmin)
// bounds both with room; the shortcut is kept for origins with dev(D) <= slack / 2 (hits_lim2, checked per
// ray on the device: the camera eye per render, every start of a ray list), and only when that covers the
// hit points themselves (D = R: the origins of later levels).
// inner2 > 0: DevScene::inner2; far: an upper bound of |q - bc| over every hit point q; rmin: the smallest sphere
// radius; absbc: |bc|.  Returns whether the shortcut holds, and then *lim2 = the square of the largest such D.
bool hits_limit(double inner2, double far, double rmin, double absbc, double* lim2) {
    const double Rin = std::sqrt(inner2) * (1.0 - 1e-9);
    const double slack = Rin - far - 1e-6 * (1.0 + far);
    const double e = 0x1p-44, a = rmin > 0 ? e / rmin : kInf, c = e * (absbc + far + 1.0) - slack / 2;
    double dlim = -1.0;                                  // largest D with a D^2 + e D + c <= 0
    if (std::isfinite(far) && std::isfinite(absbc) && slack > 0 && c < 0)
        dlim = std::isfinite(a) ? (-e + std::sqrt(e * e - 4 * a * c)) / (2 * a) : -c / e;
    if (!(dlim >= Rin)) return false;
    *lim2 = dlim * dlim * (1.0 - 1e-9);
    return true;
}

// Rays that start at a hit point pass g_scene's bounding-sphere cull when every hit point lies within
// R - 1 of its centre (the kernel's bound_pass shortcut, rt_device.hpp): an upper bound of |q - bc| over
// the spheres (|C - bc| + r), the board's corners and the meshes' bounding spheres, with a margin far
// above the rounding of the hit points (hits_limit), lets the kernel skip the test for them (hits_inside).
void prove_hits_inside(const rt_scene* s, HP bc, const rt::DevSphere* sph, const rt::DevMesh* dmesh, rt::DevScene* d) {
    if (!(d->bound_on && d->inner2 > 0)) return;
    double far = 0.0;
    for (int k = 0; k < s->n_spheres; ++k)
        far = std::max(far, length(hp(sph[k].c) - bc) + std::fabs(s->spheres[k].radius));
    if (d->has_board) {
        const double h = s->board_half_size;
        const HP quad = hp(s->board_position) + bc;
        for (int cx = -1; cx <= 1; cx += 2)
            for (int cz = -1; cz <= 1; cz += 2) far = std::max(far, length(quad + hp(cx * h, 0, cz * h) - bc));
    }
    for (int m = 0; m < s->n_meshes; ++m) far = std::max(far, length(hp(dmesh[m].bc) - bc) + std::sqrt(dmesh[m].br2));
    double rmin = kInf;
    for (int k = 0; k < s->n_spheres; ++k) rmin = std::min(rmin, std::fabs(s->spheres[k].radius));
    if (hits_limit(d->inner2, far, rmin, length(bc), &d->hits_lim2)) d->hits_inside = 1;
}

}  // namespace

int rt_build_dev_scene(const rt_scene* s, std::vector<unsigned char>* blob) {
    int n_tris = 0;
    if (int rc = check_scene(s, &n_tris)) return rc;
    // (rounded up to 16 B: kernels may copy the whole record into LDS in 4- or 16-byte words)
    const size_t bytes = ((size_t)rt::scene_bytes_for(s->n_spheres, s->n_meshes, n_tris, s->n_lights) + 15) & ~(size_t)15;
    blob->assign(bytes, 0);
    rt::DevScene* d = reinterpret_cast<rt::DevScene*>(blob->data());
    const HP bc = hp(s->position) + hp(0.0, 0.0, 0.0);                          // g_scene: _position + offset (:739)
    put_header(s, bc, n_tris, d);
    // (the header's counts place the arrays; A.prim, A.primf, A.cone: per-eye data, filled on the device by
    // rt_prepare_kernel)
    const rt::SceneArrays A = rt::scene_arrays(d);
    const int ns = d->n_stride;
    put_materials(s, d);
    if (int rc = put_board(s, bc, d)) return rc;
    put_spheres(s, bc, ns, writable(A.sph), writable(A.sphf));
    put_light_cones(s, ns, A.sph, writable(A.lightf));
    put_meshes(s, bc, writable(A.mesh), writable(A.tri));
    prove_hits_inside(s, bc, A.sph, A.mesh, d);
    return RT_OK;
}

// The motion record of rt_set_motion (rt_layout.hpp DevMotion) for the flattened scene `blob`, the scene-local sphere
// centres cl[3 n] that scene was built from and the displacements disp[3 n] (null: none).  For sphere k with the
// stored world centre c0 = cl + bc, every sample's centre c = (cl + sigma d) + bc, |sigma| < 1, lies within
//     rho - r,   rho = (r + |d|) (1 + 2^-30) + 2^-40 max_i(|cl_i| + |d_i| + |bc_i|)
// of c0: |sigma d| < |d|, and the three roundings of c and the one of c0 move a component by at most
// 2^-51 (|cl_i| + |d_i| + |bc_i|).  So the sample's sphere lies inside the SWEPT sphere (c0, rho), and
//  * the FP32 filter record of sphere k is filter_record on (c0, rho): the filter rejects a ray only when its
//    line misses the swept sphere, by the margin that DESIGN.md 5h turns into "the exact test on c computes disc < 0";
//  * hits_inside / hits_lim2 are hits_limit's proof with every sphere's extent |c0 - bc| + rho: a hit point of
//    a sample lies on a sphere inside the swept one.  The other extents (board corners, meshes' bounding spheres) are
//    read back from the record; the flag is only ever set where the scene's own is.
int rt_build_motion(const std::vector<unsigned char>& blob, const double* cl, const double* disp, int n,
                    std::vector<unsigned char>* out) {
    const rt::DevScene* d = reinterpret_cast<const rt::DevScene*>(blob.data());
    if (n != d->n_spheres) return rt_fail(RT_EINVAL, "rt_set_motion: n_spheres is not the uploaded scene's");
    const int ns = d->n_stride;
    const rt::SceneArrays A = rt::scene_arrays(d);
    out->assign(rt::motion_bytes_for(ns), 0);
    rt::DevMotion* M = reinterpret_cast<rt::DevMotion*>(out->data());
    rt::DevMotionSphere* ms = writable(rt::motion_arrays(M, ns).ms);
    rt::DevSphereF* sphf = writable(rt::motion_arrays(M, ns).sphf);
    const HP bc = hp(d->bc);
    put(M->pos, bc);
    M->n_stride = ns;
    M->hits_inside = 0;
    M->hits_lim2 = -1.0;
    double far = 0.0, rmin = kInf;
    for (int k = 0; k < n; ++k) {
        const HP c = hp(cl + 3 * k), dk = disp ? hp(disp + 3 * k) : hp(0.0, 0.0, 0.0);
        put(ms[k].cl, c);
        put(ms[k].d, dk);
        const double r = std::sqrt(A.sph[k].r2) * (1.0 + 0x1p-50);              // >= |radius|
        const double m = std::max(std::fabs(c.x) + std::fabs(dk.x) + std::fabs(bc.x),
                                  std::max(std::fabs(c.y) + std::fabs(dk.y) + std::fabs(bc.y),
                                           std::fabs(c.z) + std::fabs(dk.z) + std::fabs(bc.z)));
        const double rho = (r + length(dk)) * (1.0 + 0x1p-30) + 0x1p-40 * m;
        const HP rel = hp(A.sph[k].c) - bc;
        sphf[k] = filter_record(rel, rho * rho);
        far = std::max(far, length(rel) + rho);
        rmin = std::min(rmin, std::sqrt(A.sph[k].r2));
    }
    for (int k = n; k < ns; ++k) sphf[k].rm = -std::numeric_limits<float>::infinity();   // padding: never a hit (cl = d = 0)
    if (d->hits_inside && d->bound_on && d->inner2 > 0) {
        if (d->has_board) {
            const HP p1 = hp(d->tri[0].v0);
            const HP corner[4] = {p1, p1 + hp(d->tri[0].u), p1 + hp(d->tri[0].v), p1 + hp(d->tri[1].v)};
            for (const HP& p : corner) far = std::max(far, length(p - bc));
        }
        for (int m = 0; m < d->n_meshes; ++m) far = std::max(far, length(hp(A.mesh[m].bc) - bc) + std::sqrt(A.mesh[m].br2));
        double lim2;
        if (hits_limit(d->inner2, far, rmin, length(bc), &lim2)) {
            M->hits_inside = 1;
            M->hits_lim2 = std::min(d->hits_lim2, lim2);
        }
    }
    return RT_OK;
}

// R = G = B bit for bit in every frame of the scene: rayTraceRay's colour (:1213-1247) is built from the
// light colours, the material terms and scalar factors by component-wise products and sums only, and every
// decision (hits, shadows, which continuations, :1221, :1230-1247) is the same for the three channels (it
// depends on geometry and on "any component != 0" tests), so equal components in every term that enters the
// sum give equal channels.  Checked: the materials the scene's objects carry and every light colour.
extern "C" int rt_scene_achromatic(const rt_scene* s, int* out) {
    if (!s || !out) return rt_fail(RT_EINVAL, "rt_scene_achromatic: null pointer");
    *out = 0;
    auto grey = [](const double v[3]) { return v[0] == v[1] && v[1] == v[2]; };
    auto grey_mat = [&](const rt_material& m) {
        return grey(m.ambient) && grey(m.diffuse) && grey(m.specular) && grey(m.transparency);
    };
    if (s->n_lights > 0 && !s->lights) return rt_fail(RT_EINVAL, "rt_scene_achromatic: null lights");
    if (s->n_meshes > 0 && !s->meshes) return rt_fail(RT_EINVAL, "rt_scene_achromatic: null meshes");
    bool ok = true;
    if (s->has_board) ok = ok && grey_mat(s->white_square) && grey_mat(s->black_square);
    if (s->n_spheres > 0) ok = ok && grey_mat(s->sphere_material);
    for (int m = 0; m < s->n_meshes && ok; ++m)
        ok = grey_mat(s->meshes[m].kind == RT_MESH_TETRAHEDRON ? s->tetrahedron_material : s->cube_material);
    for (int k = 0; k < s->n_lights && ok; ++k) ok = grey(s->lights[k].color);
    *out = ok ? 1 : 0;
    return RT_OK;
}

// The sky verdict of every 8 x 8 tile of a frame (include/rt_diag.h), evaluated on the host with the functions the
// render kernel's cone phase runs (rt_cone.hpp): the per-eye records as rt_prepare_kernel writes them, the tile
// geometry as render_body forms it.
extern "C" int rt_diag_sky_tiles(const rt_scene* scene, const rt_camera* cam, int width, int height,
                                 const rt_rows* rows, uint8_t* out, size_t n) {
    if (!cam || !out || width <= 0 || height <= 0) return rt_fail(RT_EINVAL, "rt_diag_sky_tiles: bad arguments");
    std::vector<unsigned char> blob;
    int rc = rt_build_dev_scene(scene, &blob);
    if (rc) return rc;
    int nl = 0;
    rc = rt_local_rows(height, rows, &nl);
    if (rc) return rc;
    const int tiles_x = (width + 7) / 8, tiles_y = (nl + 7) / 8;
    if (n != (size_t)tiles_x * tiles_y) return rt_fail(RT_EINVAL, "rt_diag_sky_tiles: out must hold one byte per tile");
    memset(out, 0, n);
    const rt::DevScene* d = reinterpret_cast<const rt::DevScene*>(blob.data());
    const int np = d->n_padded;
    // the instances that take the early-out: opaque, mesh-free scenes whose cone mask covers every sphere
    if (d->tree || d->transparent || d->n_meshes > 0 || np < rt::kPrimaryConeMin || np > 64) return RT_OK;
    const rt::DevSphere* sph = rt::scene_arrays(d).sph;
    const double* eye = cam->eye;
    rt::DevSphereCone cone[64];
    for (int k = 0; k < np; ++k) {
        const HP dP = hp(sph[k].c) - hp(eye);                                   // as rt_prepare_kernel
        cone[k] = rt::sphere_cone_record(dP.x, dP.y, dP.z, dot(dP, dP), sph[k].r2);
    }
    rt::DevBoardEdge edge[4];
    for (int e = 0; e < 4; ++e) edge[e] = rt::board_edge_record(d, eye[0], eye[1], eye[2], e);
    double right[3], upp[3];
    rt_camera_basis(cam, right, upp);
    const rt::ConeCam C = rt::cone_camera(cam->look_at, right, upp, eye, cam->pitch, cam->bottom_x, cam->bottom_y,
                                          width, height);
    // image row (within its frame) of local row lr, defined past the last row as the kernel's global_row_of is
    const bool banded = rows && rows->n_ranks > 1;
    const int frames = frames_of(rows), frame_rows = nl / frames;
    const int hb = banded ? rows->band_height : height, G = banded ? rows->n_ranks : 1, rank = banded ? rows->rank : 0;
    auto row_of = [&](int lr) {
        if (frames > 1) lr %= frame_rows;
        return G <= 1 ? lr : ((lr / hb) * G + rank) * hb + (lr - (lr / hb) * hb);
    };
    const float h = 3.5f, half_diag = sqrtf(h * h + h * h);
    for (int ty = 0; ty < tiles_y; ++ty) {
        // the block's rows must be 8 consecutive image rows of one frame (the gate of primary_cone_mask)
        const int lr0 = ty * 8, ja = row_of(lr0), jb = row_of(lr0 + 7);
        if (!(frames <= 1 || lr0 / frame_rows == (lr0 + 7) / frame_rows) || jb - ja != 7) continue;
        for (int tx = 0; tx < tiles_x; ++tx)
            out[(size_t)ty * tiles_x + tx] = rt::sky_tile(C, cone, np, edge, (float)(tx * 8 + cam->bottom_x) + h,
                                                          (float)(ja + cam->bottom_y) + h, half_diag);
    }
    return RT_OK;
}

// The run plan of a grid of sky verdicts (include/rt_diag.h), tile by tile through the function the device's table
// kernel runs (rt_cone.hpp sky_run_at).
extern "C" int rt_diag_sky_run_plan(const uint8_t* sky, int tiles_x, int tiles_y, int run_max, int32_t* run,
                                    int* positions) {
    if (!sky || !run || !positions || tiles_x <= 0 || tiles_y <= 0 || run_max < 1)
        return rt_fail(RT_EINVAL, "rt_diag_sky_run_plan: bad arguments");
    int n = 0;
    for (int ty = 0; ty < tiles_y; ++ty) {
        const uint8_t* v = sky + (size_t)ty * tiles_x;
        int32_t* r = run + (size_t)ty * tiles_x;
        for (int x = 0; x < tiles_x; ++x) {
            r[x] = rt::sky_run_at(tiles_x, run_max, x, [&](int q) { return v[q] != 0; });
            n += r[x] >= 0;
        }
    }
    *positions = n;
    return RT_OK;
}

// The class of every tile (include/rt_diag.h), through the function the device's class kernel runs (rt_cone.hpp
// tile_sphere_free).
extern "C" int rt_diag_tile_class_plan(const uint64_t* cone, const uint8_t* sky, const uint64_t* masks, int tiles,
                                       int slots, int n_spheres, uint8_t* out) {
    if (!cone || !out || tiles < 0 || slots < 0 || (slots > 0 && !masks) || n_spheres < 0 || n_spheres > 64)
        return rt_fail(RT_EINVAL, "rt_diag_tile_class_plan: bad arguments");
    for (int t = 0; t < tiles; ++t)
        out[t] = rt::tile_sphere_free(cone[t], sky && sky[t] != 0, slots > 0 ? masks + (size_t)t * slots : nullptr, slots,
                                      n_spheres)
                     ? 1
                     : 0;
    return RT_OK;
}

// The `sky` word of a dispatch record (include/rt_diag.h), through the function the device's table kernels run (rt_cone.hpp
// disp_sky_word).
extern "C" int rt_diag_disp_sky_word(uint32_t run, int sphere_free, int flat, uint32_t* word) {
    if (!word || run > rt::kDispRunMax || (sphere_free && run != 0))
        return rt_fail(RT_EINVAL, "rt_diag_disp_sky_word: bad arguments");
    *word = rt::disp_sky_word(run, sphere_free != 0, flat != 0);
    return RT_OK;
}

// The flat class's wave-uniform gates for `scene` seen from `eye` (include/rt_diag.h), through the function the device runs
// (rt_cone.hpp flat_gates_of) on the scene record the device gets; and hits_ok for that eye as rt_prepare_kernel sets it
// (rt_device.hpp hits_ok_from: the same expression).
extern "C" int rt_diag_flat_gates(const rt_scene* scene, const double* eye, int* gates, int* hits_ok, double* skip_y) {
    if (!eye || !gates || !hits_ok) return rt_fail(RT_EINVAL, "rt_diag_flat_gates: bad arguments");
    std::vector<unsigned char> blob;
    const int rc = rt_build_dev_scene(scene, &blob);
    if (rc) return rc;
    const rt::DevScene* d = reinterpret_cast<const rt::DevScene*>(blob.data());
    *gates = rt::flat_gates_of(d->has_board != 0, d->board_skip_y, eye[1]) ? 1 : 0;
    const double dx = eye[0] - d->bc[0], dy = eye[1] - d->bc[1], dz = eye[2] - d->bc[2];
    *hits_ok = ((d->hits_inside != 0) & (dx * dx + dy * dy + dz * dz <= d->hits_lim2)) ? 1 : 0;
    if (skip_y) *skip_y = d->board_skip_y;
    return RT_OK;
}

extern "C" int rt_write_ppm(const char* path, const uint8_t* px, int W, int H, int channels) {
    // writePpmScreenshot (Hw4/ppm.cpp:15-25): header "P6 W H 255\n", then the bottom-up GL image's rows
    // written top-down (image[3*w*(h-1-i)]).
    if (!path || !px || W <= 0 || H <= 0 || (channels != 1 && channels != 3 && channels != 4))
        return rt_fail(RT_EINVAL, "rt_write_ppm: bad args");
    FILE* f = fopen(path, "wb");
    if (!f) return rt_fail(RT_EINVAL, std::string("rt_write_ppm: cannot open ") + path);
    fprintf(f, "P6 %d %d 255\n", W, H);
    std::vector<unsigned char> row((size_t)W * 3);
    for (int i = 0; i < H; ++i) {
        const uint8_t* src = px + (size_t)(H - 1 - i) * W * channels;
        for (int x = 0; x < W; ++x) {                        // GRAY8 (channels 1): R = G = B
            row[3 * x] = src[channels * x];
            row[3 * x + 1] = src[channels * x + (channels > 1 ? 1 : 0)];
            row[3 * x + 2] = src[channels * x + (channels > 1 ? 2 : 0)];
        }
        if (fwrite(row.data(), 1, row.size(), f) != row.size()) {
            fclose(f);
            return rt_fail(RT_EINVAL, "rt_write_ppm: short write");
        }
    }
    fclose(f);
    return RT_OK;
}
