// ref_harness.cpp — TEST INFRASTRUCTURE (oracle/_ref build only; appended after the reference's own
// hot-path source ranges by oracle/Makefile, so every class and function used below is the reference's).
//
// Scenes are built exactly the way the reference app builds them (loadScene, MySdlApplication.cpp:
// 1495-1539): a g_scene-like Shape (:590), CheckerBoard(Point(0,0,0)) first (:1442-1443), then the
// children in the order of `children` (3-char tokens: 'S'|'T'|'C' + square): Sphere(
// convertStringCoordinate(sq) [+ (0,yoff,0)], r), Tetrahedron(convertStringCoordinate(sq), edge),
// Cube(convertStringCoordinate(sq), edge); lights Light(color, BOARD_POSITION +
// (0,3.5*SQUARE_EDGE_SIZE,0) + convertStringCoordinate(sq)) (:1511).  Pixels use the deterministic
// primary ray of SURVEY.md Appendix B with the rayTraceScreen basis (:1270-1279) and are shaded by the
// reference rayTraceRay (:1184-1249).
#include <omp.h>
#include <cstdint>

namespace {

struct RefScene {
    Shape* scene;
    vector<Light> lights;
};

// The g_scene-like root with the board as its first child, and the light list of one frame (lights by square).
RefScene root_and_lights(const char* light_sq, const double* light_col, int n_lights) {
    RefScene r;
    r.scene = new Shape(Point(BOARD_POSITION), Material(), sqrt((double)3) * BOARD_HALF_SIZE, false);
    r.scene->addRayObject(new CheckerBoard(Point(0.0, 0.0, 0.0)));
    for (int k = 0; k < n_lights; ++k) {
        string sq(light_sq + 2 * k, 2);
        Point pos = Point(BOARD_POSITION) + Point(0.0, 3.5 * SQUARE_EDGE_SIZE, 0.0) + convertStringCoordinate(sq);
        r.lights.push_back(Light(Point(light_col + 3 * k), pos));
    }
    return r;
}

RefScene build(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
               const double* mesh_edge, const char* light_sq, const double* light_col, int n_lights) {
    RefScene r = root_and_lights(light_sq, light_col, n_lights);
    int ks = 0, km = 0;
    for (int c = 0; c < n_children; ++c) {
        char type = children[3 * c];
        string sq(children + 3 * c + 1, 2);
        Point p = convertStringCoordinate(sq);
        if (type == 'S') {
            if (sph_yoff) p = p + Point(0.0, sph_yoff[ks], 0.0);
            r.scene->addRayObject(new Sphere(p, sph_r[ks]));
            ++ks;
        } else if (type == 'T') {
            r.scene->addRayObject(new Tetrahedron(p, mesh_edge[km++]));
        } else {
            r.scene->addRayObject(new Cube(p, mesh_edge[km++]));
        }
    }
    return r;
}

// The same g_scene with every sphere given by its scene-local centre instead of a board square (the tangent
// constructions of tests/tangent_common.py place spheres anywhere): the board first, then Sphere(centres[k], radii[k])
// in order; the lights by square, as build() places them.
RefScene build_at(const double* centres, const double* radii, int n_spheres, const char* light_sq,
                  const double* light_col, int n_lights) {
    RefScene r = root_and_lights(light_sq, light_col, n_lights);
    for (int k = 0; k < n_spheres; ++k) r.scene->addRayObject(new Sphere(Point(centres + 3 * k), radii[k]));
    return r;
}

int material_id(Material m) {
    if (m.transparency().x() != 0) return 3;      // g_tetrahedronMaterial
    if (m.ambient().y() == 0 && m.ambient().x() != 0) return 4;   // g_cubeMaterial (red)
    if (m.specular().x() == 0) return 1;          // g_blackSquare
    if (m.ambient().x() != 0) return 0;           // g_whiteSquare
    return 2;                                     // g_sphereMaterial
}

}  // namespace

extern "C" {

// Render rows [row_begin, row_end) of a W x H frame; rgb has (row_end-row_begin)*W*3 doubles.
int ref_render(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
               const double* mesh_edge, const char* light_sq, const double* light_col, int n_lights, int W, int H,
               int depth,
               double pitch, int row_begin, int row_end, double* rgb, int nthreads) {
    RefScene rs = build(children, n_children, sph_yoff, sph_r, mesh_edge, light_sq, light_col, n_lights);
    Point camera(CAMERA_POSITION);
    Point lookAt(LOOK_AT_VECTOR);
    Point up(UP_VECTOR);
    Point lookDirection = lookAt - camera;          // rayTraceScreen basis, :1270-1277
    Point right = lookDirection * up;
    right.normalize();
    up = right * lookDirection;
    up.normalize();
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 1)
    for (int j = row_begin; j < row_end; ++j) {
        for (int i = 0; i < W; ++i) {
            Point sp = (lookAt + (pitch * (double)(i - W / 2)) * right) + (pitch * (double)(j - H / 2)) * up;
            Point color(0.0, 0.0, 0.0);
            rayTraceRay(*rs.scene, rs.lights, Line(camera, sp), color, (unsigned)depth);
            size_t k = ((size_t)(j - row_begin) * W + i) * 3;
            rgb[k] = color.x(); rgb[k + 1] = color.y(); rgb[k + 2] = color.z();
        }
    }
    delete rs.scene;
    return 0;
}

// Sampled pixels (i[k], j[k]) of a W x H frame.
int ref_render_pixels(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
                      const double* mesh_edge, const char* light_sq, const double* light_col, int n_lights,
                      int W, int H, int depth, double pitch, const int32_t* pi, const int32_t* pj, int n,
                      double* rgb, int nthreads) {
    RefScene rs = build(children, n_children, sph_yoff, sph_r, mesh_edge, light_sq, light_col, n_lights);
    Point camera(CAMERA_POSITION);
    Point lookAt(LOOK_AT_VECTOR);
    Point up(UP_VECTOR);
    Point lookDirection = lookAt - camera;
    Point right = lookDirection * up;
    right.normalize();
    up = right * lookDirection;
    up.normalize();
    if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel for schedule(dynamic, 64)
    for (int k = 0; k < n; ++k) {
        int i = pi[k], j = pj[k];
        Point sp = (lookAt + (pitch * (double)(i - W / 2)) * right) + (pitch * (double)(j - H / 2)) * up;
        Point color(0.0, 0.0, 0.0);
        rayTraceRay(*rs.scene, rs.lights, Line(camera, sp), color, (unsigned)depth);
        rgb[3 * k] = color.x(); rgb[3 * k + 1] = color.y(); rgb[3 * k + 2] = color.z();
    }
    delete rs.scene;
    return 0;
}

// rayTraceRay on arbitrary rays Line(starts[k], ends[k]).
int ref_trace_rays(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
                   const double* mesh_edge, const char* light_sq, const double* light_col, int n_lights,
                   const double* starts,
                   const double* ends, int n, int depth, double* rgb) {
    RefScene rs = build(children, n_children, sph_yoff, sph_r, mesh_edge, light_sq, light_col, n_lights);
#pragma omp parallel for schedule(dynamic, 64)
    for (int k = 0; k < n; ++k) {
        Point color(0.0, 0.0, 0.0);
        rayTraceRay(*rs.scene, rs.lights, Line(Point(starts + 3 * k), Point(ends + 3 * k)), color,
                    (unsigned)depth);
        rgb[3 * k] = color.x(); rgb[3 * k + 1] = color.y(); rgb[3 * k + 2] = color.z();
    }
    delete rs.scene;
    return 0;
}

// g_scene.intersection(ray, Point(0,0,0), inter) on arbitrary rays: per ray 12 doubles
// (point, normal, reflectedRay end, transmittedRay end) + hit flag + material id.
int ref_intersect(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
                  const double* mesh_edge, const double* starts, const double* ends, int n, double* out12,
                  int32_t* hit, int32_t* mat) {
    RefScene rs = build(children, n_children, sph_yoff, sph_r, mesh_edge, "", nullptr, 0);
    for (int k = 0; k < n; ++k) {
        Intersection in;
        rs.scene->intersection(Line(Point(starts + 3 * k), Point(ends + 3 * k)), Point(0.0, 0.0, 0.0), in);
        hit[k] = in.intersects() ? 1 : 0;
        mat[k] = -1;
        for (int q = 0; q < 12; ++q) out12[12 * k + q] = 0.0;
        if (hit[k]) {
            Point p = in.point(), nn = in.normal(), e = in.reflectedRay().endPoint();
            Point t = in.transmittedRay().endPoint();
            double* o = out12 + 12 * k;
            o[0] = p.x(); o[1] = p.y(); o[2] = p.z();
            o[3] = nn.x(); o[4] = nn.y(); o[5] = nn.z();
            o[6] = e.x(); o[7] = e.y(); o[8] = e.z();
            o[9] = t.x(); o[10] = t.y(); o[11] = t.z();
            mat[k] = material_id(in.material());
        }
    }
    delete rs.scene;
    return 0;
}

// ref_trace_rays / ref_intersect on a scene whose spheres are given by scene-local centre (build_at).
int ref_trace_rays_at(const double* centres, const double* radii, int n_spheres, const char* light_sq,
                      const double* light_col, int n_lights, const double* starts, const double* ends, int n,
                      int depth, double* rgb) {
    RefScene rs = build_at(centres, radii, n_spheres, light_sq, light_col, n_lights);
#pragma omp parallel for schedule(dynamic, 64)
    for (int k = 0; k < n; ++k) {
        Point color(0.0, 0.0, 0.0);
        rayTraceRay(*rs.scene, rs.lights, Line(Point(starts + 3 * k), Point(ends + 3 * k)), color,
                    (unsigned)depth);
        rgb[3 * k] = color.x(); rgb[3 * k + 1] = color.y(); rgb[3 * k + 2] = color.z();
    }
    delete rs.scene;
    return 0;
}

int ref_intersect_at(const double* centres, const double* radii, int n_spheres, const double* starts,
                     const double* ends, int n, double* out12, int32_t* hit, int32_t* mat) {
    RefScene rs = build_at(centres, radii, n_spheres, "", nullptr, 0);
    for (int k = 0; k < n; ++k) {
        Intersection in;
        rs.scene->intersection(Line(Point(starts + 3 * k), Point(ends + 3 * k)), Point(0.0, 0.0, 0.0), in);
        hit[k] = in.intersects() ? 1 : 0;
        mat[k] = -1;
        for (int q = 0; q < 12; ++q) out12[12 * k + q] = 0.0;
        if (hit[k]) {
            Point p = in.point(), nn = in.normal(), e = in.reflectedRay().endPoint();
            Point t = in.transmittedRay().endPoint();
            double* o = out12 + 12 * k;
            o[0] = p.x(); o[1] = p.y(); o[2] = p.z();
            o[3] = nn.x(); o[4] = nn.y(); o[5] = nn.z();
            o[6] = e.x(); o[7] = e.y(); o[8] = e.z();
            o[9] = t.x(); o[10] = t.y(); o[11] = t.z();
            mat[k] = material_id(in.material());
        }
    }
    delete rs.scene;
    return 0;
}

// The reference's own rayTraceScreen (:1251-1324) on the draw() camera (:1552-1560), rand() seeded with
// `seed` (the app never calls srand: seed 1).  Its glBegin/glColor3d/glVertex2i/glEnd go to the image's
// real libGL with no current context, where they do nothing, so the colours are not observable; what is
// observable is how many rand() calls the frame made: 3 per jittered sample (randomUnit, :1148-1169),
// i.e. the sample counts the convergence test and the colour carry-over produced.  The count is found
// by locating the next three outputs in the stream restarted from `seed`.
uint64_t ref_screen_rand_calls(const char* children, int n_children, const double* sph_yoff, const double* sph_r,
                               const double* mesh_edge, const char* light_sq, const double* light_col,
                               int n_lights, int W, int H, int bottom_x, int bottom_y, unsigned seed,
                               uint64_t max_calls) {
    RefScene rs = build(children, n_children, sph_yoff, sph_r, mesh_edge, light_sq, light_col, n_lights);
    srand(seed);
    rayTraceScreen(*rs.scene, rs.lights, Point(CAMERA_POSITION), Point(LOOK_AT_VECTOR), Point(UP_VECTOR),
                   bottom_x, bottom_y, W, H);
    int a = rand(), b = rand(), c = rand();
    delete rs.scene;
    srand(seed);
    int x0 = rand(), x1 = rand(), x2 = rand();
    for (uint64_t n = 0; n < max_calls; ++n) {
        if (x0 == a && x1 == b && x2 == c) return n;
        x0 = x1; x1 = x2; x2 = rand();
    }
    return ~0ull;
}

// The five material globals the scene classes copy at construction (:583-588): g_whiteSquare, g_blackSquare,
// g_sphereMaterial, g_tetrahedronMaterial, g_cubeMaterial; 13 doubles each (ambient, diffuse, specular,
// transparency, refraction).  ref_get_materials reads them, ref_set_materials replaces them for the scenes
// built afterwards (tests of materials the app never uses, e.g. partially transparent ones: ray trees).
static Material* const g_mats[5] = {&g_whiteSquare, &g_blackSquare, &g_sphereMaterial, &g_tetrahedronMaterial,
                                    &g_cubeMaterial};

void ref_get_materials(double* m) {
    for (int k = 0; k < 5; ++k, m += 13) {
        Material& M = *g_mats[k];
        Point a = M.ambient(), d = M.diffuse(), s = M.specular(), t = M.transparency();
        Point* v[4] = {&a, &d, &s, &t};
        for (int q = 0; q < 4; ++q) {
            m[3 * q] = v[q]->x(); m[3 * q + 1] = v[q]->y(); m[3 * q + 2] = v[q]->z();
        }
        m[12] = M.refraction();
    }
}

// The globals as the reference initialised them (snapshot taken at load, after their definitions in this
// translation unit).
static struct DefaultMats {
    double m[65];
    DefaultMats() { ref_get_materials(m); }
} g_default_mats;

void ref_default_materials(double* m) {
    for (int k = 0; k < 65; ++k) m[k] = g_default_mats.m[k];
}

void ref_set_materials(const double* m) {
    for (int k = 0; k < 5; ++k, m += 13)
        *g_mats[k] = Material(Point(m), Point(m + 3), Point(m + 6), Point(m + 9), m[12]);
}

// convertStringCoordinate (:1326-1346).
void ref_convert_string_coordinate(const char* sq, double out[3]) {
    Point p = convertStringCoordinate(string(sq, 2));
    out[0] = p.x(); out[1] = p.y(); out[2] = p.z();
}

}  // extern "C"
