// rt_cone.hpp — the per-wave primary-ray bounds, in functions the kernels and the host share (plain C++ under a
// host compiler, __host__ __device__ under hipcc): the tile axis and chord radius of an 8 x 8 block's rays, the
// per-eye cone record of a sphere, the per-eye edge records of the board, and the two tests a wave makes with them.
// The render kernel evaluates them in its cone phase (rt_device.hpp primary_cone_mask); the host evaluates the same
// functions tile by tile for rt_diag_sky_tiles (rt_host.cpp), so the soundness of the "sky tile" verdict — no primary
// ray of the tile hits anything — is checkable without a device.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rt_layout.hpp"

// FP32 square root and reciprocal of the wave-culling tests: on the device the hardware instructions
// (v_sqrt_f32, v_rcp_f32, 1 ulp: relative error < 2^-22 on normal operands) instead of the correctly rounded
// sequences (scaling, Newton and fixup steps around them: ~10 instructions each).  The culling tests only need
// conservative bounds, and their margins (R inflated by 2^-12 relative, chord limits by 2^-14 absolute, shadow
// cones by 2^-16 in cos, the primary cone's slack >= 2^-16) are > 2^6 times the extra error; 0, +inf and NaN keep
// their meaning (sqrt(0) = 0, rcp(+inf) = 0, NaN propagates and fails the `>` compares, i.e. keeps the sphere).
// The host evaluates the correctly rounded forms: its verdicts are sound for the same reason, and equal the
// device's except where a test lands within that error of its threshold.

namespace rt {

RT_HD float msqrt(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}
RT_HD float mrcp(float x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
RT_HD float mdiv(float a, float b) {
#ifdef __HIP_DEVICE_COMPILE__
    return a * __builtin_amdgcn_rcpf(b);
#else
    return a / b;
#endif
}
RT_HD float mchord_of_sin(float s) { return s * msqrt(mdiv(2.0f, 1.0f + msqrt(fmaxf(0.0f, 1.0f - s * s)))); }

// (float)x rounded towards +inf.
RT_HD float float_ru(double x) {
#ifdef __HIP_DEVICE_COMPILE__
    return __double2float_ru(x);
#else
    const float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
#endif
}

// FP32 camera of the per-wave tests, and the bound `slack` on its error as a chord distance: every FP32 coordinate
// is below M in magnitude and carries < 16 roundings, and |sp - eye| >= |look - eye| (right, up' are orthogonal to
// look - eye), so direction errors are < 64 eps32 M / |look - eye|.  slack = 8: no test may cull.
struct ConeCam {
    float look[3], right[3], upp[3], eye[3], pitch, slack;
};
inline ConeCam cone_camera(const double look[3], const double right[3], const double upp[3], const double eye[3],
                           double pitch, int bottom_x, int bottom_y, int W, int H) {
    ConeCam C;
    double M = 1.0, D2 = 0.0;
    for (int q = 0; q < 3; ++q) {
        C.look[q] = (float)look[q];
        C.right[q] = (float)right[q];
        C.upp[q] = (float)upp[q];
        C.eye[q] = (float)eye[q];
        const double s = fabs(look[q]) + fabs(eye[q]);
        M = M > s ? M : s;
        D2 += (look[q] - eye[q]) * (look[q] - eye[q]);
    }
    C.pitch = (float)pitch;
    M += fabs(pitch) * (fabs((double)bottom_x) + fabs((double)bottom_y) + W + H + 16.0);
    const double slack = 0x1p-16 + 64.0 * 0x1p-24 * M / sqrt(D2);
    C.slack = (D2 > 0.0 && slack < 0.25) ? (float)slack : 8.0f;
    return C;
}

// The rays of a wave go from the eye through the screen points of its bw x bh block, all within R = half_diag pitch
// of the block centre c (half_diag = |((bw - 1) / 2, (bh - 1) / 2)|, centre at pixel (ci, cj) of the image plane),
// hence (exact geometry) within angle asin(R / |c - eye|) of a = unit(c - eye): chord distance |u - a| <= rho for
// every ray direction u, where rho includes `slack`, the bound on the FP32 error of a and of the tests made with it.
// ok = false (the eye too close to the screen, or a NaN): nothing may be concluded.
struct WaveAxis {
    float ax, ay, az, rho;
    bool ok;
};
RT_HD WaveAxis wave_axis(const float look[3], const float right[3], const float upp[3], const float eye[3],
                         float pitch, float ci, float cj, float half_diag, float slack) {
    const float a_r = pitch * ci, a_u = pitch * cj;
    float dx = fmaf(a_u, upp[0], fmaf(a_r, right[0], look[0])) - eye[0];
    float dy = fmaf(a_u, upp[1], fmaf(a_r, right[1], look[1])) - eye[1];
    float dz = fmaf(a_u, upp[2], fmaf(a_r, right[2], look[2])) - eye[2];
    const float dn = msqrt(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    const float sn = mdiv((half_diag * 1.001f) * pitch, dn);
    WaveAxis w;
    w.ok = sn < 0.5f;
    w.rho = mchord_of_sin(sn) + slack;
    const float idn = mrcp(dn);
    w.ax = dx * idn, w.ay = dy * idn, w.az = dz * idn;
    return w;
}

// Cone of directions from the eye that can hit a sphere (dP = C - eye, dd = |dP|^2 as the exact test computes
// them, r2): f32(unit(dP)) and the chord radius, rounded up.  A ray that hits has |u - v| <= chord; r' covers the
// FP64 test's rounding (disc error < 4 ulp of 3 D^2 < D^2 2^-48): r'^2 = r2 (1 + 2^-20) + D^2 2^-46.
RT_HD DevSphereCone sphere_cone_record(double dPx, double dPy, double dPz, double dd, double r2) {
    DevSphereCone cn;
    if (!(r2 >= 0.0)) {                                     // padding: never kept
        cn.vx = cn.vy = cn.vz = 1e30f;
        cn.chord = 0.0f;
        return cn;
    }
    const double D = sqrt(dd);
    const double rp = sqrt(r2 * (1.0 + 0x1p-20) + dd * 0x1p-46);
    const double sn = rp / D;
    if (!(sn < 0.999)) {                                    // eye inside / at the sphere: always kept
        cn.vx = cn.vy = cn.vz = 0.0f;
        cn.chord = 4.0f;
    } else {
        const double ch = sn * sqrt(2.0 / (1.0 + sqrt(1.0 - sn * sn))) + 0x1p-20;
        cn.vx = (float)(dPx / D); cn.vy = (float)(dPy / D); cn.vz = (float)(dPz / D);
        cn.chord = float_ru(ch);
    }
    return cn;
}

// The wave must test the sphere: |a - v| <= rho + chord.  NaNs keep the sphere.
RT_HD bool cone_keeps(const WaveAxis& w, const DevSphereCone& c) {
    const float ex = w.ax - c.vx, ey = w.ay - c.vy, ez = w.az - c.vz;
    const float lim = w.rho + c.chord;
    return !(fmaf(ex, ex, fmaf(ey, ey, ez * ez)) > lim * lim);
}

// ---- The board, seen from the eye ----
// The directions from the eye E that hit the board quad Q (convex, in the plane y = v0.y) are the intersection of
// four half-spaces m_e . u >= 0, one per edge (A, B) of Q: m_e = +-unit((A - E) x (B - E)), oriented towards Q's
// centre.  A wave whose axis has m_e . a < -(rho + mg) for one edge misses the board with every ray: m_e . u =
// m_e . a + m_e . (u - a) <= m_e . a + rho < -mg.  The record of edge e holds f32(m_e) and the margin mg, which covers
// (S = the largest coordinate magnitude of the eye and the corners + the largest distance between them, u = 2^-53):
//  * the board test's own FP64 rounding.  For the reference's board (DevScene::board_fast: normal (0, -1, 0), corners
//    v0 + {0, L}^2, the only board the proof is made for) board_hit hits only if its computed w = q - v0 lies in
//    [-2 E L, L (1 + 2 E)]^2, E < 2^-45 (the bound at board_hit: the position decision hits strictly inside Q, the
//    exact triangles' s, t err by E), and q = E + m d is a point of the ray up to u (|E| + 2 |m d|), the plane
//    parameter m = num / nd up to 2 u relative (num, nd one rounding each; nd = -d.y exactly) with m >= eps > 0: the
//    ray's exact plane point lies within eps_abs = 2^-40 S of Q, ahead of the eye.  Its direction is within
//    2 eps_abs / |h| of a direction that hits Q exactly (h = the eye's height over the plane, <= every |q - E|):
//    t_h = 2^-39 S / |h|.
//  * the FP64 error of m_e.  A - E, B - E err by < 4 u S each (the corner's own rounding and the subtraction's), the
//    cross product c by < 15 u S^2 < 2^-48 S^2, so unit(c) errs by r_c = 2^-46 S^2 / |c| (normalisation included);
//    the orientation s = c . (centre - E) errs by < 2^-47 S^3 and is trusted when |s| > 2^-40 S^3.
//  * the FP32 rounding of m_e (sqrt(3) 2^-24), of the dot product (3 roundings of terms <= 1 + 2^-20) and of rho + mg
//    (2^-24 (rho + mg), rho + mg < 2): together < 2^-20.  (The FP32 error of a itself is in rho: wave_axis.)
// mg = 2^-20 + (t_h + r_c) (1 + 2^-20), rounded up.  "Cannot prove" is mg = +inf: the eye within 2^-19 S of the board
// plane (t_h > 2^-20) or the cross product ill-conditioned (r_c > 2^-20, |s| too small), any non-finite input, or a
// board that is not the reference's.  A scene without a board misses it trivially: m = 0, mg = -inf.
RT_HD DevBoardEdge board_edge_record(const DevScene* g, double ex, double ey, double ez, int e) {
    DevBoardEdge r;
    r.mx = r.my = r.mz = 0.0f;
    r.mg = -INFINITY;
    if (!g->has_board) return r;
    r.mg = INFINITY;
    if (!g->board_fast) return r;
    const double* v0 = g->tri[0].v0;
    const double L = g->tri[0].u[0];
    const double cx[4] = {v0[0], v0[0] + L, v0[0] + L, v0[0]}, cz[4] = {v0[2], v0[2], v0[2] + L, v0[2] + L};
    const int f = (e + 1) & 3;
    const double ax = cx[e] - ex, ay = v0[1] - ey, az = cz[e] - ez;
    const double bx = cx[f] - ex, by = ay, bz = cz[f] - ez;
    const double gx = (v0[0] + 0.5 * L) - ex, gz = (v0[2] + 0.5 * L) - ez;
    double S = fabs(ex);
    S = fmax(S, fmax(fabs(ey), fabs(ez)));
    S = fmax(S, fmax(fabs(v0[1]), fmax(fabs(v0[0]) + L, fabs(v0[2]) + L)));
    S += sqrt(fmax(ax * ax + ay * ay + az * az, bx * bx + by * by + bz * bz)) + L;
    double px = ay * bz - az * by, py = az * bx - ax * bz, pz = ax * by - ay * bx;
    const double pn = sqrt(px * px + py * py + pz * pz);
    const double s = px * gx + py * ay + pz * gz;
    const double t_h = 0x1p-39 * S / fabs(ay), r_c = 0x1p-46 * S * S / pn;
    if (!(t_h <= 0x1p-20) || !(r_c <= 0x1p-20) || !(fabs(s) > 0x1p-40 * S * S * S)) return r;
    const double sg = s < 0.0 ? -1.0 : 1.0;
    px = sg * px / pn, py = sg * py / pn, pz = sg * pz / pn;
    if (!(fabs(px) <= 1.0 && fabs(py) <= 1.0 && fabs(pz) <= 1.0)) return r;      // (a NaN: cannot prove)
    r.mx = (float)px, r.my = (float)py, r.mz = (float)pz;
    r.mg = float_ru(0x1p-20 + (t_h + r_c) * (1.0 + 0x1p-20));
    return r;
}

// Every ray of the wave is on the outer side of this edge's plane: the wave misses the board.  NaNs prove nothing.
RT_HD bool edge_misses(const WaveAxis& w, const DevBoardEdge& m) {
    const float d = fmaf(w.az, m.mz, fmaf(w.ay, m.my, w.ax * m.mx));
    return d < -(w.rho + m.mg);
}

// The sky verdict of one wave, as the kernel's cone phase reaches it (host): np padded spheres with their cone
// records, the four edge records, the block centre.  (The kernel's lanes evaluate the same tests, one sphere and one
// edge per lane, and combine them by ballot.)
inline bool sky_tile(const ConeCam& C, const DevSphereCone* cone, int np, const DevBoardEdge edge[4], float ci,
                     float cj, float half_diag) {
    if (np < kPrimaryConeMin || np > 64) return false;
    const WaveAxis w = wave_axis(C.look, C.right, C.upp, C.eye, C.pitch, ci, cj, half_diag, C.slack);
    if (!w.ok) return false;
    for (int k = 0; k < np; ++k)
        if (cone_keeps(w, cone[k])) return false;
    for (int e = 0; e < 4; ++e)
        if (edge_misses(w, edge[e])) return true;
    return false;
}

// The run plan of one tile row of a cached view's dispatch, tile by tile (rt_plain.hip rt_run_plan_kernel on the device,
// rt_diag_sky_run_plan on the host): the row's n tiles in dispatch order, sky(x) their verdicts.  A tile that is not sky
// is a dispatch position of its own (0).  A maximal streak of sky tiles is cut from its first tile into runs of at most
// run_max tiles, each one position: its first tile is the run's head (the run's length, 1 .. run_max), the others are
// covered by it (-1).  So runs never leave the row, every tile belongs to exactly one position, and run_max = 1 is one
// position per tile.
template <class Sky>
RT_HD int sky_run_at(int n, int run_max, int x, Sky sky) {
    if (!sky(x)) return 0;
    int first = x;
    while (first > 0 && sky(first - 1)) --first;
    if ((x - first) % run_max != 0) return -1;
    int len = 1;
    while (len < run_max && x + len < n && sky(x + len)) ++len;
    return len;
}

// The class of one tile of a calibrated view, decided where its dispatch record is built (rt_plain.hip rt_class_kernel on
// the device, rt_diag_tile_class_plan on the host): the tile is sphere-free when it traces (not sky) and neither its
// primary cone mask nor any of its `slots` level masks (rt_device.hpp LevelMasks: the ray masks of levels 1 .. B, the
// shadow masks of every light at every level; a slot no wave reached reads 0) keeps one of the scene's np <= 64 (padded)
// spheres.  Every mask is conservative — a clear bit proves that no ray of the tile's wave at that level can meet the
// sphere — so no primary, reflected or shadow ray of such a tile touches a sphere, and the fast kernels trace it without
// the sphere code (rt_render.hpp render_body).  Bits at or above np are ignored.
RT_HD bool tile_sphere_free(uint64_t cone, bool sky, const uint64_t* masks, int slots, int np) {
    if (sky || np > 64) return false;
    uint64_t any = cone;
    for (int k = 0; k < slots; ++k) any |= masks[k];
    const uint64_t bits = np >= 64 ? ~0ull : ((1ull << (np < 0 ? 0 : np)) - 1);
    return (any & bits) == 0;
}

// The `sky` word of a dispatch record (rt_render.hpp DispRec), built by the two table kernels of rt_plain.hip and, on the
// host, by rt_diag_disp_sky_word.  `run` is what the word holds for a tile outside the classes: 0 for a tracing tile, the
// run length (at most kDispRunMax) for a sky record.  A sphere-free tile — a tracing tile, run = 0 — carries
// kDispSphereFree and, when it is also flat (rt_device.hpp trace_flat), kDispFlat beside it: flat is never set alone, and
// no run length reaches either bit.
constexpr uint32_t kDispSphereFree = 0x80000000u, kDispFlat = 0x40000000u, kDispRunMax = 65535u;
constexpr uint32_t kDispClassBits = kDispSphereFree | kDispFlat;
static_assert(kDispRunMax < kDispFlat, "run lengths stay below the class bits");
// The wave-uniform gates of the flat class (rt_device.hpp trace_flat has the proof they feed; rt_plain.hip rt_flat_kernel
// on the device, rt_diag_flat_gates on the host): the scene has its board, and the eye passes the board's origin skip
// (origin_skip: |eye.y| <= DevScene::board_skip_y, which is -1 where the skip is not proven).  NaN fails the compare.
RT_HD bool flat_gates_of(bool has_board, double board_skip_y, double eye_y) {
    return has_board & (fabs(eye_y) <= board_skip_y);
}

RT_HD uint32_t disp_sky_word(uint32_t run, bool sphere_free, bool flat) {
    if (!sphere_free) return run;
    return kDispSphereFree | (flat ? kDispFlat : 0u);
}

}  // namespace rt
