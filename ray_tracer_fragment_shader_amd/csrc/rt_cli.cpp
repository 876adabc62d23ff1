// rt_cli.cpp — `rt_render`: the reference application's frame flow on the MI355X path.
//
// Reference flow (Hw4/MySdlApplication.cpp): onInit -> initScene2 (stdin dialogue, :1430-1493) ->
// loadScene (:1495-1539) -> every frame draw() (:1541-1563) -> rayTraceScreen -> GL points; a screenshot
// would go through writePpmScreenshot (Hw4/ppm.cpp:15-25).  Here: the same dialogue (or a canonical
// scene) -> rt_load_scene -> rt_render (one HIP launch) -> RGBA8 -> rt_write_ppm.  No SDL/GL window:
// the image goes to a PPM file (the output path the reference already has).
//
//   rt_render --config c2 --out c2.ppm            canonical scene
//   rt_render --config demo --out demo.ppm        initScene's demo (tetrahedron, sphere, cube), 500x500
//   rt_render --stdin --width 500 --height 500 --pitch 1 --out app.ppm < answers.txt
//                                                  initScene2's questions answered on stdin
//   rt_render --config demo --faithful glibc|msvc [--seed S] --out demo_ref.ppm
//                                                  rayTraceScreen exactly as the app runs it (jitter, up to
//                                                  16 adaptive samples, colour carry-over): rt_render_screen
//   rt_render --config c4 --gpus 8 [--band H] [--repeat K] --out c4.ppm
//                                                  one frame's rows split over 8 GPUs (rt_group, RCCL gather to
//                                                  GPU 0); with fewer GPUs than --gpus the
//                                                  contexts share devices and the gather is a device copy
//   rt_render --config c2 --samples 4 --out c2_ss.ppm
//                                                  S x S regular-grid samples per pixel summed in the kernel
//                                                  (rt_render_ss; S in 1, 2, 4, 8 — not the app's jittered mode)
//   rt_render --config c2 --samples 4 --adaptive 8 --out c2_ad.ppm
//                                                  ... only for the pixels whose one-sample RGBA8 differs from a
//                                                  4-neighbour by more than 8 in some channel (rt_render_adaptive;
//                                                  threshold in -1 .. 255), one sample elsewhere
//   rt_render --config c2 --samples 4 --aperture 8 [--focus 0.8] --out c2_dof.ppm
//                                                  depth of field: the S x S samples start on a square lens of
//                                                  half-width 8 around the eye (rt_render_dof); --focus moves the
//                                                  focal plane to RATIO times the look-at distance (rt_camera_focus)
//   rt_render --config c2 --samples 4 --light-size 40 [--aperture 8 [--focus 0.8]] --out c2_soft.ppm
//                                                  soft shadows: every light a square panel of half-width 40 in the
//                                                  world xz-plane, one of its S x S points per sample (rt_render_soft)
//   rt_render --config c2 --samples 4 --shutter 1 --move 0:40,0,0 [--move K:DX,DY,DZ ...] [--light-size 40]
//             [--aperture 8 [--focus 0.8]] --out c2_motion.ppm
//                                                  motion blur: sphere 0 moves by +-(40, 0, 0) (scene-local) during the
//                                                  exposure, of which the shutter is open for the share 1; each of the
//                                                  S x S samples has its own time (rt_render_motion)
//   rt_render --config c2 --samples 4 --coarse 2 --refine 8 [--aperture 8 [--focus 0.8]] [--light-size 40]
//             [--shutter 1 --move 0:40,0,0 ...] --out c2_lens_ad.ppm
//                                                  the frame of the three modes above with 2 x 2 samples per pixel, and
//                                                  4 x 4 only where the 2 x 2 samples' RGBA8 bytes spread by more than 8
//                                                  or the coarse RGBA8 differs from a 4-neighbour by more than 8
//                                                  (rt_render_lens_adaptive; threshold in -1 .. 255)
//   rt_render --config c2 --samples 4 --jitter 16 [--seed 7] [--aperture 8 [--focus 0.8]] [--light-size 40]
//             [--shutter 1 --move 0:40,0,0 ...] --out c2_jitter.ppm
//                                                  the frame of the lens, soft-shadow and motion modes with every sample
//                                                  at one of 16 hashed sub-positions of its stratum in each dimension
//                                                  (rt_render_jitter; J in 1, 2, 4, 8, 16; the seed defaults to 1)
//   rt_render --config c2 --samples 4 --shutter 1 --eye-move 0,40,0 [--look-move DX,DY,DZ] [--jitter 16 [--seed 7]]
//             [--move 0:40,0,0 ...] [--aperture 8 [--focus 0.8]] [--light-size 40] --out c2_shutter.ppm
//                                                  camera motion blur: the eye moves by +-(0, 40, 0) and the look-at
//                                                  point by +-(DX, DY, DZ) (world units) during the exposure; every sample
//                                                  sees from the camera of its own time (rt_render_shutter; J defaults to 1)
//   rt_render --config c2 --samples 2 --jitter 16 [--seed 7] --passes 64 [--shutter 1 [--eye-move 0,40,0] ...]
//             [--aperture 8] [--light-size 40] --out c2_accum.ppm
//                                                  64 jittered passes with the seeds 7 .. 70 summed in the kernel; the
//                                                  image is their mean (rt_render_accum; K in 1 .. 65536)
//   ... --passes 64 --tolerance 0.004 [--min-passes 4]
//                                                  64 is a budget: a pixel stops receiving passes once it has 4 and the
//                                                  standard error of its mean is at most 0.004 in every channel
//                                                  (rt_render_converge; M in 2 .. 2^31, default 4)
//   ... --passes 64 [--tolerance 0.004] --window X,Y,W,H
//                                                  only the W x H rectangle at (X, Y) of the frame (Y = 0: the bottom row),
//                                                  with the full frame's bytes; the PPM is W x H
//                                                  (rt_render_accum_window / rt_render_converge_window)
//   ... --passes 64 [--tolerance 0.004] --windows X,Y,W,H:X,Y,W,H:...
//                                                  the listed disjoint rectangles of the frame in one launch per launch
//                                                  group, in place; the PPM is the full frame, black outside the windows
//                                                  (rt_render_accum_windows / rt_render_converge_windows)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/rt_api.h"

namespace {

struct Options {
    std::string config = "c2";
    std::string out = "frame.ppm";
    bool from_stdin = false;
    int width = 0, height = 0, depth = -1, device = 0;
    double pitch = 0;
    int faithful = -1;                       // RT_RAND_GLIBC / RT_RAND_MSVC: rt_render_screen
    unsigned seed = 1;
    int gpus = 0;                            // > 0: rt_group over this many ranks (rt_render_multi)
    int band = 0;                            // band height (0: auto)
    int repeat = 1;                          // frames rendered (the last one is written)
    int samples = 0;                         // > 0: rt_render_ss with this many samples per axis (plain frames only)
    bool adaptive = false;                   // --adaptive T: rt_render_adaptive with threshold T (needs --samples)
    int threshold = 0;
    bool dof = false;                        // --aperture A: rt_render_dof with lens half-width A (needs --samples)
    double aperture = 0.0;
    bool focus = false;                      // --focus RATIO: rt_camera_focus before a --aperture render
    double focus_ratio = 1.0;
    bool soft = false;                       // --light-size R: rt_render_soft with panel half-width R (needs --samples)
    double light_size = 0.0;
    bool motion = false;                     // --shutter F: rt_render_motion with the --move displacements (needs --samples)
    double shutter = 0.0;
    int coarse = 0;                          // --coarse C with --refine T: rt_render_lens_adaptive, C x C samples per pixel
    bool refine = false;                     // ... and --samples x --samples where they disagree by more than T
    int refine_t = 0;
    int jitter = 0;                          // --jitter J: rt_render_jitter with --seed (needs --samples)
    bool camera_motion = false;              // --eye-move / --look-move DX,DY,DZ: rt_render_shutter (needs --shutter)
    rt_camera_motion camera_move = {};
    int passes = 0;                          // --passes K: rt_render_accum, K passes from --seed on (needs --jitter)
    bool converge = false;                   // --tolerance E: rt_render_converge with the budget --passes (needs it)
    double tolerance = 0.0;
    long long min_passes = 0;                // --min-passes M (needs --tolerance; default 4)
    bool window = false;                     // --window X,Y,W,H: that rectangle of the frame alone (needs --passes)
    rt_window win{};
    std::vector<rt_window> windows;         // --windows X,Y,W,H:...: those rectangles in one launch (needs --passes)
    std::vector<int> move_k;                // --move K:DX,DY,DZ (repeatable): sphere K's displacement
    std::vector<double> move_d;
};

// A finite number that fills the whole argument, or a usage error.
double number_arg(const std::string& flag, const std::string& v) {
    char* end = nullptr;
    const double x = std::strtod(v.c_str(), &end);
    if (v.empty() || *end != 0 || !std::isfinite(x)) {
        std::fprintf(stderr, "rt_render: %s needs a number, got '%s'\n", flag.c_str(), v.c_str());
        std::exit(2);
    }
    return x;
}

// --move K:DX,DY,DZ: a sphere index and three finite numbers, or a usage error.
void move_arg(const std::string& v, Options* o) {
    int k = -1, used = 0;
    double d[3];
    if (std::sscanf(v.c_str(), "%d:%lf,%lf,%lf%n", &k, &d[0], &d[1], &d[2], &used) != 4 || used != (int)v.size() ||
        k < 0 || !std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) {
        std::fprintf(stderr, "rt_render: --move needs K:DX,DY,DZ (a sphere index and three numbers), got '%s'\n",
                     v.c_str());
        std::exit(2);
    }
    o->move_k.push_back(k);
    o->move_d.insert(o->move_d.end(), d, d + 3);
}

// --eye-move / --look-move DX,DY,DZ: three finite numbers, or a usage error.
void camera_move_arg(const std::string& flag, const std::string& v, double out[3]) {
    int used = 0;
    double d[3];
    if (std::sscanf(v.c_str(), "%lf,%lf,%lf%n", &d[0], &d[1], &d[2], &used) != 3 || used != (int)v.size() ||
        !std::isfinite(d[0]) || !std::isfinite(d[1]) || !std::isfinite(d[2])) {
        std::fprintf(stderr, "rt_render: %s needs DX,DY,DZ (three numbers), got '%s'\n", flag.c_str(), v.c_str());
        std::exit(2);
    }
    std::copy(d, d + 3, out);
}

[[noreturn]] void die(const std::string& what, int code) {
    std::fprintf(stderr, "rt_render: %s failed (%d): %s\n", what.c_str(), code, rt_last_error());
    std::exit(1);
}

void check(int code, const char* what) {
    if (code != RT_OK) die(what, code);
}

// initScene2 (:1430-1493): "(a) light, (b) tetrahedron, (c) cube, (d) sphere, (e) cylinder, (f) cone",
// then a square "a1-h8", then "yes/no" for another object.  Returns the boardMap entries in input order.
void read_dialogue(std::vector<std::string>* squares, std::vector<int32_t>* types) {
    std::string tmp;
    bool finished = false;
    while (!finished) {
        bool answered = false;
        while (!answered) {
            std::cout << "Please select the type of object to add:\n"
                      << "(a) light, (b) tetrahedron, (c) cube, (d) sphere, (e) cylinder, (f) cone" << std::endl;
            if (!(std::cin >> tmp)) return;
            answered = tmp.size() <= 1;
            int type = tmp[0] - 'a';
            if (type >= 0 && type < 6) {
                std::cout << "Please enter the position: (a1-h8)" << std::endl;
                if (!(std::cin >> tmp)) return;
                squares->push_back(tmp);
                types->push_back(type);
            } else {
                answered = false;
            }
        }
        answered = false;
        while (!answered) {
            std::cout << "Would you like to add another object? (yes/no)" << std::endl;
            if (!(std::cin >> tmp)) return;
            if (tmp == "no" || tmp == "n") finished = answered = true;
            else if (tmp == "yes" || tmp == "y") answered = true;
        }
    }
}

struct Canonical {
    int w, h, nsph, nl, depth;
};

Canonical canonical(const std::string& c) {
    if (c == "c1") return {640, 480, 3, 1, 0};
    if (c == "c2") return {1920, 1080, 8, 1, 1};
    if (c == "c3" || c == "c4") return {3840, 2160, 8, 2, 2};
    if (c == "c5") return {7680, 4320, 64, 2, 3};
    std::fprintf(stderr, "rt_render: unknown config %s\n", c.c_str());
    std::exit(2);
}

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        std::fprintf(stderr, "rt_render: %s failed: %s\n", what, hipGetErrorString(e));
        std::exit(1);
    }
}

// --gpus N: one context per rank on device q % (devices), one rt_group, rt_render_multi into an RGBA8 image
// on rank 0's device (draw()'s frame, MySdlApplication.cpp:1541-1563, with its rows split over the GPUs).
int render_multi(const Options& o, const rt_scene& scene, const rt_camera& cam, int W, int H, int depth) {
    int ndev = 0;
    check(rt_device_count(&ndev), "rt_device_count");
    std::vector<rt_ctx*> ctxs(o.gpus, nullptr);
    for (int q = 0; q < o.gpus; ++q) {
        check(rt_ctx_create(q % ndev, &ctxs[q]), "rt_ctx_create");
        check(rt_set_scene(ctxs[q], &scene), "rt_set_scene");
    }
    rt_group* g = nullptr;
    check(rt_group_create(ctxs.data(), o.gpus, RT_TRANSPORT_AUTO, &g), "rt_group_create");
    int transport = 0, band = 0, slab = 0;
    check(rt_group_info(g, nullptr, nullptr, nullptr, &transport), "rt_group_info");
    check(rt_band_plan(H, o.gpus, o.band, &band, &slab), "rt_band_plan");
    hip_check(hipSetDevice(0), "hipSetDevice");
    uint8_t* d8 = nullptr;
    hip_check(hipMalloc(&d8, (size_t)W * H * 4), "hipMalloc");
    hipStream_t st = nullptr;
    hip_check(hipStreamCreate(&st), "hipStreamCreate");
    check(rt_render_multi(g, &cam, W, H, depth, o.band, RT_OUT_RGBA8, nullptr, d8, st), "rt_render_multi");
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");                  // first frame (setup)
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < o.repeat; ++k)
        check(rt_render_multi(g, &cam, W, H, depth, o.band, RT_OUT_RGBA8, nullptr, d8, st), "rt_render_multi");
    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / o.repeat;
    std::vector<uint8_t> rgba8((size_t)W * H * 4);
    hip_check(hipMemcpy(rgba8.data(), d8, rgba8.size(), hipMemcpyDeviceToHost), "hipMemcpy");
    check(rt_write_ppm(o.out.c_str(), rgba8.data(), W, H, 4), "rt_write_ppm");
    std::printf("rt_render: %dx%d depth %d over %d ranks (%d device(s), band %d rows, %s gather to rank 0) -> %s | "
                "%.3f ms per frame over %d frame(s)\n", W, H, depth, o.gpus, std::min(ndev, o.gpus), band,
                transport == RT_TRANSPORT_RCCL ? "RCCL" : "device-copy", o.out.c_str(), ms, o.repeat);
    rt_group_destroy(g);
    (void)hipFree(d8);
    (void)hipStreamDestroy(st);
    for (auto* c : ctxs) rt_ctx_destroy(c);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto next = [&]() -> std::string {
            if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); }
            return argv[++i];
        };
        if (a == "--config") o.config = next();
        else if (a == "--out") o.out = next();
        else if (a == "--stdin") o.from_stdin = true;
        else if (a == "--width") o.width = std::atoi(next().c_str());
        else if (a == "--height") o.height = std::atoi(next().c_str());
        else if (a == "--depth") o.depth = std::atoi(next().c_str());
        else if (a == "--pitch") o.pitch = std::atof(next().c_str());
        else if (a == "--device") o.device = std::atoi(next().c_str());
        else if (a == "--faithful") o.faithful = next() == "msvc" ? RT_RAND_MSVC : RT_RAND_GLIBC;
        else if (a == "--seed") o.seed = (unsigned)std::strtoul(next().c_str(), nullptr, 10);
        else if (a == "--gpus") o.gpus = std::atoi(next().c_str());
        else if (a == "--band") o.band = std::atoi(next().c_str());
        else if (a == "--repeat") o.repeat = std::max(1, std::atoi(next().c_str()));
        else if (a == "--samples") o.samples = std::atoi(next().c_str());
        else if (a == "--adaptive") { o.adaptive = true; o.threshold = std::atoi(next().c_str()); }
        else if (a == "--aperture") { o.dof = true; o.aperture = number_arg(a, next()); }
        else if (a == "--focus") { o.focus = true; o.focus_ratio = number_arg(a, next()); }
        else if (a == "--light-size") { o.soft = true; o.light_size = number_arg(a, next()); }
        else if (a == "--shutter") { o.motion = true; o.shutter = number_arg(a, next()); }
        else if (a == "--move") move_arg(next(), &o);
        else if (a == "--eye-move") { o.camera_motion = true; camera_move_arg(a, next(), o.camera_move.eye); }
        else if (a == "--look-move") { o.camera_motion = true; camera_move_arg(a, next(), o.camera_move.look_at); }
        else if (a == "--coarse") o.coarse = std::atoi(next().c_str());
        else if (a == "--refine") { o.refine = true; o.refine_t = std::atoi(next().c_str()); }
        else if (a == "--jitter") { o.jitter = std::atoi(next().c_str()); if (o.jitter == 0) o.jitter = -1; }
        else if (a == "--passes") { o.passes = std::atoi(next().c_str()); if (o.passes == 0) o.passes = -1; }
        else if (a == "--tolerance") { o.converge = true; o.tolerance = number_arg(a, next()); }
        else if (a == "--window") {
            const std::string v = next();
            long long q[4];
            char tail = 0;
            if (std::sscanf(v.c_str(), "%lld,%lld,%lld,%lld%c", &q[0], &q[1], &q[2], &q[3], &tail) != 4 ||
                v.find_first_not_of("0123456789,-") != std::string::npos) {
                std::fprintf(stderr, "rt_render: --window takes X,Y,W,H (four integers)\n");
                return 2;
            }
            for (long long t : q)
                if (t < INT32_MIN || t > INT32_MAX) {
                    std::fprintf(stderr, "rt_render: --window takes X,Y,W,H (four integers)\n");
                    return 2;
                }
            o.window = true;
            o.win = rt_window{(int32_t)q[0], (int32_t)q[1], (int32_t)q[2], (int32_t)q[3], (int32_t)q[2]};
        }
        else if (a == "--windows") {
            const std::string v = next();
            bool ok = !v.empty() && v.find_first_not_of("0123456789,-:") == std::string::npos;
            for (size_t at = 0; ok && at <= v.size();) {
                const size_t end = std::min(v.find(':', at), v.size());
                const std::string item = v.substr(at, end - at);
                long long q[4] = {0, 0, 0, 0};
                char tail = 0;
                ok = std::sscanf(item.c_str(), "%lld,%lld,%lld,%lld%c", &q[0], &q[1], &q[2], &q[3], &tail) == 4;
                for (long long t : q) ok = ok && t >= INT32_MIN && t <= INT32_MAX;
                if (ok) o.windows.push_back(rt_window{(int32_t)q[0], (int32_t)q[1], (int32_t)q[2], (int32_t)q[3], 0});
                at = end + 1;
            }
            if (!ok) {
                std::fprintf(stderr, "rt_render: --windows takes X,Y,W,H:X,Y,W,H:... (four integers per window)\n");
                return 2;
            }
        }
        else if (a == "--min-passes") { o.min_passes = std::atoll(next().c_str()); if (o.min_passes == 0) o.min_passes = -1; }
        else { std::fprintf(stderr, "usage: rt_render [--config c1|c2|c3|c5|demo | --stdin] [--width W --height H "
                                    "--pitch P --depth B] [--device N] [--faithful glibc|msvc [--seed S]] "
                                    "[--gpus N [--band H]] [--samples 1|2|4|8 [--adaptive T | [--light-size R] "
                                    "[--aperture A [--focus RATIO]] [--shutter F [--move K:DX,DY,DZ]...] [--coarse C --refine T | --jitter J [--seed K] [--passes K [--tolerance E [--min-passes M]] [--window X,Y,W,H | --windows X,Y,W,H:...]]] "
                                    "[--eye-move DX,DY,DZ] [--look-move DX,DY,DZ]]] "
                                    "[--repeat K] [--out file.ppm]\n");
               return 2; }
    }
    if (o.camera_motion && (!o.motion || o.samples == 0 || o.adaptive || o.refine || o.coarse != 0 || o.faithful >= 0 ||
                            o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --eye-move and --look-move need --shutter and --samples, exclude --adaptive, "
                             "--coarse and --refine and apply to plain frames (not --faithful or --gpus)\n");
        return 2;
    }
    if (o.adaptive && (o.samples == 0 || o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --adaptive needs --samples and applies to plain frames (not --faithful or "
                             "--gpus)\n");
        return 2;
    }
    if (o.dof && (o.samples == 0 || o.adaptive || o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --aperture needs --samples, excludes --adaptive and applies to plain frames "
                             "(not --faithful or --gpus)\n");
        return 2;
    }
    if (o.dof && o.aperture < 0.0) {
        std::fprintf(stderr, "rt_render: --aperture must be >= 0\n");
        return 2;
    }
    if (o.soft && (o.samples == 0 || o.adaptive || o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --light-size needs --samples, excludes --adaptive and applies to plain frames "
                             "(not --faithful or --gpus)\n");
        return 2;
    }
    if (o.soft && o.light_size < 0.0) {
        std::fprintf(stderr, "rt_render: --light-size must be >= 0\n");
        return 2;
    }
    if (o.motion && (o.samples == 0 || o.adaptive || o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --shutter needs --samples, excludes --adaptive and applies to plain frames "
                             "(not --faithful or --gpus)\n");
        return 2;
    }
    if (o.motion && !(o.shutter >= 0.0 && o.shutter <= 1.0)) {
        std::fprintf(stderr, "rt_render: --shutter must be in [0, 1]\n");
        return 2;
    }
    if (!o.motion && !o.move_k.empty()) {
        std::fprintf(stderr, "rt_render: --move needs --shutter\n");
        return 2;
    }
    if (o.focus && (!o.dof || !(o.focus_ratio > 0.0))) {
        std::fprintf(stderr, "rt_render: --focus needs --aperture and a ratio > 0\n");
        return 2;
    }
    if (o.jitter != 0 && (o.samples == 0 || o.adaptive || o.refine || o.coarse != 0 || o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --jitter needs --samples, excludes --adaptive, --coarse and --refine and applies "
                             "to plain frames (not --faithful or --gpus)\n");
        return 2;
    }
    if (o.jitter != 0 && o.jitter != 1 && o.jitter != 2 && o.jitter != 4 && o.jitter != 8 && o.jitter != 16) {
        std::fprintf(stderr, "rt_render: --jitter must be 1, 2, 4, 8 or 16\n");
        return 2;
    }
    if (o.passes != 0 && o.jitter == 0) {
        std::fprintf(stderr, "rt_render: --passes needs --jitter\n");
        return 2;
    }
    if (o.passes != 0 && (o.passes < 1 || o.passes > 65536)) {
        std::fprintf(stderr, "rt_render: --passes must lie in 1 .. 65536\n");
        return 2;
    }
    if (o.converge && o.passes == 0) {
        std::fprintf(stderr, "rt_render: --tolerance needs --passes\n");
        return 2;
    }
    if (o.converge && !(o.tolerance >= 0.0)) {
        std::fprintf(stderr, "rt_render: --tolerance must be >= 0\n");
        return 2;
    }
    if (o.min_passes != 0 && !o.converge) {
        std::fprintf(stderr, "rt_render: --min-passes needs --tolerance\n");
        return 2;
    }
    if (o.min_passes != 0 && (o.min_passes < 2 || o.min_passes > (1ll << 31))) {
        std::fprintf(stderr, "rt_render: --min-passes must lie in 2 .. 2147483648\n");
        return 2;
    }
    if (o.window && o.passes == 0) {
        std::fprintf(stderr, "rt_render: --window needs --passes\n");
        return 2;
    }
    if (!o.windows.empty() && (o.passes == 0 || o.window)) {
        std::fprintf(stderr, "rt_render: --windows needs --passes and excludes --window\n");
        return 2;
    }
    if ((o.coarse != 0) != o.refine) {
        std::fprintf(stderr, "rt_render: --coarse and --refine need each other\n");
        return 2;
    }
    if (o.refine && o.samples == 0) {
        std::fprintf(stderr, "rt_render: --coarse and --refine need --samples\n");
        return 2;
    }
    if (o.refine && o.adaptive) {
        std::fprintf(stderr, "rt_render: --coarse and --refine exclude --adaptive\n");
        return 2;
    }
    if (o.refine && o.faithful >= 0) {
        std::fprintf(stderr, "rt_render: --coarse and --refine exclude --faithful\n");
        return 2;
    }
    if (o.refine && o.gpus > 0) {
        std::fprintf(stderr, "rt_render: --coarse and --refine exclude --gpus\n");
        return 2;
    }
    if (o.refine && o.coarse > o.samples) {
        std::fprintf(stderr, "rt_render: --coarse must not exceed --samples\n");
        return 2;
    }
    if (o.samples != 0 && (o.faithful >= 0 || o.gpus > 0)) {
        std::fprintf(stderr, "rt_render: --samples applies to plain frames (not --faithful or --gpus)\n");
        return 2;
    }

    rt_scene scene;
    std::vector<rt_sphere> spheres(RT_MAX_SPHERES);
    std::vector<rt_mesh> meshes(RT_MAX_MESHES);
    std::vector<rt_light> lights(2);
    int W, H, depth;
    double pitch;
    if (o.from_stdin) {
        std::vector<std::string> sq;
        std::vector<int32_t> ty;
        read_dialogue(&sq, &ty);
        std::vector<const char*> csq;
        for (auto& s : sq) csq.push_back(s.c_str());
        check(rt_load_scene(csq.data(), ty.data(), (int)csq.size(), &scene, spheres.data(), RT_MAX_SPHERES,
                            meshes.data(), RT_MAX_MESHES, &lights[0]),
              "rt_load_scene");
        W = o.width > 0 ? o.width : 500;                    // g_windowWidth/Height (:570)
        H = o.height > 0 ? o.height : 500;
        depth = o.depth >= 0 ? o.depth : 5;                 // MAX_DEPTH (:48)
        pitch = o.pitch > 0 ? o.pitch : 1.0;                // rayTraceScreen's unit pixel step
    } else if (o.config == "demo") {
        // initScene (MySdlApplication.cpp:1387-1428): light b6, tetrahedron b4, sphere d7 (r 20),
        // cube a7, inserted in that order after the board; the app's 500x500 window, MAX_DEPTH 5.
        check(rt_scene_init_reference(&scene), "rt_scene_init_reference");
        check(rt_convert_string_coordinate("d7", spheres[0].center), "rt_convert_string_coordinate");
        spheres[0].radius = 20.0;
        meshes[0] = rt_mesh{RT_MESH_TETRAHEDRON, 0, {0, 0, 0}, 40.0};
        meshes[1] = rt_mesh{RT_MESH_CUBE, 1, {0, 0, 0}, 40.0};
        check(rt_convert_string_coordinate("b4", meshes[0].position), "rt_convert_string_coordinate");
        check(rt_convert_string_coordinate("a7", meshes[1].position), "rt_convert_string_coordinate");
        check(rt_light_position_from_square("b6", lights[0].position), "rt_light_position_from_square");
        for (int q = 0; q < 3; ++q) lights[0].color[q] = 1.0;
        scene.n_spheres = 1;
        scene.spheres = spheres.data();
        scene.n_meshes = 2;
        scene.meshes = meshes.data();
        scene.n_lights = 1;
        scene.lights = lights.data();
        W = o.width > 0 ? o.width : 500;
        H = o.height > 0 ? o.height : 500;
        depth = o.depth >= 0 ? o.depth : 5;
        pitch = o.pitch > 0 ? o.pitch : 1.0;
    } else {
        Canonical c = canonical(o.config);
        check(rt_scene_init_reference(&scene), "rt_scene_init_reference");
        static const char* kSq[8] = {"d7", "b2", "f5", "h8", "c4", "e2", "g6", "a5"};
        int n = 0;
        if (c.nsph == 64) {
            for (int r = 0; r < 8; ++r)
                for (int cc = 0; cc < 8; ++cc) {
                    char s[3] = {(char)('a' + r), (char)('1' + cc), 0};
                    check(rt_convert_string_coordinate(s, spheres[n].center), "rt_convert_string_coordinate");
                    spheres[n].center[0] += 0.0;
                    spheres[n].center[1] += (double)(((r + cc) % 3) * 25);
                    spheres[n].center[2] += 0.0;
                    spheres[n].radius = 10.0;
                    ++n;
                }
        } else {
            for (; n < c.nsph; ++n) {
                check(rt_convert_string_coordinate(kSq[n], spheres[n].center), "rt_convert_string_coordinate");
                spheres[n].radius = 20.0;
            }
        }
        const char* lsq[2] = {"b6", "g3"};
        const double lcol[2] = {1.0, 0.5};
        for (int k = 0; k < c.nl; ++k) {
            check(rt_light_position_from_square(lsq[k], lights[k].position), "rt_light_position_from_square");
            for (int q = 0; q < 3; ++q) lights[k].color[q] = lcol[k];
        }
        scene.n_spheres = n;
        scene.spheres = spheres.data();
        scene.n_lights = c.nl;
        scene.lights = lights.data();
        W = o.width > 0 ? o.width : c.w;
        H = o.height > 0 ? o.height : c.h;
        depth = o.depth >= 0 ? o.depth : c.depth;
        pitch = o.pitch > 0 ? o.pitch : 500.0 / W;          // canonical framing
    }

    std::vector<double> displacement((size_t)3 * (size_t)std::max(scene.n_spheres, 1), 0.0);
    for (size_t m = 0; m < o.move_k.size(); ++m) {
        if (o.move_k[m] >= scene.n_spheres) {
            std::fprintf(stderr, "rt_render: --move %d: the scene has %d spheres\n", o.move_k[m], scene.n_spheres);
            return 2;
        }
        for (int q = 0; q < 3; ++q) displacement[3 * (size_t)o.move_k[m] + q] = o.move_d[3 * m + q];
    }

    if (o.window && (o.win.x0 < 0 || o.win.y0 < 0 || o.win.width < 1 || o.win.height < 1 ||
                     (long long)o.win.x0 + o.win.width > W || (long long)o.win.y0 + o.win.height > H)) {
        std::fprintf(stderr, "rt_render: --window %d,%d,%d,%d is empty or leaves the %d x %d frame\n", o.win.x0, o.win.y0,
                     o.win.width, o.win.height, W, H);
        return 2;
    }
    // the buffers of a window are dense: OW x OH is the image written
    const int OW = o.window ? o.win.width : W, OH = o.window ? o.win.height : H;
    rt_camera cam;
    check(rt_camera_init_reference(&cam, W, H, pitch), "rt_camera_init_reference");
    if (o.focus) check(rt_camera_focus(&cam, o.focus_ratio, &cam), "rt_camera_focus");
    rt_ctx* ctx = nullptr;
    check(rt_ctx_create(o.device, &ctx), "rt_ctx_create");
    std::vector<uint8_t> rgba8((size_t)W * H * 4);
    std::vector<double> accum(o.passes != 0 ? (size_t)W * H * 3 : 0);
    std::vector<double> accum2(o.converge ? (size_t)W * H * 3 : 0);
    std::vector<uint32_t> count(o.converge ? (size_t)W * H : 0);
    const uint32_t min_passes = o.min_passes != 0 ? (uint32_t)o.min_passes : 4u;
    uint64_t n_active = 0;
    if (o.faithful >= 0) {
        uint64_t calls = 0;
        std::vector<uint8_t> ns((size_t)W * H);
        check(rt_render_screen(ctx, &scene, &cam, W, H, depth, o.faithful, o.seed, nullptr, rgba8.data(), ns.data(),
                               &calls), "rt_render_screen");
        check(rt_write_ppm(o.out.c_str(), rgba8.data(), W, H, 4), "rt_write_ppm");
        unsigned long long samples = 0;
        for (uint8_t v : ns) samples += v;
        std::printf("rt_render: %dx%d depth %d faithful rayTraceScreen (%s rand, seed %u) -> %s | %llu samples, "
                    "%llu rand() calls\n", W, H, depth, o.faithful == RT_RAND_MSVC ? "msvc" : "glibc", o.seed,
                    o.out.c_str(), samples, (unsigned long long)calls);
        rt_ctx_destroy(ctx);
        return 0;
    }
    if (o.gpus > 0) {
        rt_ctx_destroy(ctx);
        return render_multi(o, scene, cam, W, H, depth);
    }
    rt_stats st;
    uint64_t n_refined = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < o.repeat; ++k) {
        if (o.refine)
            check(rt_render_lens_adaptive(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam, W, H, depth,
                                          o.coarse, o.samples, o.refine_t, o.aperture, o.light_size, o.shutter, nullptr,
                                          rgba8.data(), nullptr, nullptr, &st, &n_refined), "rt_render_lens_adaptive");
        else if (!o.windows.empty()) {
            // in place: the arrays are the full frame's, zero (black) outside the windows
            std::fill(count.begin(), count.end(), 0u);      // every repeat is a new sum
            const int nw = (int)o.windows.size();
            if (o.converge)
                check(rt_render_converge_windows(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                                 o.camera_motion ? &o.camera_move : nullptr, W, H, depth, o.samples,
                                                 o.jitter, (uint32_t)o.seed, o.passes, min_passes, o.tolerance,
                                                 o.aperture, o.light_size, o.shutter, accum.data(), accum2.data(),
                                                 count.data(), nullptr, rgba8.data(), nullptr, &st, &n_active,
                                                 o.windows.data(), nw, RT_WINDOWS_IN_PLACE),
                      "rt_render_converge_windows");
            else
                check(rt_render_accum_windows(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                              o.camera_motion ? &o.camera_move : nullptr, W, H, depth, o.samples,
                                              o.jitter, (uint32_t)o.seed, 0u, o.passes, o.aperture, o.light_size,
                                              o.shutter, accum.data(), nullptr, rgba8.data(), nullptr, &st,
                                              o.windows.data(), nw, RT_WINDOWS_IN_PLACE),
                      "rt_render_accum_windows");
        } else if (o.converge && o.window) {
            std::fill(count.begin(), count.end(), 0u);      // every repeat is a new sum
            check(rt_render_converge_window(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                            o.camera_motion ? &o.camera_move : nullptr, W, H, &o.win, depth, o.samples,
                                            o.jitter, (uint32_t)o.seed, o.passes, min_passes, o.tolerance, o.aperture,
                                            o.light_size, o.shutter, accum.data(), accum2.data(), count.data(), nullptr,
                                            rgba8.data(), nullptr, &st, &n_active), "rt_render_converge_window");
        } else if (o.window)
            check(rt_render_accum_window(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                         o.camera_motion ? &o.camera_move : nullptr, W, H, &o.win, depth, o.samples,
                                         o.jitter, (uint32_t)o.seed, 0u, o.passes, o.aperture, o.light_size, o.shutter,
                                         accum.data(), nullptr, rgba8.data(), nullptr, &st), "rt_render_accum_window");
        else if (o.converge) {
            std::fill(count.begin(), count.end(), 0u);      // every repeat is a new sum
            check(rt_render_converge(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                     o.camera_motion ? &o.camera_move : nullptr, W, H, depth, o.samples, o.jitter,
                                     (uint32_t)o.seed, o.passes, min_passes, o.tolerance, o.aperture, o.light_size,
                                     o.shutter, accum.data(), accum2.data(), count.data(), nullptr, rgba8.data(), nullptr,
                                     &st, &n_active), "rt_render_converge");
        } else if (o.passes != 0)
            check(rt_render_accum(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam,
                                  o.camera_motion ? &o.camera_move : nullptr, W, H, depth, o.samples, o.jitter,
                                  (uint32_t)o.seed, 0u, o.passes, o.aperture, o.light_size, o.shutter, accum.data(),
                                  nullptr, rgba8.data(), nullptr, &st), "rt_render_accum");
        else if (o.camera_motion)
            check(rt_render_shutter(ctx, &scene, displacement.data(), &cam, &o.camera_move, W, H, depth, o.samples,
                                    o.jitter != 0 ? o.jitter : 1, (uint32_t)o.seed, o.aperture, o.light_size, o.shutter,
                                    nullptr, rgba8.data(), nullptr, &st), "rt_render_shutter");
        else if (o.jitter != 0)
            check(rt_render_jitter(ctx, &scene, o.motion ? displacement.data() : nullptr, &cam, W, H, depth, o.samples,
                                   o.jitter, (uint32_t)o.seed, o.aperture, o.light_size, o.shutter, nullptr, rgba8.data(),
                                   nullptr, &st), "rt_render_jitter");
        else if (o.motion)
            check(rt_render_motion(ctx, &scene, displacement.data(), &cam, W, H, depth, o.samples, o.aperture,
                                   o.light_size, o.shutter, nullptr, rgba8.data(), nullptr, &st), "rt_render_motion");
        else if (o.soft)
            check(rt_render_soft(ctx, &scene, &cam, W, H, depth, o.samples, o.aperture, o.light_size, nullptr,
                                 rgba8.data(), nullptr, &st), "rt_render_soft");
        else if (o.dof)
            check(rt_render_dof(ctx, &scene, &cam, W, H, depth, o.samples, o.aperture, nullptr, rgba8.data(), nullptr,
                                &st), "rt_render_dof");
        else if (o.adaptive)
            check(rt_render_adaptive(ctx, &scene, &cam, W, H, depth, o.samples, o.threshold, nullptr, rgba8.data(),
                                     nullptr, nullptr, &st, &n_refined), "rt_render_adaptive");
        else if (o.samples != 0)
            check(rt_render_ss(ctx, &scene, &cam, W, H, depth, o.samples, nullptr, rgba8.data(), nullptr, &st),
                  "rt_render_ss");
        else
            check(rt_render(ctx, &scene, &cam, W, H, depth, nullptr, nullptr, rgba8.data(), nullptr, &st), "rt_render");
    }
    const double per_call_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() /
                               o.repeat;
    check(rt_write_ppm(o.out.c_str(), rgba8.data(), OW, OH, 4), "rt_write_ppm");
    if (o.window)
        std::printf("rt_render: window %d,%d,%d,%d of the %d x %d frame\n", o.win.x0, o.win.y0, OW, OH, W, H);
    unsigned long long list_px = 0;
    for (const rt_window& w : o.windows) list_px += (unsigned long long)w.width * (unsigned long long)w.height;
    if (!o.windows.empty())
        std::printf("rt_render: %zu windows, %llu pixels of the %d x %d frame, in place\n", o.windows.size(), list_px, W, H);
    const unsigned long long out_px = o.windows.empty() ? (unsigned long long)OW * OH : list_px;
    const uint64_t rays = st.primary_rays + st.reflect_rays + st.shadow_rays;
    std::printf("rt_render: %dx%d depth %d -> %s | rays %llu (primary %llu, reflect %llu, shadow %llu) | kernel %.3f ms"
                " | %.1f Mray/s\n",
                W, H, depth, o.out.c_str(), (unsigned long long)rays, (unsigned long long)st.primary_rays,
                (unsigned long long)st.reflect_rays, (unsigned long long)st.shadow_rays, st.kernel_ms,
                rays / (st.kernel_ms * 1e3));
    if (o.converge) {
        unsigned long long traced = 0;
        for (size_t k = 0; k < (size_t)OW * OH; ++k) traced += count[k];
        std::printf("rt_render: converged, a budget of %d passes from seed %u, tolerance %g, at least %u passes: %llu of "
                    "%llu pixels still active, %llu of %llu pixel-passes traced, %llu primary rays\n", o.passes, o.seed,
                    o.tolerance, min_passes, (unsigned long long)n_active, out_px, traced,
                    out_px * (unsigned long long)o.passes, (unsigned long long)st.primary_rays);
    } else if (o.passes != 0)
        std::printf("rt_render: accumulated, %d passes with the seeds %u .. %u: the mean of %d x %d x %d samples per "
                    "pixel, %llu primary rays\n", o.passes, o.seed, (unsigned)(o.seed + (unsigned)o.passes - 1u), o.passes,
                    o.samples, o.samples, (unsigned long long)st.primary_rays);
    if (o.refine)
        std::printf("rt_render: adaptive lens render, threshold %d, shutter %g, light half-width %g, lens half-width %g: "
                    "%llu of %llu pixels refined from %d x %d to %d x %d samples\n", o.refine_t, o.shutter, o.light_size,
                    o.aperture, (unsigned long long)n_refined, (unsigned long long)W * H, o.coarse, o.coarse, o.samples,
                    o.samples);
    else if (o.camera_motion)
        std::printf("rt_render: camera motion, eye +-(%g, %g, %g), look-at +-(%g, %g, %g), shutter %g, J = %d, seed %u, %d "
                    "moving spheres, light half-width %g, lens half-width %g: %d x %d samples per pixel, %llu primary "
                    "rays\n", o.camera_move.eye[0], o.camera_move.eye[1], o.camera_move.eye[2], o.camera_move.look_at[0],
                    o.camera_move.look_at[1], o.camera_move.look_at[2], o.shutter, o.jitter != 0 ? o.jitter : 1, o.seed,
                    (int)o.move_k.size(), o.light_size, o.aperture, o.samples, o.samples,
                    (unsigned long long)st.primary_rays);
    else if (o.jitter != 0)
        std::printf("rt_render: jittered, J = %d sub-positions per stratum and axis, seed %u, shutter %g, %d moving "
                    "spheres, light half-width %g, lens half-width %g: %d x %d samples per pixel, %llu primary rays\n",
                    o.jitter, o.seed, o.shutter, (int)o.move_k.size(), o.light_size, o.aperture, o.samples, o.samples,
                    (unsigned long long)st.primary_rays);
    else if (o.motion)
        std::printf("rt_render: motion blur, shutter %g, %d moving spheres, light half-width %g, lens half-width %g: "
                    "%d x %d shutter times per pixel, %llu primary rays\n", o.shutter, (int)o.move_k.size(),
                    o.light_size, o.aperture, o.samples, o.samples, (unsigned long long)st.primary_rays);
    else if (o.soft)
        std::printf("rt_render: soft shadows, light half-width %g, lens half-width %g: %d x %d light samples per "
                    "pixel, %llu primary rays\n", o.light_size, o.aperture, o.samples, o.samples,
                    (unsigned long long)st.primary_rays);
    else if (o.dof)
        std::printf("rt_render: depth of field, lens half-width %g, focus ratio %g: %d x %d lens samples per pixel\n",
                    o.aperture, o.focus_ratio, o.samples, o.samples);
    else if (o.adaptive)
        std::printf("rt_render: adaptive, threshold %d: %llu of %llu pixels refined with %d x %d samples\n", o.threshold,
                    (unsigned long long)n_refined, (unsigned long long)W * H, o.samples, o.samples);
    else if (o.samples != 0)
        std::printf("rt_render: %d x %d samples per pixel, summed in the kernel\n", o.samples, o.samples);
    if (o.repeat > 1) std::printf("rt_render: %d calls, %.3f ms per call (host to host)\n", o.repeat, per_call_ms);
    rt_ctx_destroy(ctx);
    return 0;
}
