// tile_class_test.cpp -- the tile classifier of crt_tile_class.h against brute force, on the CPU.  For hand-made quantised
// root nodes and a handful of cameras, every tile the classifier calls MISS must hold only rays whose root step misses,
// every ENTER tile none: checked with the header's scalar functions at the corners of every valid pixel's sample / jitter
// box and at seeded random (pixel, sample, jitter) points.  Built and run by tests/test_tile_class_cpu.py; calls no HIP function.
#include <cstdio>
#include <cstring>
#include <cmath>

#include "crt_tile_class.h"

using namespace crt;

static int g_failed = 0;
static long g_checked = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        g_checked++;                                                                   \
        if (!(cond)) { if (g_failed++ < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// camera_frame of crt_scene.cpp (eye, look-at, up, vertical field of view in radians)
static TcCam camera(f3 eye, f3 lookat, f3 up, float fov, uint32_t W, uint32_t H)
{
    const f3 w = normalize(eye - lookat), u = normalize(cross(up, w)), v = cross(w, u);
    const float vh = 2.0f * tan_(fov / 2.0f), vw = ((float)W / (float)H) * vh;
    const f3 hor = u * vw, ver = v * vh;
    const f3 llc = ((eye - hor / 2.0f) - ver / 2.0f) - w;
    return TcCam{llc, hor, ver, eye, (float)W, (float)H};
}
static TcCam standard(uint32_t W, uint32_t H) { return camera(f3{278, 273, -800}, f3{278, 273, 0}, f3{0, 1, 0}, 0.7f, W, H); }

// A quantised root node of n <= 4 boxes (lo.xyz, hi.xyz), the way crt_bvh.cpp quantises: planes widened by one step,
// an empty slot lo = 65535, hi = 0.
static TcRoot root_of(const float (*box)[6], int n, float base, float extent)
{
    TcRoot R{};
    const float scale = extent / 65535.0f;
    R.qbase = f3{base, base, base};
    R.qscale = f3{scale, scale, scale};
    for (uint32_t k = 0; k < 4u; k++)
        for (uint32_t a = 0; a < 3u; a++) {
            long ql = 65535, qh = 0;
            if ((int)k < n) {
                ql = (long)std::floor(((double)box[k][a] - base) / scale) - 1;
                qh = (long)std::ceil(((double)box[k][3 + a] - base) / scale) + 1;
                ql = ql < 0 ? 0 : ql; qh = qh > 65535 ? 65535 : qh;
            }
            R.q[2u * a + (k >> 1)] |= (uint32_t)ql << ((k & 1u) * 16u);
            R.q[6u + 2u * a + (k >> 1)] |= (uint32_t)qh << ((k & 1u) * 16u);
        }
    return R;
}

static uint32_t g_rng = 0x2545F491u;
static uint32_t rnd32() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

struct Census { uint32_t miss = 0, enter = 0, maybe = 0; };

static Census sweep(const char *name, const TcCam &C, const TcRoot &R, const TcTiles &T, uint32_t tiles_y)
{
    Census n;
    const float jend[2] = {0.0f, bits_f(0x3F7FFFFFu)};
    const uint32_t send[2] = {0u, kTcGrid - 1u};
    long evals = 0;
    for (uint32_t tile = 0; tile < T.tiles_x * tiles_y; tile++) {
        const uint32_t cls = tc_tile_class(C, R, T, tile);
        if (cls == kTcMiss) n.miss++; else if (cls == kTcEnter) n.enter++; else n.maybe++;
        if (cls == kTcMaybe) continue;
        uint32_t misses = 0, total = 0, valid[64], nvalid = 0;
        for (uint32_t l = 0; l < 64u; l++) {
            uint32_t px, py;
            if (!tc_pixel(T, tile, l, px, py)) continue;
            valid[nvalid++] = l;
            for (int s = 0; s < 2; s++) for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) {
                const f3 d = tc_camera_dir(C, px, py, send[s], jend[a], jend[b]);
                misses += tc_root_step_misses(R, C.eye, d) ? 1u : 0u; total++;
            }
        }
        CHECK(nvalid > 0u);                                          // (a tile without a valid pixel is MAYBE)
        for (int i = 0; i < 256 && nvalid; i++) {
            uint32_t px, py;
            tc_pixel(T, tile, valid[rnd32() % nvalid], px, py);
            const float jx = (float)(rnd32() >> 8) * 5.9604644775390625e-8f, jy = (float)(rnd32() >> 8) * 5.9604644775390625e-8f;
            const f3 d = tc_camera_dir(C, px, py, rnd32(), jx, jy);
            misses += tc_root_step_misses(R, C.eye, d) ? 1u : 0u; total++;
        }
        evals += total;
        if (cls == kTcMiss) CHECK(misses == total); else CHECK(misses == 0u);
    }
    std::printf("%-34s %4ux%-4u tiles %5u: MISS %5u ENTER %5u MAYBE %5u (%ld rays checked)\n", name, T.tw, T.th, T.tiles_x * tiles_y,
                n.miss, n.enter, n.maybe, evals);
    return n;
}

static TcTiles whole(uint32_t W, uint32_t H) { return TcTiles{0, 0, W, H, 0x40000000u, 1, 0, (W + 7u) / 8u}; }

int main()
{
    // four children inside [0, 555]^3; two children and two empty slots; one box filling the view
    const float four[4][6] = {{0, 0, 0, 277, 277, 555}, {278, 0, 0, 555, 277, 555}, {0, 278, 100, 277, 555, 555}, {278, 278, 0, 555, 548.8f, 559.2f}};
    const float two[2][6] = {{130, 0, 65, 295, 165, 230}, {265, 0, 247, 430, 330, 412}};
    const float wide[1][6] = {{-3000, -3000, 0, 3500, 3500, 555}};
    const TcRoot R4 = root_of(four, 4, -10.0f, 600.0f), R2 = root_of(two, 2, -10.0f, 600.0f), R1 = root_of(wide, 1, -3100.0f, 6700.0f);

    const uint32_t shapes[4][2] = {{100, 76}, {192, 108}, {480, 270}, {101, 77}};   // (odd: the central pixel's d.x, d.y intervals hold zero)
    for (const auto &s : shapes) {
        const uint32_t W = s[0], H = s[1];
        const TcCam C = standard(W, H);
        const TcTiles T = whole(W, H);
        const Census a = sweep("standard camera, four children", C, R4, T, (H + 7u) / 8u);
        CHECK(a.miss > 0u && a.enter > 0u);
        const Census b = sweep("standard camera, empty slots", C, R2, T, (H + 7u) / 8u);
        CHECK(b.miss > 0u && b.enter > 0u);
        const Census c = sweep("standard camera, box fills view", C, R1, T, (H + 7u) / 8u);
        CHECK(c.miss == 0u && c.enter > 0u);
    }
    {   // two ranks, bands of 8 rows: rank p holds rows y with (y / 8) % 2 == p
        const uint32_t W = 192, H = 108;
        const TcCam C = standard(W, H);
        for (uint32_t phase = 0; phase < 2u; phase++) {
            uint32_t rows = 0;
            for (uint32_t b = phase; b * 8u < H; b += 2u) rows += (H - b * 8u) < 8u ? H - b * 8u : 8u;
            const TcTiles T{0, 0, W, rows, 8, 2, phase, (W + 7u) / 8u};
            const Census a = sweep(phase ? "row bands, phase 1" : "row bands, phase 0", C, R4, T, (rows + 7u) / 8u);
            CHECK(a.miss > 0u && a.enter > 0u);
        }
        // a crop that is ragged on both sides
        const TcTiles T{37, 21, 83, 45, 0x40000000u, 1, 0, 11};
        sweep("crop 83x45 at (37, 21)", C, R4, T, 6);
    }
    {
        const uint32_t W = 192, H = 108;
        const TcTiles T = whole(W, H);
        const TcCam in = camera(f3{278, 273, 278}, f3{278, 273, 500}, f3{0, 1, 0}, 0.7f, W, H);
        const Census a = sweep("camera inside the box", in, R4, T, (H + 7u) / 8u);
        CHECK(a.miss == 0u);
        const TcCam away = camera(f3{278, 273, -800}, f3{278, 273, -1600}, f3{0, 1, 0}, 0.7f, W, H);
        const Census b = sweep("camera looking away", away, R4, T, (H + 7u) / 8u);
        CHECK(b.miss == T.tiles_x * ((H + 7u) / 8u) && b.enter == 0u && b.maybe == 0u);
        const TcCam skew = camera(f3{-300, 900, -500}, f3{278, 100, 278}, f3{0.1f, 1, 0.05f}, 0.9f, W, H);
        sweep("oblique camera", skew, R4, T, (H + 7u) / 8u);
        sweep("oblique camera, empty slots", skew, R2, T, (H + 7u) / 8u);
        // a camera that is not finite classifies nothing
        TcCam bad = standard(W, H);
        bad.eye.x = bits_f(0x7FC00000u);
        const Census c = sweep("NaN eye", bad, R4, T, (H + 7u) / 8u);
        CHECK(c.miss == 0u && c.enter == 0u);
    }
    {   // the culled value: +0 for a table of finite, not all negative entries; not for a negative or a non-finite one
        static float cie[3 * kTcNCie];
        for (uint32_t i = 0; i < 3 * kTcNCie; i++) cie[i] = 0.001f * (float)(i % 97u);
        CHECK(tc_culled_is_zero(cie));
        for (uint32_t i = 0; i < 3 * kTcNCie; i++) cie[i] = -1.0f;
        CHECK(!tc_culled_is_zero(cie));                            // (-0 in every channel)
        for (uint32_t i = 0; i < 3 * kTcNCie; i++) cie[i] = 1.0f;
        cie[kTcNCie + 100] = bits_f(0x7F800000u);
        CHECK(!tc_culled_is_zero(cie));
    }
    std::printf("%ld checked, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
