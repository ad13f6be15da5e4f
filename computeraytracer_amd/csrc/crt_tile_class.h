// crt_tile_class.h -- what a camera ray's root step can be for a whole 8x8 tile, decided once per run.
//
// k_wf_gen's CULL form draws every camera ray and takes the root step of the quantised 4-wide tree for it,
// to find out what is the same for every sample of most tiles: the tile's rays all miss the root's four child boxes, or
// all enter one.  Here that is decided per tile from the run's inputs alone (camera, frame size, tile rectangle and row
// mapping, the root node's words), by evaluating the SAME operations in the SAME order on intervals:
//   * every operation of the camera ray and of the root step (+, -, *, /, sqrt, fma, max, min, int -> float) is correctly
//     rounded and monotone in each argument, so it maps a box of inputs into the interval spanned by its values at the
//     corners of the box, computed in the same f32 round-to-nearest arithmetic;
//   * a variable that occurs twice is taken as two independent ones, which only widens the result;
//   * the one non-monotone step, the clamp and reciprocal of a direction component, is split at zero into a negative and a
//     positive part (below), on each of which it is monotone and the near / far plane choice is fixed.
// There is no epsilon and no geometric argument: a MISS tile holds only rays the per-sample test would cull, an ENTER tile
// none.  Host + device, one definition; nothing of the HIP runtime is called.
#pragma once
#include "crt_math.h"

namespace crt {

constexpr uint32_t kTcMaybe = 0, kTcMiss = 1, kTcEnter = 2;        // 2 bits per tile, 16 tiles per word of the table
constexpr uint32_t kTcGrid = 16;                                    // = kGrid (crt_shade.h: the stratum grid of the film jitter)
constexpr uint32_t kTcNLambda = 301, kTcNCie = 471;                 // = kNLambda, kNCie (crt_device.h)

struct TcCam { f3 llc, hor, ver, eye; float W, H; };               // DevScene::cam, (float)DevScene::W, (float)DevScene::H
struct TcRoot { uint32_t q[12]; f3 qscale, qbase; };               // the root node's plane words Q0, Q1, Q2 (crt_bvh.cpp)
struct TcTiles { uint32_t x0, y0, tw, th, band, stride, phase, tiles_x; };

CRT_HD TcCam tc_cam(const float cam[12], uint32_t W, uint32_t H)
{
    return TcCam{f3{cam[0], cam[1], cam[2]}, f3{cam[3], cam[4], cam[5]}, f3{cam[6], cam[7], cam[8]}, f3{cam[9], cam[10], cam[11]},
                 (float)W, (float)H};
}

// Lane l of tile t: its full-frame pixel (k_wf_gen's mapping); false outside a ragged tile.
CRT_HD bool tc_pixel(const TcTiles &T, uint32_t tile, uint32_t l, uint32_t &px, uint32_t &py)
{
    const uint32_t lx = (tile % T.tiles_x) * 8u + (l & 7u), ly = (tile / T.tiles_x) * 8u + (l >> 3);
    px = T.x0 + lx;
    py = T.y0 + (ly / T.band) * T.band * T.stride + T.phase * T.band + ly % T.band;
    return lx < T.tw && ly < T.th;
}

CRT_HD bool tc_finite(float v) { return abs_(v) <= 3.402823466e38f; }     // (false for a NaN)

// ---------------------------------------------------------------- the scalar functions
// camera_ray's direction (crt_wavefront.hip) with the two film jitters as inputs.
CRT_HD float tc_film(float base, float sgrid, float j, float n) { return (base + (sgrid + j) / (float)kTcGrid) / n; }
CRT_HD f3 tc_camera_dir(const TcCam &C, uint32_t px, uint32_t py, uint32_t sample, float jx, float jy)
{
    const float fs = tc_film((float)px, (float)(sample % kTcGrid), jx, C.W);
    const float ft = tc_film(C.H - (float)py, (float)(sample % kTcGrid), jy, C.H);
    return normalize(((C.llc + C.hor * fs) + C.ver * ft) - C.eye);
}

CRT_HD float tc_clamp(float d) { const float tiny = 1.0e-20f; return abs_(d) > tiny ? d : __builtin_copysignf(tiny, d); }
// the quantised plane of box k on an axis: lo planes in words 0..5 (x, y, z: two words each), hi planes in words 6..11
CRT_HD float tc_plane(const TcRoot &R, uint32_t axis, bool hi, uint32_t k)
{
    const uint32_t w = R.q[(hi ? 6u : 0u) + 2u * axis + (k >> 1)];
    return (float)((k & 1u) ? w >> 16 : w & 0xFFFFu);
}

// root_step_misses (crt_wavefront.hip): the four keys of a camera ray (t_min 0.001, t_max infinite); true when no box is entered.
CRT_HD bool tc_root_step_misses(const TcRoot &R, f3 ro, f3 rd)
{
    const float t_min = 0.001f, t_max = bits_f(0x7F800000u);
    const float rdv[3] = {rd.x, rd.y, rd.z}, rov[3] = {ro.x, ro.y, ro.z};
    const float qs[3] = {R.qscale.x, R.qscale.y, R.qscale.z}, qb[3] = {R.qbase.x, R.qbase.y, R.qbase.z};
    float oid[3], id[3];
    bool g[3];
    for (int a = 0; a < 3; a++) {
        const float i3 = 1.0f / tc_clamp(rdv[a]);
        oid[a] = fma_(qb[a], i3, -(rov[a] * i3));
        id[a] = qs[a] * i3;
        g[a] = i3 < 0.0f;                                            // the hi plane is the near one on that axis
    }
    bool miss = true;
    for (uint32_t k = 0; k < 4u; k++) {
        float n[3], f[3];
        for (uint32_t a = 0; a < 3u; a++) {
            n[a] = fma_(tc_plane(R, a, g[a], k), id[a], oid[a]);
            f[a] = fma_(tc_plane(R, a, !g[a], k), id[a], oid[a]);
        }
        const float tn = __builtin_fmaxf(__builtin_fmaxf(n[0], n[1]), __builtin_fmaxf(n[2], t_min));
        const float tf = __builtin_fminf(__builtin_fminf(f[0], f[1]), __builtin_fminf(f[2], t_max));
        const float key = (tn <= tf * 1.0000005f) ? tn : 3.0e38f;
        if (key < 3.0e38f) miss = false;
    }
    return miss;
}

// ---------------------------------------------------------------- the interval forms
struct iv { float lo, hi; };
CRT_HD iv iv_pt(float v) { return iv{v, v}; }
CRT_HD bool iv_finite(iv a) { return tc_finite(a.lo) && tc_finite(a.hi); }
// the hull of four corner values; a NaN among them stays one (min_ / max_ would drop it)
CRT_HD iv iv_hull(float a, float b, float c, float d)
{
    if (a != a || b != b || c != c || d != d) return iv{bits_f(0x7FC00000u), bits_f(0x7FC00000u)};
    return iv{min_(min_(a, b), min_(c, d)), max_(max_(a, b), max_(c, d))};
}
CRT_HD iv iv_add(iv a, iv b) { return iv{a.lo + b.lo, a.hi + b.hi}; }
CRT_HD iv iv_sub(iv a, iv b) { return iv{a.lo - b.hi, a.hi - b.lo}; }
CRT_HD iv iv_neg(iv a) { return iv{-a.hi, -a.lo}; }
CRT_HD iv iv_mul(iv a, iv b) { return iv_hull(a.lo * b.lo, a.lo * b.hi, a.hi * b.lo, a.hi * b.hi); }
CRT_HD iv iv_div(iv a, iv b) { return iv_hull(a.lo / b.lo, a.lo / b.hi, a.hi / b.lo, a.hi / b.hi); }   // b: one sign, without zero
// fma(a, b, c): one rounding of a * b + c -- monotone in c, and for a fixed c extreme at a corner of (a, b)
CRT_HD iv iv_fma(iv a, iv b, iv c)
{
    const iv l = iv_hull(fma_(a.lo, b.lo, c.lo), fma_(a.lo, b.hi, c.lo), fma_(a.hi, b.lo, c.lo), fma_(a.hi, b.hi, c.lo));
    const iv h = iv_hull(fma_(a.lo, b.lo, c.hi), fma_(a.lo, b.hi, c.hi), fma_(a.hi, b.lo, c.hi), fma_(a.hi, b.hi, c.hi));
    return iv{l.lo, h.hi};
}
// a * a and fma(a, a, c): the square of an interval that holds zero has the lower bound 0
CRT_HD iv iv_sq(iv a)
{
    const iv r = iv_hull(a.lo * a.lo, a.hi * a.hi, a.lo * a.lo, a.hi * a.hi);
    return (a.lo <= 0.0f && a.hi >= 0.0f) ? iv{0.0f, r.hi} : r;
}
CRT_HD iv iv_fma_sq(iv a, iv c)
{
    const iv l = iv_hull(fma_(a.lo, a.lo, c.lo), fma_(a.hi, a.hi, c.lo), fma_(a.lo, a.lo, c.lo), fma_(a.hi, a.hi, c.lo));
    const iv h = iv_hull(fma_(a.lo, a.lo, c.hi), fma_(a.hi, a.hi, c.hi), fma_(a.lo, a.lo, c.hi), fma_(a.hi, a.hi, c.hi));
    return (a.lo <= 0.0f && a.hi >= 0.0f) ? iv{fma_(0.0f, 0.0f, c.lo), h.hi} : iv{l.lo, h.hi};
}
CRT_HD iv iv_max(iv a, iv b) { return iv{__builtin_fmaxf(a.lo, b.lo), __builtin_fmaxf(a.hi, b.hi)}; }   // (finite operands)
CRT_HD iv iv_min(iv a, iv b) { return iv{__builtin_fminf(a.lo, b.lo), __builtin_fminf(a.hi, b.hi)}; }

// One signed part of a direction component after the clamp, and what the root step makes of it.  tc_clamp takes the
// sign from the sign bit, so a component interval that touches zero has both parts (either zero may occur): the negative
// part is [lo, -0], the positive one [+0, hi], and the clamp (monotone on each) maps them into (-inf, -tiny] and
// [tiny, inf), where the reciprocal is monotone and of one sign.
struct TcPart { iv oid, id; bool near_hi, ok; };
CRT_HD TcPart tc_part(iv d, bool negative, float ro, float qscale, float qbase)
{
    TcPart p;
    iv c;
    if (negative) c = iv{tc_clamp(d.lo < 0.0f ? d.lo : -0.0f), tc_clamp(d.hi < 0.0f ? d.hi : -0.0f)};
    else c = iv{tc_clamp(d.lo > 0.0f ? d.lo : 0.0f), tc_clamp(d.hi > 0.0f ? d.hi : 0.0f)};
    const iv i3 = iv{1.0f / c.hi, 1.0f / c.lo};                      // 1 / x falls on either side of zero
    p.oid = iv_fma(iv_pt(qbase), i3, iv_neg(iv_mul(iv_pt(ro), i3)));
    p.id = iv_mul(iv_pt(qscale), i3);
    p.near_hi = negative;
    p.ok = iv_finite(i3) && iv_finite(p.oid) && iv_finite(p.id);
    return p;
}

// The class of one pixel: every sample, every jitter.
CRT_HD uint32_t tc_pixel_class(const TcCam &C, const TcRoot &R, uint32_t px, uint32_t py)
{
    const float t_min = 0.001f, t_max = bits_f(0x7F800000u);
    const float jmax = bits_f(0x3F7FFFFFu);                          // 1 - 2^-24: the largest value of rnd
    // the film position: +, / by positive constants, monotone -- its ends are the scalar expression at the ends
    const iv fs = iv{tc_film((float)px, 0.0f, 0.0f, C.W), tc_film((float)px, (float)(kTcGrid - 1u), jmax, C.W)};
    const iv ft = iv{tc_film(C.H - (float)py, 0.0f, 0.0f, C.H), tc_film(C.H - (float)py, (float)(kTcGrid - 1u), jmax, C.H)};
    const float llc[3] = {C.llc.x, C.llc.y, C.llc.z}, hor[3] = {C.hor.x, C.hor.y, C.hor.z}, ver[3] = {C.ver.x, C.ver.y, C.ver.z};
    const float eye[3] = {C.eye.x, C.eye.y, C.eye.z};
    const float qs[3] = {R.qscale.x, R.qscale.y, R.qscale.z}, qb[3] = {R.qbase.x, R.qbase.y, R.qbase.z};
    iv v[3];
    bool ok = iv_finite(fs) && iv_finite(ft) && tc_finite(eye[0]) && tc_finite(eye[1]) && tc_finite(eye[2]);
    for (int a = 0; a < 3; a++) {                                    // ((llc + hor * fs) + ver * ft) - eye
        v[a] = iv_sub(iv_add(iv_add(iv_pt(llc[a]), iv_mul(iv_pt(hor[a]), fs)), iv_mul(iv_pt(ver[a]), ft)), iv_pt(eye[a]));
        ok = ok && iv_finite(v[a]);
    }
    const iv len2 = iv_fma_sq(v[2], iv_fma_sq(v[1], iv_sq(v[0])));   // dot(a, a) = fma(z, z, fma(y, y, x * x))
    const iv len = iv{sqrt_(len2.lo), sqrt_(len2.hi)};
    ok = ok && iv_finite(len2) && iv_finite(len) && len.lo > 0.0f;
    if (!ok) return kTcMaybe;
    iv d[3];
    for (int a = 0; a < 3; a++) {
        d[a] = iv_div(v[a], len);
        if (!iv_finite(d[a])) return kTcMaybe;
    }
    bool all_miss = true, all_enter = true;
    for (uint32_t combo = 0; combo < 8u; combo++) {                  // bit a: the negative part of axis a
        TcPart p[3];
        bool exists = true;
        for (uint32_t a = 0; a < 3u; a++) {
            const bool negative = ((combo >> a) & 1u) != 0u;
            if (negative ? !(d[a].lo <= 0.0f) : !(d[a].hi >= 0.0f)) { exists = false; break; }
            p[a] = tc_part(d[a], negative, eye[a], qs[a], qb[a]);
        }
        if (!exists) continue;
        if (!p[0].ok || !p[1].ok || !p[2].ok) return kTcMaybe;
        bool some_enter = false;
        for (uint32_t k = 0; k < 4u; k++) {
            iv n[3], f[3];
            for (uint32_t a = 0; a < 3u; a++) {
                n[a] = iv_fma(iv_pt(tc_plane(R, a, p[a].near_hi, k)), p[a].id, p[a].oid);
                f[a] = iv_fma(iv_pt(tc_plane(R, a, !p[a].near_hi, k)), p[a].id, p[a].oid);
                if (!iv_finite(n[a]) || !iv_finite(f[a])) return kTcMaybe;
            }
            const iv tn = iv_max(iv_max(n[0], n[1]), iv_max(n[2], iv_pt(t_min)));
            const iv tf = iv_min(iv_min(f[0], f[1]), iv_min(f[2], iv_pt(t_max)));
            if (!(tn.lo > tf.hi * 1.0000005f)) all_miss = false;     // some ray of the part may enter box k
            if (tn.hi <= tf.lo * 1.0000005f && tn.hi < 3.0e38f) some_enter = true;   // every ray of the part enters box k
        }
        if (!some_enter) all_enter = false;
    }
    return all_miss ? kTcMiss : all_enter ? kTcEnter : kTcMaybe;     // (some part exists: both cannot hold)
}

// The class of a tile: what all of its valid pixels agree on.  (The device form takes one lane per pixel and two ballots.)
CRT_HD uint32_t tc_tile_class(const TcCam &C, const TcRoot &R, const TcTiles &T, uint32_t tile)
{
    bool any = false, all_miss = true, all_enter = true;
    for (uint32_t l = 0; l < 64u; l++) {
        uint32_t px, py;
        if (!tc_pixel(T, tile, l, px, py)) continue;
        const uint32_t cls = tc_pixel_class(C, R, px, py);
        any = true;
        all_miss = all_miss && cls == kTcMiss;
        all_enter = all_enter && cls == kTcEnter;
    }
    return !any ? kTcMaybe : all_miss ? kTcMiss : all_enter ? kTcEnter : kTcMaybe;
}

// What a culled path stores for a first wavelength index: spectral_to_xyz (crt_shade.h) of zero radiance, restated.  +0 in
// all three whenever the 12 gathered CIE entries are finite and not all negative; k_wf_gen stores the constant for a MISS
// chunk only where tc_culled_is_zero holds for the uploaded table.
CRT_HD f3 tc_culled_xyz(const float *cie, uint32_t lambda0)
{
    const uint32_t wl[4] = {lambda0, (lambda0 + 4u) % kTcNLambda, (lambda0 + 8u) % kTcNLambda, (lambda0 + 12u) % kTcNLambda};
    const float *X = cie, *Y = cie + kTcNCie, *Z = cie + 2 * kTcNCie;
    const f4 zero = f4{0.0f, 0.0f, 0.0f, 0.0f};
    const f4 xb = f4{X[wl[0] + 40], X[wl[1] + 40], X[wl[2] + 40], X[wl[3] + 40]};
    const f4 yb = f4{Y[wl[0] + 40], Y[wl[1] + 40], Y[wl[2] + 40], Y[wl[3] + 40]};
    const f4 zb = f4{Z[wl[0] + 40], Z[wl[1] + 40], Z[wl[2] + 40], Z[wl[3] + 40]};
    const f3 xyzc = f3{dot(xb, zero), dot(yb, zero), dot(zb, zero)};
    return (xyzc * 300.0f) / (106.856895f * 4.0f);
}
CRT_HD bool tc_culled_is_zero(const float *cie)
{
    for (uint32_t l = 0; l < kTcNLambda; l++) {
        const f3 c = tc_culled_xyz(cie, l);
        if (f_bits(c.x) != 0u || f_bits(c.y) != 0u || f_bits(c.z) != 0u) return false;
    }
    return true;
}

}  // namespace crt
