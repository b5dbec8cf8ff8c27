// lens.h -- row f4's arithmetic, stated ONCE for the host and the device (DESIGN.md section 4 "View input"): where an output pixel of the
// undistorted image finds its colour in the distorted one.  undistort_kernel (k_prep.hip, one image per launch), lens_kernel (k_lens.hip,
// a batch of views per launch) and the sequential host twin below all call lens_source(); oracle/oracle.cpp restates it independently.
//   generate_texture_views.cpp:153-165: mve::image::image_undistort_k2k4 when both coefficients are set, image_undistort_vsfm when only
//   the first is, a plain copy when the first is zero.  MVE is absent; DEFINED HERE from recollection of mve/image_tools.h: every pixel of
//   the UNDISTORTED output looks up its position in the distorted source -- coordinates centred on (w/2, h/2) and normalised by
//   max(w, h), rsq = (fx^2 + fy^2) / flen^2 -- and samples it with Image::linear_at (dmath.h); positions more than half a pixel outside
//   stay black.  k2k4: factor = 1 + rsq k2 + rsq^2 k4.  vsfm (x_u = x_d (1 + k1 r_d^2), to be inverted): 8 guarded Newton steps on
//   k1 r_d^3 + r_d - r_u = 0 in fp64 from r_d = r_u.  An APPROXIMATION of MVE's routine (believed to solve the cubic in closed form):
//   identical where Newton converges, i.e. to ~1e-16 relative.
// The text is fp64 + - * / and sqrt only, compiled with -ffp-contract=off (DESIGN.md section 4 "Exactness"): the GPU and the CPU agree
// bit for bit.  tests/cpp/test_lens.cpp runs the host side under the sanitizers.
#pragma once
#include <math.h>
#include <string>

#include "../../include/mvs_viewsel.h"
#include "dmath.h"

namespace mvs {

// the position (sx, sy) in the distorted w x h image that output pixel (x, y) samples, clamped to the image; false: the pixel has no source
MVS_HD bool lens_source(int x, int y, int w, int h, double flen, double d0, double d1, double& sx, double& sy) {
    const double width_half = (double)w / 2.0, height_half = (double)h / 2.0, norm = (double)(w > h ? w : h);
    double fx = ((double)x - width_half) / norm, fy = ((double)y - height_half) / norm;
    double factor;
    bool ok = true;
    if (d1 != 0.0) {
        const double rsq = (fx * fx + fy * fy) / (flen * flen);
        factor = 1.0 + rsq * d0 + (rsq * rsq) * d1;
    } else {
        const double ru = sqrt(fx * fx + fy * fy) / flen;
        double rd = ru;
        // guarded: for k1 < 0 the cubic has a turning point at r_d = 1 / sqrt(-3 k1) (derivative 3 k1 r_d^2 + 1 -> 0); beyond it there is
        // no distorted radius on the monotone branch.  A step whose derivative is not safely positive, or an iteration that has
        // not converged (residual against r_u), marks the pixel as having no source: it stays black.
        for (int it = 0; it < 8 && ok; ++it) {
            const double den = (3.0 * d0) * (rd * rd) + 1.0;
            if (!(den > 1e-3)) ok = false; else rd = rd - (((d0 * rd) * rd) * rd + rd - ru) / den;
        }
        if (ok) { const double res = ((d0 * rd) * rd) * rd + rd - ru; ok = (res < 0.0 ? -res : res) <= 1e-9 * (1.0 + ru); }
        factor = ru > 0.0 ? rd / ru : 1.0;
    }
    if (!ok) return false;
    fx = (fx * factor) * norm + width_half;
    fy = (fy * factor) * norm + height_half;
    if (!(fx >= -0.5 && fx <= (double)w - 0.5 && fy >= -0.5 && fy <= (double)h - 0.5)) return false;   // the half-pixel outside test
    sx = fx < 0.0 ? 0.0 : (fx > (double)w - 1.0 ? (double)w - 1.0 : fx);
    sy = fy < 0.0 ? 0.0 : (fy > (double)h - 1.0 ? (double)h - 1.0 : fy);
    return true;
}

// output pixel (x, y) of the undistorted image; false: black, no source
MVS_HD bool lens_pixel(const uint8_t* src, int w, int h, int x, int y, double flen, double d0, double d1, uint8_t rgb[3]) {
    double sx, sy;
    if (!lens_source(x, y, w, h, flen, d0, d1, sx, sy)) { rgb[0] = rgb[1] = rgb[2] = 0; return false; }
    for (int c = 0; c < 3; ++c) rgb[c] = linear_at(src, w, h, 3, (float)sx, (float)sy, c);
    return true;
}

// A view's MASK under a lens (DESIGN.md section 4 "View input" item 10): `mask` is a [h][w] byte image in the camera's frame, 0 = leave out,
// anything else = keep.  It is read as the one-channel image of 0 / 255 and undistorted as a colour channel is: output pixel (x, y) is
// kept iff it has a source and linear_at there gives the byte 255.  The expression is linear_at's (dmath.h), restated on the two
// values a tap can take, so that this equals undistorting the 0 / 255 replica and comparing with 255, bit for bit.
MVS_HD bool lens_keep(const uint8_t* mask, int w, int h, int x, int y, double flen, double d0, double d1) {
    double sx, sy;
    if (!lens_source(x, y, w, h, flen, d0, d1, sx, sy)) return false;
    const float fx = smax(0.0f, smin((float)(w - 1), (float)sx)), fy = smax(0.0f, smin((float)(h - 1), (float)sy));
    const int floor_x = (int)fx, floor_y = (int)fy;
    const int floor_xp1 = imin(floor_x + 1, w - 1), floor_yp1 = imin(floor_y + 1, h - 1);
    const float w1 = fx - (float)floor_x, w0 = 1.0f - w1;
    const float w3 = fy - (float)floor_y, w2 = 1.0f - w3;
    const size_t row1 = (size_t)floor_y * w, row2 = (size_t)floor_yp1 * w;
    const float v1 = mask[row1 + floor_x] ? 255.0f : 0.0f, v2 = mask[row1 + floor_xp1] ? 255.0f : 0.0f;
    const float v3 = mask[row2 + floor_x] ? 255.0f : 0.0f, v4 = mask[row2 + floor_xp1] ? 255.0f : 0.0f;
    return (uint8_t)(((v1 * (w0 * w2) + v2 * (w1 * w2)) + v3 * (w0 * w3)) + v4 * (w1 * w3) + 0.5f) == 255;
}

// what is wrong with a view's lens (empty: nothing).  dist0 == 0 is a plain copy whatever flen and dist1 say, as long as they are numbers.
inline std::string lens_refusal(const mvs_lens& L) {
    if (!isfinite(L.flen) || !isfinite(L.dist0) || !isfinite(L.dist1)) return "lens: flen, dist0 and dist1 must be finite";
    if (L.reserved != 0u) return "lens: reserved must be 0";
    if (L.dist0 != 0.0f && !(L.flen > 0.0f)) return "lens: undistortion needs a positive focal length";
    return std::string();
}

// the sequential host twin: rgb [h][w][3] -> out, pixel by pixel; returns the pixels without a source
inline uint64_t undistort_image_host(const uint8_t* rgb, int w, int h, float flen, float dist0, float dist1, uint8_t* out) {
    if (dist0 == 0.0f) { memcpy(out, rgb, (size_t)w * h * 3); return 0; }   // :153 -- only a non-zero first coefficient undistorts
    uint64_t none = 0;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            if (!lens_pixel(rgb, w, h, x, y, (double)flen, (double)dist0, (double)dist1, out + ((size_t)y * w + x) * 3)) ++none;
    return none;
}

}  // namespace mvs
