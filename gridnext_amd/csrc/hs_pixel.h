// Pillow's per-pixel colour arithmetic, operation for operation: ImageEnhance.Color's blend with the grey value, and the
// RGB <-> HSV byte conversions of Image.convert (libImaging Convert.c: rgb2hsv_row, hsv2rgb_row; Blend.c).  Plain C++ that a
// host compiler takes as well, so the expressions can be compared with the numpy restatement (gridnext_amd/transforms.py:
// saturate_u8, rgb_to_hsv_u8, hsv_to_rgb_u8) on every colour without a device.
//
// Every rounding is the one Pillow's C makes: `float` variables round to float32 where they are assigned, everything else is
// double.  The compiler must not fuse a product into the following sum (hipcc does by default), hence the pragma in every
// function; the divisions are IEEE divisions (hipcc's default for both widths), never a reciprocal and a product.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HS_FN __host__ __device__ __forceinline__
#else
#define HS_FN inline
#endif

// Pillow's convert('L') of one pixel
HS_FN int hs_grey(int r, int g, int b) { return (int)((19595u * (unsigned)r + 38470u * (unsigned)g + 7471u * (unsigned)b + 0x8000u) >> 16); }

// Image.blend(grey, image, f) of one channel byte: `inside` = 0 <= f <= 1, where Pillow truncates without clipping
HS_FN int hs_blend(int L, int c, float f, bool inside) {
#pragma clang fp contract(off)
    const float t = (float)L + f * (float)(c - L);
    if (inside) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

HS_FN int hs_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// rgb2hsv_row
HS_FN void hs_rgb_to_hsv(int r, int g, int b, int& uh, int& us, int& uv) {
#pragma clang fp contract(off)
    const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
    const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
    uv = maxc;
    if (maxc == minc) {
        uh = us = 0;
        return;
    }
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    // the two of rc, gc, bc that the maximum's branch reads: h = off + q1 - q2
    const bool rmax = r == maxc, gmax = !rmax && g == maxc;
    const float q1 = (float)(maxc - (rmax ? b : (gmax ? r : g))) / cr;
    const float q2 = (float)(maxc - (rmax ? g : (gmax ? b : r))) / cr;
    float h;
    if (rmax)
        h = q1 - q2;                                                    // float32
    else
        h = (float)(((gmax ? 2.0 : 4.0) + (double)q1) - (double)q2);    // the literal is a double
    const double x = (double)h / 6.0 + 1.0;                             // 0.83 <= x < 1.84: fmod(x, 1.0) = x - floor(x), exactly
    h = (float)(x - floor(x));
    uh = hs_clip8((int)((double)h * 255.0));
    us = hs_clip8((int)((double)s * 255.0));
}

// What hsv2rgb_row derives from h alone, i = floor(h * 6.0 / 255.0) % 6 and float f = h * 6.0 / 255.0 - i, and from s alone,
// float fs = s / 255.0: 256 values each, which the kernel keeps in tables.
HS_FN void hs_hue_sector(int h, int& i, float& f) {
#pragma clang fp contract(off)
    const double x = (double)h * 6.0 / 255.0;
    const double fl = floor(x);
    f = (float)(x - fl);
    i = (int)fl % 6;
}

HS_FN float hs_sat_unit(int s) { return (float)((double)s / 255.0); }

HS_FN int hs_round8(double x) { return hs_clip8((int)round(x)); }       // round: halves away from zero

// hsv2rgb_row, given the values above for this pixel's h and s
HS_FN void hs_hsv_to_rgb(int i, float f, float fs, int s, int v, int& r, int& g, int& b) {
#pragma clang fp contract(off)
    if (s == 0) {
        r = g = b = v;
        return;
    }
    const double dv = (double)v;
    const float fsf = fs * f;                                            // float32 product
    const int p = hs_round8(dv * (1.0 - (double)fs));
    const int q = hs_round8(dv * (1.0 - (double)fsf));
    const int t = hs_round8(dv * (1.0 - (double)fs * (1.0 - (double)f)));
    r = (i == 0 || i == 5) ? v : (i == 1 ? q : (i == 4 ? t : p));
    g = (i == 1 || i == 2) ? v : (i == 0 ? t : (i == 3 ? q : p));
    b = (i == 3 || i == 4) ? v : (i == 2 ? t : (i == 5 ? q : p));
}
