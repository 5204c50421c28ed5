// Host driver for tests/test_augment_hs_ref_host.py: csrc/hs_pixel.h - the expressions the kernel of csrc/augment.hip
// evaluates per pixel - compiled for the CPU and evaluated on every input.  Writes, into the directory given as argv[1]:
//   hsv.bin     hs_rgb_to_hsv of every colour R << 16 | G << 8 | B                      [2^24][3] bytes
//   rgb.bin     hs_hsv_to_rgb of every triple H << 16 | S << 8 | V, through the per-H and per-S values
//               (hs_hue_sector, hs_sat_unit) as the kernel tabulates them                [2^24][3] bytes
//   grey.bin    hs_grey of every colour                                                 [2^24] bytes
//   sat<j>.bin  hs_blend(L, c, argv[2 + j]) of every grey value L and channel byte c    [256][256] bytes
// (the saturation of a pixel is hs_blend of its hs_grey with each of its channels: these two domains are all of it)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "hs_pixel.h"

static int dump(const std::string& path, const std::vector<uint8_t>& v) {
    FILE* fp = fopen(path.c_str(), "wb");
    if (!fp) return 1;
    const size_t n = fwrite(v.data(), 1, v.size(), fp);
    return (fclose(fp) != 0 || n != v.size()) ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const size_t N = (size_t)1 << 24;
    std::vector<uint8_t> hsv(3 * N), rgb(3 * N), grey(N);
    int sector[256];
    float frac[256], unit[256];
    for (int h = 0; h < 256; ++h) {
        hs_hue_sector(h, sector[h], frac[h]);
        unit[h] = hs_sat_unit(h);
    }
    for (size_t k = 0; k < N; ++k) {
        const int a = (int)(k >> 16) & 255, b = (int)(k >> 8) & 255, c = (int)k & 255;
        int h, s, v, r, g, bl;
        hs_rgb_to_hsv(a, b, c, h, s, v);
        hsv[3 * k] = (uint8_t)h, hsv[3 * k + 1] = (uint8_t)s, hsv[3 * k + 2] = (uint8_t)v;
        hs_hsv_to_rgb(sector[a], frac[a], unit[b], b, c, r, g, bl);
        rgb[3 * k] = (uint8_t)r, rgb[3 * k + 1] = (uint8_t)g, rgb[3 * k + 2] = (uint8_t)bl;
        grey[k] = (uint8_t)hs_grey(a, b, c);
    }
    if (dump(dir + "/hsv.bin", hsv) || dump(dir + "/rgb.bin", rgb)) return 1;
    if (dump(dir + "/grey.bin", grey)) return 1;
    std::vector<uint8_t> sat(256 * 256);
    for (int j = 0; j + 2 < argc; ++j) {
        const float f = (float)atof(argv[2 + j]);                           // the double, rounded as Pillow's `float alpha`
        const bool inside = f >= 0.0f && f <= 1.0f;
        for (int L = 0; L < 256; ++L)
            for (int c = 0; c < 256; ++c) sat[256 * L + c] = (uint8_t)hs_blend(L, c, f, inside);
        if (dump(dir + "/sat" + std::to_string(j) + ".bin", sat)) return 1;
    }
    return 0;
}
