// TEST INFRASTRUCTURE: host replay of the per-pixel arithmetic of the 8-bit bilinear remap (mac-vo_amd/csrc/remap.hip).  It includes the kernel's own arithmetic
// header (csrc/remap_math.h) and calls the same functions — quantise, tap mask, blend, / 255 — one output pixel after the other.  Built by tests/remap_twin.py
// with g++ -ffp-contract=off.  The product never builds or loads it.
//
// With -DREMAP_TWIN_MAIN it is a plain stand-alone program (its own main) for a host-only -fsanitize=address,undefined run.
#include <stddef.h>

#include <vector>

#include "../../mac-vo_amd/csrc/remap_math.h"

// src uint8 [h][w][C] (hwc != 0) or [C][h][w]; maps fp32 [oh][ow]; dst uint8 planar [C][oh][ow]
extern "C" void remap_twin_u8(const uint8_t* src, int h, int w, int C, int hwc, int reverse, const float* mx, const float* my, int oh, int ow, uint8_t* dst) {
    const size_t plane = (size_t)h * w, oplane = (size_t)oh * ow;
    for (size_t i = 0; i < oplane; ++i) {
        const rmm::Tap t = rmm::tap_of(mx[i], my[i]);
        for (int c = 0; c < C; ++c) {
            const int sc = rmm::src_channel(c, C, reverse);
            dst[c * oplane + i] = (uint8_t)rmm::sample(t, w, h, [&](int y, int x) {
                const size_t p = (size_t)y * w + x;
                return hwc ? src[p * C + sc] : src[sc * plane + p];
            });
        }
    }
}

// out[256]: what a float destination stores for every byte value
extern "C" void remap_twin_unit(float* out) {
    for (int v = 0; v < 256; ++v) out[v] = rmm::unit(v);
}

// the fixed-point form of one map coordinate: returns ok, writes s
extern "C" int remap_twin_quantise(float m, int32_t* s) { return rmm::quantise(m, *s) ? 1 : 0; }

#ifdef REMAP_TWIN_MAIN
#include <stdio.h>
int main() {
    const int h = 37, w = 53, oh = 29, ow = 61;
    const float nan = NAN, inf = INFINITY;
    const float crafted[] = {0.5f / 32, 1.5f / 32, 2.5f / 32, -0.5f / 32, -0.25f, -0.99f, -1.0f, w - 1 + 0.5f, h - 1 + 0.5f, (float)(w - 1), (float)(h - 1), 1e9f,
                             -1e9f, inf, -inf, nan, 33554432.0f, -33554432.0f, 3.4e38f};
    const int nc = (int)(sizeof(crafted) / sizeof(crafted[0]));
    long sum = 0;
    for (int C : {1, 3, 4})
        for (int hwc = 0; hwc < 2; ++hwc) {
            std::vector<uint8_t> src((size_t)h * w * C), dst((size_t)oh * ow * C);
            std::vector<float> mx((size_t)oh * ow), my((size_t)oh * ow);
            uint32_t s = 12345u + C;
            for (auto& b : src) b = (uint8_t)((s = s * 1664525u + 1013904223u) >> 24);
            for (size_t i = 0; i < mx.size(); ++i) {
                mx[i] = -3.f + (w + 6.f) * (float)((s = s * 1664525u + 1013904223u) >> 8) / 16777216.f;
                my[i] = -3.f + (h + 6.f) * (float)((s = s * 1664525u + 1013904223u) >> 8) / 16777216.f;
            }
            for (int a = 0; a < nc; ++a)
                for (int b = 0; b < nc; ++b) {                 // every crafted value on either axis against every other
                    const size_t i = (size_t)a * nc + b;
                    if (i < mx.size()) mx[i] = crafted[a], my[i] = crafted[b];
                }
            remap_twin_u8(src.data(), h, w, C, hwc, C >= 3, mx.data(), my.data(), oh, ow, dst.data());
            for (uint8_t b : dst) sum += b;
        }
    float unit[256];
    remap_twin_unit(unit);
    if (unit[0] != 0.f || unit[255] != 1.f) return 1;
    printf("remap_twin OK: checksum %ld\n", sum);
    return 0;
}
#endif
