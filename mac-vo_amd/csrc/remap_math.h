// Per-pixel arithmetic of the 8-bit bilinear remap (csrc/remap.hip), shared by the kernel and by a host twin (tests/c_abi/remap_twin.cpp), as
// resample_math.h and se3_interp.h are shared.
//
// Restates, parity-unpinned, OpenCV's fixed-point `remap(..., INTER_LINEAR)` of an 8-bit image under BORDER_CONSTANT 0 (what
// DataLoader/Dataset/EuRoC.py:231-236 and VBR.py:60-64 run on every image), entirely in integers:
//   s = rndne(map * 32) in fp32 (round half to even), per axis; i = s >> 5 (an arithmetic shift: floor for negatives), f = s & 31;
//   the taps (ix, iy) .. (ix + 1, iy + 1) are read where they fall inside the source, a tap outside counts 0, each one on its own;
//   S = (32 - fx)(32 - fy) p00 + fx (32 - fy) p01 + (32 - fx) fy p10 + fx fy p11;  out = (S + 512) >> 10.
// For fractions in 1/32 OpenCV's 15-bit weight table holds exactly 32 times these integer weights (they sum to 32768 without its correction step), so
// (S * 32 + 2^14) >> 15 is this expression.
// Defined where OpenCV's result depends on the platform: a NaN map entry, or one whose * 32 leaves [-2^30, 2^30] (+-inf included), yields 0.
// Float destinations store float(out) / 255.0f, a true IEEE division (the loaders' `result /= 255.`), rounded once more for fp16 / bf16.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RMM_HD __host__ __device__ __forceinline__
#else
#define RMM_HD static inline
#endif

namespace rmm {

constexpr int kFracBits = 5, kFrac = 1 << kFracBits;           // 1/32 pixel
constexpr float kLimit = 1073741824.0f;                         // 2^30: |s| <= 2^30 keeps s, s >> 5 and s + 32 inside an int

// one map coordinate -> its fixed-point form; false for NaN and anything outside [-2^30, 2^30] after the scaling
RMM_HD bool quantise(float m, int32_t& s) {
    const float v = m * (float)kFrac;
    if (!(v >= -kLimit && v <= kLimit)) {
        s = 0;
        return false;
    }
    s = (int32_t)rintf(v);                                      // the default rounding mode on the host, v_rndne_f32 on the device: half to even
    return true;
}

struct Tap {
    int32_t ix, iy, fx, fy;
    bool ok;                                                    // false: the pixel is 0 whatever the source holds
};

RMM_HD Tap tap_of(float mx, float my) {
    int32_t sx, sy;
    const bool okx = quantise(mx, sx), oky = quantise(my, sy);
    Tap t;
    t.ix = sx >> kFracBits, t.iy = sy >> kFracBits;
    t.fx = sx & (kFrac - 1), t.fy = sy & (kFrac - 1);
    t.ok = okx && oky;
    return t;
}

RMM_HD bool inside(int32_t x, int32_t y, int32_t w, int32_t h) { return x >= 0 && x < w && y >= 0 && y < h; }
// all four taps inside the source
RMM_HD bool interior(const Tap& t, int32_t w, int32_t h) { return t.ix >= 0 && t.ix < w - 1 && t.iy >= 0 && t.iy < h - 1; }

RMM_HD int32_t blend(const Tap& t, int32_t p00, int32_t p01, int32_t p10, int32_t p11) {
    const int32_t S = (kFrac - t.fx) * (kFrac - t.fy) * p00 + t.fx * (kFrac - t.fy) * p01 + (kFrac - t.fx) * t.fy * p10 + t.fx * t.fy * p11;
    return (S + (1 << (2 * kFracBits - 1))) >> (2 * kFracBits);
}

// one output value through a fetch(y, x) -> uint8 that is only called for taps inside the w x h source
template <class Fetch>
RMM_HD int32_t sample(const Tap& t, int32_t w, int32_t h, Fetch fetch) {
    if (!t.ok) return 0;
    const int32_t p00 = inside(t.ix, t.iy, w, h) ? (int32_t)fetch(t.iy, t.ix) : 0;
    const int32_t p01 = inside(t.ix + 1, t.iy, w, h) ? (int32_t)fetch(t.iy, t.ix + 1) : 0;
    const int32_t p10 = inside(t.ix, t.iy + 1, w, h) ? (int32_t)fetch(t.iy + 1, t.ix) : 0;
    const int32_t p11 = inside(t.ix + 1, t.iy + 1, w, h) ? (int32_t)fetch(t.iy + 1, t.ix + 1) : 0;
    return blend(t, p00, p01, p10, p11);
}

RMM_HD float unit(int32_t v) { return (float)v / 255.0f; }

// the source channel a destination channel reads: reverse_channels swaps channels 0 and 2 (BGR <-> RGB; a fourth channel stays where it is)
RMM_HD int src_channel(int c, int channels, int reverse) { return (reverse && channels >= 3 && c < 3) ? 2 - c : c; }

}  // namespace rmm
