// Arithmetic of the image-gradient keypoint selectors (GradientSelector / SparseGradienSelector, Module/KeypointSelector.py:121-213), shared by the
// kernels of kp_gradient.hip and their host twin (tests/c_abi/kp_grad_twin.cpp): one definition of every rounding step and of the order of every sum.
//
//   grad  = |conv2d(image [3, H, W], Laplacian [[0,1,0],[1,-4,1],[0,1,0]] over the 3 channels, padding = 1)|          (:129-135, :172-178)
//   thr   = grad.mean() + grad_std * grad.std()    (unbiased)                                                          (:136-139, :179-182)
//   cand  = grad > thr  &  border [m:-m, m:-m]  [&  grad == max_pool2d(grad, nms_size, 1, nms_size // 2)]              (:139-147, :182-201)
//
// Per pixel (fp32, no contraction): per channel ((up + down) + (left + right)) - 4 * c with zeros outside the image, the channels added in order
// 0, 1, 2, then fabsf.  Mean and standard deviation come from fp64 sums of g and g * g in a FIXED order:
//   thread    (tile column tx, wave ty): its PX_PER_THREAD pixels, rows ty * PX_PER_THREAD + 0 .. in order (a pixel outside the image adds nothing)
//   wave      the xor butterfly over its 64 lanes, offsets 32, 16, 8, 4, 2, 1  (v[i] + v[i ^ o]: both partners form the same sum)
//   tile      ((wave 0 + wave 1) + wave 2) + wave 3
//   image     the tiles in ascending index (tile row * tiles per row + tile column), one after the other
// so a lane's bits do not depend on the launch, the lane count or the run.  var = (S2 - n * mean^2) / (n - 1) in fp64 (a negative rounding residue of a
// constant plane counts as 0), mean and sqrt(var) are rounded to fp32 once each, thr = mean32 + (float)grad_std * std32 in fp32.  A NaN anywhere makes
// both sums NaN, thr NaN and every compare false: no candidates, as in the reference.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MV_KG_FN __host__ __device__ __forceinline__
#else
#define MV_KG_FN inline
#endif

namespace mvkg {

constexpr int TILE_W = 64;            // one 64-pixel candidate word (= one wave) per tile row
constexpr int TILE_H = 16;
constexpr int WAVES = 4;              // 256 threads: thread (tx, ty) owns column tx, rows ty * PX_PER_THREAD ..
constexpr int PX_PER_THREAD = TILE_H / WAVES;
constexpr int MAX_R = 7;              // nms_size <= 15

MV_KG_FN float laplace(float c, float up, float down, float left, float right) { return ((up + down) + (left + right)) - 4.f * c; }
MV_KG_FN float grad_of(float l0, float l1, float l2) { return fabsf((l0 + l1) + l2); }

struct Sums {
    double s, s2;
};
MV_KG_FN void accumulate(Sums& a, float g) {
    a.s += (double)g;
    a.s2 += (double)g * (double)g;
}
MV_KG_FN Sums add(const Sums& a, const Sums& b) { return Sums{a.s + b.s, a.s2 + b.s2}; }

struct Stats {
    float mean, std, thr;
};
MV_KG_FN Stats stats_of(const Sums& t, int64_t n, float grad_std) {
    const double mean = t.s / (double)n;
    double var = (t.s2 - (double)n * (mean * mean)) / (double)(n - 1);
    if (var < 0.0) var = 0.0;        // (a NaN stays a NaN)
    Stats o;
    o.mean = (float)mean;
    o.std = (float)sqrt(var);
    o.thr = o.mean + grad_std * o.std;
    return o;
}

// the border mask [m:-m, m:-m]: the empty slice 0:-0 for m = 0, empty as well for 2m >= H or 2m >= W
MV_KG_FN bool in_border(int x, int y, int W, int H, int m) { return m > 0 && x >= m && x < W - m && y >= m && y < H - m; }

}  // namespace mvkg
