// Index and weight arithmetic of the frame resampler (csrc/preprocess.hip), shared by the kernels and by a host twin
// (tests/c_abi/resample_twin.cpp), as pgo_math.h and se3_interp.h are shared.
//
// Restates, parity-unpinned, what torchvision's `resize` on a tensor reaches through F.interpolate (DataLoader/Transform.py:74-86; torchvision is unpinned in
// the reference, requirements.txt:17):
//   nearest  = InterpolationMode.NEAREST_EXACT = mode "nearest-exact": src = min(floorf((dst + 0.5f) * (float(in) / float(out))), in - 1), all in fp32;
//   bilinear = mode "bilinear", align_corners False, antialias True, per axis with scale = in / out:
//                support = scale >= 1 ? scale : 1, invscale = scale >= 1 ? 1 / scale : 1, center = scale * (i + 0.5),
//                xmin = max(0, int(center - support + 0.5)), xmax = min(in, int(center + support + 0.5)),
//                w_j = max(0, 1 - |(j - center + 0.5) * invscale|) for j in [xmin, xmax), normalised to sum 1.
//              An axis whose size does not change is not resampled at all (torch skips that pass: a NaN does not spread along it).
// The window is computed in fp64 — it then equals the fp64 formula's exactly, no tap is gained or lost to an fp32 rounding of `center` — and so are the
// weights, which are rounded to fp32 once (half an ulp from the fp64 value; torch's fp32 weights are a few ulp from it, and at an exact tie — 175 -> 155,
// output 78: center - support + 0.5 = 88 exactly — torch's fp32 window gains a tap of weight 3e-6 that the formula excludes).  A tap inside the window whose
// weight is 0 stays a tap: 0 * NaN = NaN, as in torch.
// torch's nearest-exact kernel is this fp32 expression in its source and in its build without vector extensions; its AVX2 / AVX512 builds contract part of a
// row into a fused multiply-add and then differ from their own scalar lanes at exact ties (tests/test_preprocess_host.py has the count).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RSM_HD __host__ __device__ __forceinline__
#else
#define RSM_HD static inline
#endif

namespace rsm {

// bilinear taps of one output element at a downscale of at most kMaxScale: xmax - xmin <= 2 * support + 1
constexpr int kMaxScale = 8;
constexpr int kMaxTaps = 2 * kMaxScale + 1;

RSM_HD int nearest_index(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    const int s = (int)floorf(((float)dst + 0.5f) * scale);
    return s < in - 1 ? s : in - 1;
}

struct Window {
    int xmin, xsize;
};

RSM_HD Window aa_window(int i, int in, int out) {
    if (in == out) return Window{i, 1};
    const double scale = (double)in / (double)out;
    const double support = scale >= 1.0 ? scale : 1.0;
    const double center = scale * ((double)i + 0.5);
    int xmin = (int)(center - support + 0.5);          // (truncation, as Python's int(); the argument is > -1)
    int xmax = (int)(center + support + 0.5);
    xmin = xmin > 0 ? xmin : 0;
    xmax = xmax < in ? xmax : in;
    return Window{xmin, xmax - xmin};
}

// the un-normalised weight of tap j (an index of the input axis) of output element i
RSM_HD double aa_raw_weight(int i, int j, int in, int out) {
    if (in == out) return 1.0;
    const double scale = (double)in / (double)out;
    const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    const double center = scale * ((double)i + 0.5);
    const double w = 1.0 - fabs(((double)j - center + 0.5) * invscale);
    // a tap at the very edge of the support has weight 0 in exact arithmetic and a few 1e-15 of rounding noise here; through a mask (`resampled != 0`)
    // that noise would count as coverage.  1e-12 is far above the noise and far below anything an fp32 weight resolves.
    return w > 1e-12 ? w : 0.0;
}

// the normalised fp32 weights of window `win` of output element i, at most `cap` of them, into wt[0 .. n); returns n
RSM_HD int aa_weights(int i, int in, int out, Window win, float* wt, int cap) {
    const int n = win.xsize < cap ? win.xsize : cap;
    double total = 0.0;
    for (int k = 0; k < win.xsize; ++k) total += aa_raw_weight(i, win.xmin + k, in, out);
    for (int k = 0; k < n; ++k) {
        const double w = aa_raw_weight(i, win.xmin + k, in, out);
        wt[k] = (float)(total != 0.0 ? w / total : w);
    }
    return n;
}

}  // namespace rsm
