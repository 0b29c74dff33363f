// TEST INFRASTRUCTURE: host replay of the index and weight arithmetic of the frame resampler (mac-vo_amd/csrc/preprocess.hip).  It includes the kernels' own
// arithmetic header (csrc/resample_math.h) and calls the same functions, one output element after the other.  Built by tests/resample_twin.py with
// g++ -ffp-contract=off.  The product never builds or loads it.
//
// With -DRESAMPLE_TWIN_MAIN it is a plain stand-alone program (its own main) for a host-only -fsanitize=address,undefined run.
#include <vector>

#include "../../mac-vo_amd/csrc/resample_math.h"

// idx[out]: the nearest-exact source index of every output element
extern "C" void resample_twin_nearest(int in, int out, int32_t* idx) {
    for (int i = 0; i < out; ++i) idx[i] = rsm::nearest_index(i, in, out);
}

// xmin[out], xsize[out] and the normalised fp32 weights w[out][cap] (at most cap per element, the rest untouched) of the antialias filter
extern "C" void resample_twin_aa(int in, int out, int cap, int32_t* xmin, int32_t* xsize, float* w) {
    for (int i = 0; i < out; ++i) {
        const rsm::Window win = rsm::aa_window(i, in, out);
        xmin[i] = win.xmin, xsize[i] = win.xsize;
        rsm::aa_weights(i, in, out, win, w + (size_t)i * cap, cap);
    }
}

extern "C" int resample_twin_max_taps() { return rsm::kMaxTaps; }
extern "C" int resample_twin_max_scale() { return rsm::kMaxScale; }

#ifdef RESAMPLE_TWIN_MAIN
#include <stdio.h>
int main() {
    const int pairs[][2] = {{1241, 780}, {1920, 1137}, {37, 13}, {20, 33}, {240, 30}, {7, 7}, {1, 5}, {5, 1}};
    long taps = 0;
    for (const auto& p : pairs) {
        const int in = p[0], out = p[1], cap = rsm::kMaxTaps;
        std::vector<int32_t> idx(out), xmin(out), xsize(out);
        std::vector<float> w((size_t)out * cap, 0.f);
        resample_twin_nearest(in, out, idx.data());
        resample_twin_aa(in, out, cap, xmin.data(), xsize.data(), w.data());
        for (int i = 0; i < out; ++i) {
            if (idx[i] < 0 || idx[i] >= in || xmin[i] < 0 || xmin[i] + xsize[i] > in) return 1;
            taps += xsize[i];
        }
    }
    printf("resample_twin OK: %ld taps\n", taps);
    return 0;
}
#endif
