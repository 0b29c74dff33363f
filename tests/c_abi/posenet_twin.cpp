// TEST INFRASTRUCTURE: host replay of the PoseNet forward (mac-vo_amd/csrc/posenet.hip).  It includes the kernels' own plan header
// (posenet_math.h: layer table, packed layout, K split) and consumes the buffer mv_posenet_pack wrote, so packing, borders, strides and the
// reduction order are proven on the CPU: every output replays its fmaf chain per K range in ascending k — the padded zeros included —, adds
// the ranges in wave order, then the identity, then ReLU.  g++ -O2 -ffp-contract=off; the product path never builds or loads it.
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "posenet_math.h"

using namespace posenet;

static void conv_twin(const Conv& c, const float* pk, int lanes, const float* x, const float* x2, const float* res, float* y) {
    const int KS = CFG_KS[c.cfg], P = c.hout * c.wout;
    const int chw = c.hin * c.win, chw2 = c.ds_hin * c.ds_win;
    std::vector<const float*> src((size_t)c.K4 * 4);   // per k: the input value's address for one pixel, or null (border / padded channel)
    for (int lane = 0; lane < lanes; ++lane)
        for (int p = 0; p < P; ++p) {
            const int oy = p / c.wout, ox = p - oy * c.wout;
            for (int k4 = 0; k4 < c.K4; ++k4)
                for (int kq = 0; kq < 4; ++kq) {
                    int tap, ch;
                    k_source(c, k4, kq, tap, ch);
                    const float* s = nullptr;
                    if (tap < 9) {
                        const int iy = oy * c.stride - 1 + tap / 3, ix = ox * c.stride - 1 + tap % 3;
                        if (ch < c.cin && iy >= 0 && iy < c.hin && ix >= 0 && ix < c.win)
                            s = x + ((size_t)lane * c.cin + ch) * chw + iy * c.win + ix;
                    } else {
                        s = x2 + ((size_t)lane * c.ds_cin + ch) * chw2 + 2 * oy * c.ds_win + 2 * ox;
                    }
                    src[(size_t)k4 * 4 + kq] = s;
                }
            for (int n = 0; n < c.cout; ++n) {
                float total = 0.f;
                for (int w = 0; w < KS; ++w) {
                    float acc = w == 0 ? pk[c.b_off + n] : 0.f;
                    for (int k4 = split_begin(c.K4, KS, w); k4 < split_begin(c.K4, KS, w + 1); ++k4)
                        for (int kq = 0; kq < 4; ++kq) {
                            const float* s = src[(size_t)k4 * 4 + kq];
                            acc = fmaf(s ? *s : 0.f, pk[packed_w_index(c, n, k4, kq)], acc);
                        }
                    total = w == 0 ? acc : total + acc;
                }
                const size_t idx = ((size_t)lane * c.cout + n) * P + p;
                if (res) total += res[idx];
                y[idx] = relu(total);
            }
        }
}

// packed: the mv_posenet_pack buffer; x [lanes,5,112,160]; out [lanes,6]; stages: six buffers (NCHW per lane) or null entries
extern "C" int posenet_twin_forward(const float* pk, const float* x, int lanes, float* out, float* const* stages) {
    static Plan plan;
    if (!build_plan(plan)) return 1;
    std::vector<float> store[3];
    for (int b = 0; b < 3; ++b) store[b].resize((size_t)lanes * BUF_FLOATS[b]);
    float* buf[3] = {store[0].data(), store[1].data(), store[2].data()};
    int last = 0;
    for (int ci = 0; ci < N_CONVS; ++ci) {
        const Conv& c = plan.convs[ci];
        conv_twin(c, pk, lanes, c.src < 0 ? x : buf[c.src], c.ds_cin ? buf[c.res] : nullptr, c.residual ? buf[c.res] : nullptr, buf[c.dst]);
        if (c.stage >= 0 && stages && stages[c.stage])
            memcpy(stages[c.stage], buf[c.dst], sizeof(float) * lanes * c.cout * c.hout * c.wout);
        last = c.dst;
    }
    const Head& h = plan.head;
    for (int lane = 0; lane < lanes; ++lane) {
        const float* f = buf[last] + (size_t)lane * FEAT;
        float h1[2 * FC1], h2[2 * FC2];
        for (int j = 0; j < 2 * FC1; ++j) {
            float total = 0.f;
            for (int q = 0; q < HEAD_KS; ++q) {
                float s = q == 0 ? pk[h.b1 + j] : 0.f;
                for (int k = q * (FEAT / HEAD_KS); k < (q + 1) * (FEAT / HEAD_KS); ++k) s = fmaf(f[k], pk[h.w1 + (size_t)k * (2 * FC1) + j], s);
                total = q == 0 ? s : total + s;
            }
            h1[j] = relu(total);
        }
        for (int j = 0; j < 2 * FC2; ++j) {
            float s = pk[h.b2 + j];
            for (int k = 0; k < FC1; ++k) s = fmaf(h1[(j >> 5) * FC1 + k], pk[h.w2 + k * (2 * FC2) + j], s);
            h2[j] = relu(s);
        }
        for (int j = 0; j < 2 * FC3; ++j) {
            float s = pk[h.b3 + j];
            for (int k = 0; k < FC2; ++k) s = fmaf(h2[(j / FC3) * FC2 + k], pk[h.w3 + k * 8 + j], s);
            out[(size_t)lane * OUT_N + j] = s;
        }
    }
    return 0;
}
