// TEST INFRASTRUCTURE: host twin of the image-gradient selector kernels (mac-vo_amd/csrc/kp_gradient.hip).  It includes the kernels' own arithmetic
// header (kp_grad_math.h) and replays, thread for thread, the per-pixel gradient, the fixed-order fp64 reduction with the kernels' tile geometry (thread,
// wave butterfly, tile, ascending tiles), the statistics and the selection.  Built by tests/kp_grad_twin.py with g++ -ffp-contract=off.
// With -DKP_GRAD_TWIN_MAIN it is a plain stand-alone program (its own main) for a host-only -fsanitize=address,undefined run.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "../../mac-vo_amd/csrc/kp_grad_math.h"

using namespace mvkg;

static float px(const float* plane, int H, int W, int x, int y) { return (x >= 0 && x < W && y >= 0 && y < H) ? plane[(size_t)y * W + x] : 0.f; }

// image [3, H, W]; grad [H * W]; out_cand [H * W] (v * W + u, row-major); out_count [2] = {candidates, above the threshold inside the border};
// out_stats [3] = {mean, std, thr}; sums [2] = the image's fp64 (sum g, sum g^2)
extern "C" int kp_grad_twin(const float* image, int H, int W, int mask_width, int nms_size, float grad_std, float* grad, int32_t* out_cand, int32_t* out_count,
                            float* out_stats, double* sums) {
    if (!image || !grad || !out_cand || !out_count || !out_stats || H <= 0 || W <= 0 || nms_size < 0 || (nms_size && !(nms_size & 1)) ||
        nms_size > 2 * MAX_R + 1)
        return -1;
    const size_t plane = (size_t)H * W;
    const int tiles_x = (W + TILE_W - 1) / TILE_W, tiles_y = (H + TILE_H - 1) / TILE_H;
    Sums total{0.0, 0.0};
    for (int by = 0; by < tiles_y; ++by)
        for (int bx = 0; bx < tiles_x; ++bx) {   // ascending tile index
            Sums wave[WAVES];
            for (int ty = 0; ty < WAVES; ++ty) {
                Sums lane[64];
                for (int tx = 0; tx < 64; ++tx) {
                    Sums acc{0.0, 0.0};
                    const int gx = bx * TILE_W + tx;
                    for (int it = 0; it < PX_PER_THREAD; ++it) {
                        const int gy = by * TILE_H + ty * PX_PER_THREAD + it;
                        if (gx < W && gy < H) {
                            float l[3];
                            for (int c = 0; c < 3; ++c) {
                                const float* p = image + c * plane;
                                l[c] = laplace(px(p, H, W, gx, gy), px(p, H, W, gx, gy - 1), px(p, H, W, gx, gy + 1), px(p, H, W, gx - 1, gy), px(p, H, W, gx + 1, gy));
                            }
                            const float g = grad_of(l[0], l[1], l[2]);
                            grad[(size_t)gy * W + gx] = g;
                            accumulate(acc, g);
                        }
                    }
                    lane[tx] = acc;
                }
                for (int o = 32; o > 0; o >>= 1) {   // the xor butterfly: every lane adds its partner's value of the previous round
                    Sums nxt[64];
                    for (int i = 0; i < 64; ++i) nxt[i] = add(lane[i], lane[i ^ o]);
                    for (int i = 0; i < 64; ++i) lane[i] = nxt[i];
                }
                wave[ty] = lane[0];
            }
            total = add(total, add(add(add(wave[0], wave[1]), wave[2]), wave[3]));
        }
    const Stats st = stats_of(total, (int64_t)H * W, grad_std);
    out_stats[0] = st.mean;
    out_stats[1] = st.std;
    out_stats[2] = st.thr;
    if (sums) {
        sums[0] = total.s;
        sums[1] = total.s2;
    }
    const int r = nms_size >> 1;
    int n = 0, above_n = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const float g = grad[(size_t)y * W + x];
            const bool above = g > st.thr && in_border(x, y, W, H, mask_width);
            if (!above) continue;
            ++above_n;
            float m = g;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const int sx = x + dx, sy = y + dy;
                    if (sx < 0 || sx >= W || sy < 0 || sy >= H) continue;   // -inf padding: never the maximum
                    const float o = grad[(size_t)sy * W + sx];
                    m = o > m ? o : m;
                }
            if (g == m) out_cand[n++] = y * W + x;
        }
    out_count[0] = n;
    out_count[1] = above_n;
    return 0;
}

#ifdef KP_GRAD_TWIN_MAIN
#include <stdio.h>
// one image of H x W (values are multiples of 1 / 256) through every window size with no border, a border of 4 and one of m_all >= min(H, W) / 2;
// 0: consistent, the candidates added to *total and the last threshold left in *thr
static int check_shape(int H, int W, int m_all, int* total, float* thr) {
    std::vector<float> img((size_t)3 * H * W), grad((size_t)H * W);
    uint32_t s = 12345u;
    for (auto& v : img) {
        s = s * 1664525u + 1013904223u;
        v = (float)(s >> 24) / 256.f;
    }
    std::vector<int32_t> cand((size_t)H * W);
    int32_t count[2];
    float stats[3];
    double sums[2];
    if (2 * m_all < H && 2 * m_all < W) return 5;
    for (int nms : {0, 1, 3, 15})
        for (int m : {0, 4, m_all}) {
            if (kp_grad_twin(img.data(), H, W, m, nms, 1.f, grad.data(), cand.data(), count, stats, sums) != 0) return 1;
            if (count[0] < 0 || count[0] > count[1] || count[1] > H * W) return 2;
            if ((m == 0 || m == m_all) && count[0] != 0) return 3;
            if (m == 4 && nms == 0 && (count[0] == 0 || count[0] != count[1])) return 6;
            for (int i = 0; i < count[0]; ++i)
                if (cand[i] < 0 || cand[i] >= H * W || (i && cand[i] <= cand[i - 1])) return 7;   // row-major, ascending, inside the image
            *total += count[0];
        }
    if (kp_grad_twin(img.data(), H, W, 4, 2, 1.f, grad.data(), cand.data(), count, stats, sums) != -1) return 4;
    *thr = stats[2];
    return 0;
}

int main() {
    // 37 x 131: odd sizes, ragged tiles in both directions, more than one tile each way.  130 x 513: more than 1024 candidate words (two per compaction
    // thread, a row's last word of one pixel).  3841 x 65: 482 tiles, more than one chunk of the kernels' tile sum, a last tile row of one pixel.
    int total = 0;
    float thr = 0.f, thr_first = 0.f;
    const int shapes[3][3] = {{37, 131, 20}, {130, 513, 65}, {3841, 65, 33}};
    for (int i = 0; i < 3; ++i) {
        const int rc = check_shape(shapes[i][0], shapes[i][1], shapes[i][2], &total, &thr);
        if (rc) return 10 * (i + 1) + rc;
        if (i == 0) thr_first = thr;
    }
    printf("kp_grad_twin OK %d %.6f %.6f\n", total, (double)thr_first, (double)thr);
    return 0;
}
#endif
