// GradientSelector / SparseGradienSelector — the image-gradient keypoint selectors (Module/KeypointSelector.py:121-158, :161-213) on the GPU.
//
// Replaces, per frame, a CPU conv2d / mean / std / max_pool2d / nonzero over the full image, a host randperm and a host-to-device copy of the rows.
// The arithmetic contract (what is rounded where, the fixed order of the fp64 sums) is kp_grad_math.h, shared with the host twin.
//
// gfx950 design: ~6 MB of traffic per 480 x 640 frame (three planes in, the gradient plane out and back), a few us of HBM time — the path is bound by
// its launches, so: few launches, no atomics, no host synchronisation.  Lanes are independent frames of one launch (blockIdx.z / one workgroup each).
//   kg_grad_kernel     one 256-thread workgroup per 64 x 16 tile: the three planes + a 1-pixel halo are loaded coalesced (every global load of a thread
//                      in flight before the first LDS store) and staged in LDS; |Laplacian| per pixel -> the workspace plane `grad`; the tile's fp64
//                      (sum g, sum g^2) pair -> one slot per tile (plain stores: no floating-point atomics, the order of the sums is fixed).
//   kg_select_kernel   same grid: every workgroup adds the tile pairs in ascending tile index (a few hundred fp64 pairs out of L2, staged through LDS)
//                      and derives thr; the lane's first workgroup stores the statistics.  Threshold, border mask and — nms_size > 1 — the window
//                      maximum (separable, from an LDS tile of `grad` with an nms_size / 2 halo, -inf outside the image as max_pool2d pads) give one
//                      64-pixel candidate word per tile row (the words of kp_select.hip) and one word of the pixels above the threshold.
//   kg_compact_kernel  one 1024-thread workgroup per lane: popcounts -> workgroup scan -> the set bits in row-major order as v * W + u.
//   kp_finish_device_kernel  one workgroup per lane: torch.randperm(n)[:k] from the lane's device-resident MT19937 (randperm_dev.h), n read from
//                      device memory, the (u, v) rows gathered from the candidate list, rows past min(n, k) zeroed.
#include "common.h"
#include "kp_grad_math.h"
#include "kp_scan_dev.h"
#include "randperm_dev.h"

namespace {

using namespace mvkg;

struct GradWs {
    float* grad;                     // [H, W]
    unsigned long long* cand_bits;   // [H, words_per_row]  candidates
    unsigned long long* above_bits;  // [H, words_per_row]  grad > thr inside the border, before the NMS
    Sums* tile_sums;                 // [tiles]
    size_t lane_bytes;

    __device__ __forceinline__ GradWs lane(int l) const {
        const size_t o = (size_t)l * lane_bytes;
        return GradWs{(float*)((char*)grad + o), (unsigned long long*)((char*)cand_bits + o), (unsigned long long*)((char*)above_bits + o),
                      (Sums*)((char*)tile_sums + o), lane_bytes};
    }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

__global__ __launch_bounds__(256) void kg_grad_kernel(const float* __restrict__ image, GradWs ws_all, int H, int W) {
    constexpr int SW = TILE_W + 2, SH = TILE_H + 2, NE = 3 * SW * SH, NST = (NE + 255) / 256;
    __shared__ float t[3][SH][SW];
    __shared__ Sums wave_sums[WAVES];
    const GradWs ws = ws_all.lane(blockIdx.z);
    const size_t plane = (size_t)H * W;
    image += (size_t)blockIdx.z * 3 * plane;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;

    float v[NST];
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int e = i * 256 + tid;
        const int c = e / (SW * SH), rem = e - c * (SW * SH);
        const int ly = rem / SW, lx = rem - ly * SW;
        const int gx = x0 + lx - 1, gy = y0 + ly - 1;
        float val = 0.f;   // conv2d(padding = 1): zeros outside the image
        if (e < NE && gx >= 0 && gx < W && gy >= 0 && gy < H) val = image[(size_t)c * plane + (size_t)gy * W + gx];
        v[i] = val;
    }
#pragma unroll
    for (int i = 0; i < NST; ++i) {
        const int e = i * 256 + tid;
        if (e < NE) (&t[0][0][0])[e] = v[i];
    }
    __syncthreads();

    Sums acc{0.0, 0.0};
    const int gx = x0 + tx;
#pragma unroll
    for (int it = 0; it < PX_PER_THREAD; ++it) {
        const int ly = ty * PX_PER_THREAD + it, gy = y0 + ly;
        if (gx < W && gy < H) {
            float l[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) l[c] = laplace(t[c][ly + 1][tx + 1], t[c][ly][tx + 1], t[c][ly + 2][tx + 1], t[c][ly + 1][tx], t[c][ly + 1][tx + 2]);
            const float g = grad_of(l[0], l[1], l[2]);
            ws.grad[(size_t)gy * W + gx] = g;
            accumulate(acc, g);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {   // the butterfly of kp_grad_math.h
        acc.s += __shfl_xor(acc.s, o, 64);
        acc.s2 += __shfl_xor(acc.s2, o, 64);
    }
    if (tx == 0) wave_sums[ty] = acc;
    __syncthreads();
    if (tid == 0) ws.tile_sums[blockIdx.y * gridDim.x + blockIdx.x] = add(add(add(wave_sums[0], wave_sums[1]), wave_sums[2]), wave_sums[3]);
}

__global__ __launch_bounds__(256) void kg_select_kernel(GradWs ws_all, mvKpGradParams p, int words_per_row, float* __restrict__ out_stats) {
    __shared__ float tile[TILE_H + 2 * MAX_R][TILE_W + 2 * MAX_R + 1];
    __shared__ __align__(16) float hmax[TILE_H + 2 * MAX_R][TILE_W + 1];
    const GradWs ws = ws_all.lane(blockIdx.z);
    const int H = p.H, W = p.W;
    const int r = p.nms_size >> 1;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * 64 + tx;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const float* __restrict__ grad = ws.grad;

    // the image's sums: the tile pairs in ascending tile index, the same chain in every workgroup
    const int n_tiles = gridDim.x * gridDim.y;
    const Sums* __restrict__ ts = ws.tile_sums;
    // (staged through LDS — the row buffer of the NMS below, not yet in use — in chunks: the loads of a chunk are in flight together and the dependent
    // chain is the fp64 additions alone; read one by one from global memory the chain paid a memory latency per pair, 30 us for 300 pairs)
    constexpr int CHUNK = 480;
    static_assert(sizeof(hmax) >= CHUNK * sizeof(Sums), "the tile pairs are staged in hmax");
    Sums* const stage = reinterpret_cast<Sums*>(&hmax[0][0]);
    Sums tot{0.0, 0.0};
    for (int base = 0; base < n_tiles; base += CHUNK) {   // (uniform)
        const int cnt = min(CHUNK, n_tiles - base);
        for (int i = tid; i < cnt; i += 256) stage[i] = ts[base + i];
        __syncthreads();
        for (int i = 0; i < cnt; ++i) tot = add(tot, stage[i]);
        __syncthreads();
    }
    const Stats st = stats_of(tot, (int64_t)H * W, p.grad_std);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        float* o = out_stats + 4 * blockIdx.z;
        o[0] = st.mean;
        o[1] = st.std;
        o[2] = st.thr;
        o[3] = 0.f;
    }

    const int gx = x0 + tx;
    float gpx[PX_PER_THREAD], wmax[PX_PER_THREAD];
    if (r > 0) {
        const int tw = TILE_W + 2 * r, th = TILE_H + 2 * r;
        constexpr int NST = ((TILE_W + 2 * MAX_R) * (TILE_H + 2 * MAX_R) + 255) / 256;
        float qv[NST];
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            const int ly = e / tw, lx = e - ly * tw;
            const int sx = x0 + lx - r, sy = y0 + ly - r;
            float q = -INFINITY;   // max_pool2d pads with -inf: never the maximum
            if (e < tw * th && sx >= 0 && sx < W && sy >= 0 && sy < H) q = grad[(size_t)sy * W + sx];
            qv[i] = q;
        }
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = i * 256 + tid;
            const int ly = e / tw, lx = e - ly * tw;
            if (e < tw * th) tile[ly][lx] = qv[i];
        }
        __syncthreads();
        for (int e = tid; e < th * TILE_W; e += 256) {
            const int ly = e >> 6, lx = e & 63;
            float m = tile[ly][lx];
            for (int dx = 1; dx <= 2 * r; ++dx) {
                const float o = tile[ly][lx + dx];
                m = o > m ? o : m;
            }
            hmax[ly][lx] = m;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < PX_PER_THREAD; ++it) {
            const int ly = ty * PX_PER_THREAD + it;
            gpx[it] = tile[ly + r][tx + r];
            float m = hmax[ly][tx];
            for (int dy = 1; dy <= 2 * r; ++dy) {
                const float o = hmax[ly + dy][tx];
                m = o > m ? o : m;
            }
            wmax[it] = m;
        }
    } else {
#pragma unroll
        for (int it = 0; it < PX_PER_THREAD; ++it) {
            const int gy = y0 + ty * PX_PER_THREAD + it;
            gpx[it] = (gx < W && gy < H) ? grad[(size_t)gy * W + gx] : 0.f;
            wmax[it] = gpx[it];
        }
    }
#pragma unroll
    for (int it = 0; it < PX_PER_THREAD; ++it) {
        const int gy = y0 + ty * PX_PER_THREAD + it;
        const bool above = gx < W && gy < H && gpx[it] > st.thr && in_border(gx, gy, W, H, p.mask_width);   // strict, false for a NaN thr
        const bool cand = above && gpx[it] == wmax[it];                                                      // every tied maximum survives
        const unsigned long long above_word = __ballot(above), cand_word = __ballot(cand);
        if (tx == 0 && gy < H) {
            ws.cand_bits[(size_t)gy * words_per_row + blockIdx.x] = cand_word;
            ws.above_bits[(size_t)gy * words_per_row + blockIdx.x] = above_word;
        }
    }
}

constexpr int COMPACT_NT = 1024;

__global__ __launch_bounds__(COMPACT_NT) void kg_compact_kernel(GradWs ws_all, int H, int W, int words_per_row, int32_t* __restrict__ out_cand,
                                                                int32_t* __restrict__ out_count) {
    __shared__ int wave_tot[COMPACT_NT / 64];
    const GradWs ws = ws_all.lane(blockIdx.x);
    out_cand += (size_t)blockIdx.x * H * W;
    out_count += 4 * blockIdx.x;
    const int tid = threadIdx.x;
    const int n_words = H * words_per_row;
    const int per = (n_words + COMPACT_NT - 1) / COMPACT_NT;   // thread t owns the contiguous words [t * per, (t + 1) * per)
    const int w_begin = min(tid * per, n_words), w_end = min(w_begin + per, n_words);
    int cnt = 0, above = 0;
    for (int w = w_begin; w < w_end; ++w) {
        cnt += __popcll(ws.cand_bits[w]);
        above += __popcll(ws.above_bits[w]);
    }
    int total, total_above;
    int pos = block_exclusive_scan<COMPACT_NT>(cnt, wave_tot, total);
    block_exclusive_scan<COMPACT_NT>(above, wave_tot, total_above);
    for (int w = w_begin; w < w_end; ++w) {
        unsigned long long bits = ws.cand_bits[w];
        const int row = w / words_per_row, col0 = (w - row * words_per_row) * 64;
        while (bits) {
            const int b = __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            out_cand[pos++] = row * W + col0 + b;
        }
    }
    if (tid == 0) {
        out_count[0] = total;
        out_count[1] = total_above;
        out_count[2] = 0;
        out_count[3] = 0;
    }
}

__global__ __launch_bounds__(1024) void kp_finish_device_kernel(uint32_t* __restrict__ state, const int32_t* __restrict__ cand, size_t cand_lane_stride,
                                                                const int32_t* __restrict__ count_dev, int count_stride, int k, int cap, int W,
                                                                int64_t* __restrict__ out_uv, int32_t* __restrict__ out_n_sel) {
    __shared__ mvrp::Scratch s;
    __shared__ int32_t head[mvrp::NBUCKET];
    __shared__ int32_t perm[mvrp::MAX_HEAD];
    const int l = blockIdx.x;
    uint32_t* const st = state + (size_t)l * mvrp::MT_STRIDE;
    cand += (size_t)l * cand_lane_stride;
    out_uv += 2 * (size_t)l * cap;
    int64_t n = count_dev[(size_t)l * count_stride];
    n = n < 0 ? 0 : (n > (int64_t)cand_lane_stride ? (int64_t)cand_lane_stride : n);   // never an index outside the lane's list
    const int m = mv_randperm_head_wg(st, st, n, k, perm, s, head);
    __syncthreads();
    for (int i = threadIdx.x; i < cap; i += blockDim.x) {
        int64_t u = 0, v = 0;
        if (i < m) {
            const int lin = cand[perm[i]];
            u = lin % W;
            v = lin / W;
        }
        out_uv[2 * i + 0] = u;
        out_uv[2 * i + 1] = v;
    }
    if (threadIdx.x == 0) out_n_sel[l] = m;
}

}  // namespace

extern "C" size_t mv_kp_gradient_workspace_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    const size_t words = (size_t)H * mv_ceil_div(W, 64);
    const size_t tiles = (size_t)mv_ceil_div(H, TILE_H) * mv_ceil_div(W, TILE_W);
    return align_up((size_t)H * W * 4, 256) + 2 * align_up(words * 8, 256) + align_up(tiles * sizeof(Sums), 256);
}

extern "C" int mv_kp_gradient_lanes(const float* image, const mvKpGradParams* params, void* workspace, size_t workspace_bytes, int32_t* out_cand,
                                    int32_t* out_count, float* out_stats, int lanes, mvStream_t stream) {
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES);
    MV_CHECK_ARG(image && params && workspace && out_cand && out_count && out_stats);
    const mvKpGradParams p = *params;
    MV_CHECK_ARG(p.H > 0 && p.W > 0 && p.mask_width >= 0 && p.grad_std > 0.f);   // (a NaN grad_std fails the compare)
    MV_CHECK_ARG((int64_t)p.H * p.W < ((int64_t)1 << 31) && mv_ceil_div(p.H, TILE_H) <= 65535);
    MV_CHECK_ARG(p.nms_size >= 0 && (p.nms_size == 0 || (p.nms_size & 1)));
    if (p.nms_size > 2 * MAX_R + 1) return MV_ERR_UNSUPPORTED;
    const size_t lane_bytes = mv_kp_gradient_workspace_bytes(p.H, p.W);
    if (workspace_bytes < lane_bytes * (size_t)lanes) return MV_ERR_WORKSPACE;
    if (((uintptr_t)workspace & 7) != 0) return MV_ERR_INVALID_ARG;

    const int wpr = mv_ceil_div(p.W, 64);
    const size_t words = (size_t)p.H * wpr;
    char* base = (char*)workspace;
    GradWs ws;
    ws.grad = (float*)base;
    base += align_up((size_t)p.H * p.W * 4, 256);
    ws.cand_bits = (unsigned long long*)base;
    base += align_up(words * 8, 256);
    ws.above_bits = (unsigned long long*)base;
    base += align_up(words * 8, 256);
    ws.tile_sums = (Sums*)base;
    ws.lane_bytes = lane_bytes;

    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(wpr, mv_ceil_div(p.H, TILE_H), lanes), block(64, WAVES);
    hipLaunchKernelGGL(kg_grad_kernel, grid, block, 0, s, image, ws, p.H, p.W);
    hipLaunchKernelGGL(kg_select_kernel, grid, block, 0, s, ws, p, wpr, out_stats);
    hipLaunchKernelGGL(kg_compact_kernel, dim3(lanes), dim3(COMPACT_NT), 0, s, ws, p.H, p.W, wpr, out_cand, out_count);
    return mv_launch_status();
}

extern "C" int mv_kp_finish_device_lanes(uint32_t* state, const int32_t* cand, size_t cand_lane_stride, const int32_t* count_dev, int count_stride,
                                         int lanes, int k, int cap, int W, int64_t* out_uv, int32_t* out_n_sel, mvStream_t stream) {
    MV_CHECK_ARG(state && cand && count_dev && out_uv && out_n_sel);
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES && count_stride >= 1 && cand_lane_stride >= 1 && W > 0);
    MV_CHECK_ARG(k >= 0 && k <= cap && cap >= 1);
    if (k > mvrp::MAX_HEAD) return MV_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(kp_finish_device_kernel, dim3(lanes), dim3(1024), 0, (hipStream_t)stream, state, cand, cand_lane_stride, count_dev, count_stride, k,
                       cap, W, out_uv, out_n_sel);
    return mv_launch_status();
}
