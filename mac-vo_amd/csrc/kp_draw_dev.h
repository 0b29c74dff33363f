// RandomSelector and GridSelector (Module/KeypointSelector.py:103-118, 216-247) — the two selectors that look at no map at all.
//
// RandomSelector: `h = torch.randint(mask, H - mask, (k, 1)); w = torch.randint(mask, W - mask, (k, 1)); cat([w, h], 1)`.  On the CPU generator
// (the generator this project pins, randperm_dev.h) ATen's random_from_to draws ONE 32-bit MT19937 word per element, in order, and maps it with
// `word % (high - low) + low` (range < 2^32).  A call therefore consumes exactly 2 k words: words [0, k) are the rows' v, words [k, 2k) their u.
// Duplicates are possible and kept.  A following torch.randperm continues in the same word stream.
// With pos <= 624 the 2 k <= 1024 words of a call lie in the stored block and at most two stepped ones ("three blocks").
//
// GridSelector: closed-form integer arithmetic; the row count follows from (H, W, mask, numPoint) and may EXCEED numPoint
// (640 x 480, mask 32, numPoint 200 -> 11 x 21 = 231).
//
// Written as PHASES like randperm_dev.h: all threads of a workgroup (tid, nt) between barriers on the device, a loop over tid on the host
// (mv_kp_random_emulated).
#pragma once
#include "randperm_dev.h"

namespace mvkp {

constexpr int MAX_POINT = 512;              // rows per call the device draw covers
constexpr int MAX_WORDS = 2 * MAX_POINT;

struct Scratch {   // LDS on the device (9 KB)
    uint32_t mt[2][mvrp::MT_N];
    uint32_t w[MAX_WORDS];
};

struct Plan {
    int k, words, pos, steps, pos_out;   // block steps the call needs; position of the next draw in the last block afterwards (1 .. 624)
};
MV_RP_FN Plan plan_of(int k, int pos) {
    Plan p;
    p.k = k;
    p.words = 2 * k;
    p.pos = pos;
    p.steps = p.words > 0 ? (pos + p.words - 1) / mvrp::MT_N : 0;
    p.pos_out = pos + p.words - mvrp::MT_N * p.steps;
    return p;
}

// the call's words that lie in block `blk` (0 = the stored block, x = that block's 624 words)
MV_RP_FN void phase_words(const uint32_t* x, int blk, const Plan& pl, uint32_t* w, int tid, int nt) {
    const int base = blk * mvrp::MT_N - pl.pos;   // word index of the block's first word
    const int lo = base > 0 ? base : 0;
    const int hi = base + mvrp::MT_N < pl.words ? base + mvrp::MT_N : pl.words;
    for (int i = lo + tid; i < hi; i += nt) w[i] = mvrp::mt_temper(x[i - base]);
}

MV_RP_FN void row_of(const uint32_t* w, int k, int n, int H, int W, int mask, int& u, int& v) {
    v = (int)(w[n] % (uint32_t)(H - 2 * mask)) + mask;
    u = (int)(w[k + n] % (uint32_t)(W - 2 * mask)) + mask;
}

template <typename T>
MV_RP_FN void phase_rows(const uint32_t* w, int k, int H, int W, int mask, T* out_uv, int tid, int nt) {
    for (int n = tid; n < k; n += nt) {
        int u, v;
        row_of(w, k, n, H, W, mask, u, v);
        out_uv[2 * n] = (T)u;
        out_uv[2 * n + 1] = (T)v;
    }
}

// ---- grid ------------------------------------------------------------------------------------------------------------------------------
struct Grid {
    int cols, rows, sh, sw, mask;   // row i: u = (i % cols) * sw + mask, v = (i / cols) * sh + mask
};
// count 0 where the reference raises (a step of 0) or the masked image is empty
inline int grid_of(int H, int W, int mask, int num_point, Grid* g) {
    if (H <= 0 || W <= 0 || mask < 0 || num_point < 0 || H <= 2 * mask || W <= 2 * mask) return 0;
    const int h = H - 2 * mask, w = W - 2 * mask;
    int unit = 1;
    while ((long long)(unit + 1) * (unit + 1) <= num_point / 2) ++unit;   // max(1, int(sqrt(numPoint // 2)))
    const int sh = h / unit, sw = w / (2 * unit);
    if (sh == 0 || sw == 0) return 0;
    const int rows = (h + sh - 1) / sh, cols = (w + sw - 1) / sw;
    const long long n = (long long)rows * cols;
    if (n > 0x7fffffffLL) return 0;
    if (g) *g = Grid{cols, rows, sh, sw, mask};
    return (int)n;
}
MV_RP_FN void grid_row(const Grid& g, int i, int& u, int& v) {
    const int r = i / g.cols, c = i - r * g.cols;
    u = c * g.sw + g.mask;
    v = r * g.sh + g.mask;
}

}  // namespace mvkp

#if defined(__HIPCC__)
// One call of one lane's generator by one workgroup (all threads must call; every argument uniform): fills s.w[0 .. 2k) and, with state_out, stores
// the advanced generator (state_out == state_in is allowed when this is the only workgroup of the call).  Ends with a barrier: s.w is readable.
__device__ __forceinline__ void mv_kp_random_wg(const uint32_t* __restrict__ state_in, uint32_t* state_out, int k, mvkp::Scratch& s) {
    using namespace mvkp;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < mvrp::MT_N; i += nt) s.mt[0][i] = state_in[i];
    const Plan pl = plan_of(k, (int)state_in[mvrp::MT_N]);
    __syncthreads();
    int cur = 0;
    for (int blk = 0; blk <= pl.steps; ++blk) {   // (uniform)
        if (blk > 0) {
            mvrp::phase_step(s.mt[cur], s.mt[cur ^ 1], tid, nt);
            __syncthreads();
            cur ^= 1;
        }
        phase_words(s.mt[cur], blk, pl, s.w, tid, nt);
    }
    if (state_out) {
        for (int i = tid; i < mvrp::MT_N; i += nt) state_out[i] = s.mt[cur][i];
        if (tid == 0) state_out[mvrp::MT_N] = (uint32_t)pl.pos_out;
    }
    __syncthreads();
}
#endif
