// Frontend evaluation metrics (Evaluation/EvalFlow.py:29-47,82-127, Evaluation/EvalDepth.py:22-34,57-82, Utility/Extensions/GridRecorder.py:24-36):
// end-point / depth error, px-K rates, covariance NLL overall and within the 25 / 50 / 75 % most confident pixels, error^2-vs-variance grids.
//
// One lane = one frame.  Per call, on the caller's stream, nothing waits for the host:
//   memset            the lane's digit histograms, tickets and integer counters
//   eval_pixel_kernel per-pixel terms, masked sums (fp64 per-workgroup partials), counters, recorder grid (LDS-privatised), first radix digit
//   eval_select_kernel x 2   second and third digit of every rank the call needs (<= 6 per population, resolved together); the last one turns
//                     the order statistics into torch.nanquantile's values
//   eval_qmean_kernel NLL means under `uncertainty < threshold` (with a covariance)
// A kernel's last workgroup to arrive (a ticket from an integer atomic; nobody waits) scans the histograms / sums the partials in a fixed order and,
// in the call's last kernel, writes the row (ev_arrive: no cache-wide fence on either side).  Sums are fp64, reduced in an order that depends on
// (H, W) only: a lane's bits do not depend on the other lanes of the launch, nor on the run.  No floating-point atomics.  Everything a workgroup
// hands to the finishing one goes through agent-scope atomics (integer adds, 8-byte stores) and is read back with agent-scope atomic loads.
//
// Populations of the selects: 0 = `uncertainty` over ALL pixels of the lane (flow: cu * cv; depth: c), 1 = depth error inside the mask.  Keys are
// the sign-flipped fp32 bits (ascending order of the values; NaN is left out), digits 11 + 11 + 10 bits; keys are re-derived from the input planes
// in every pass instead of being stored.
#include "common.h"

namespace {

constexpr int EV_NT = 256;            // threads per workgroup (4 waves)
constexpr int EV_MAX_BLOCKS = 128;    // workgroups per lane: at H * W = 2^22 one handles 32768 pixels, so a 16-bit LDS grid counter cannot wrap
constexpr int EV_BINS = 2048;
constexpr int EV_SLOTS = 6;           // ranks per population: floor / ceil of three quantiles
constexpr int EV_POPS = 2;
constexpr int EV_GRID = 100;          // GridRecorder((0, 25, .25), ...) and ((0, 50, .5), ...) are both 100 x 100
constexpr int EV_GRID_WORDS = EV_GRID * EV_GRID / 2;   // two 16-bit counters per LDS word
constexpr int EV_CTRL_WORDS = 32;
constexpr int EV_PART = 4;            // fp64 partial columns per workgroup and kernel

// control words of a lane (zeroed per call)
enum { T_PIXEL = 0, T_SELECT = 1 /* + 2 * (pass - 1) + pop */, T_QMEAN = 5 };
enum { C_MASK = 8, C_MASK_FIN, C_FIN, C_PX1, C_PX3, C_PX5, C_MASK_NLL, C_NQ, C_CQ = C_NQ + 3, C_END = C_CQ + 3 };
static_assert(C_END <= EV_CTRL_WORDS, "control block");

struct EvSel {
    uint32_t n;                   // non-NaN members of the population
    uint32_t prefix[EV_SLOTS];    // key bits resolved so far
    uint32_t k[EV_SLOTS];         // rank among the keys that share the prefix
    uint32_t lead[EV_SLOTS];      // first slot with the same prefix: the one whose histogram is built
    uint32_t pad;
};

struct EvArgs {
    const float* est;     // flow [2, n] per lane; depth [n]
    const float* gt;
    const float* cov;     // flow: planes uu, vv (cov_ps apart); depth [n]; null = no covariance
    const uint8_t* valid; // flow only, nullable
    long long est_ls, gt_ls, cov_ls, cov_ps, valid_ls;
    float maxv;
    int apply_max, n, vec;
    float* rows;
    int rows_per_lane, row_index, ncols;
    uint32_t* grids;
    float *err_out, *nll_out;
    uint32_t* hist;       // [lanes][EV_POPS][EV_SLOTS][EV_BINS]
    uint32_t* ctrl;       // [lanes][EV_CTRL_WORDS]
    EvSel* state;         // [lanes][EV_POPS]
    float* thr;           // [lanes][EV_POPS][4]
    double *partA, *partB;   // [lanes][G][EV_PART]
};

__host__ __device__ inline int ev_blocks(int n) {
    const int g = (n + 4 * EV_NT - 1) / (4 * EV_NT);
    return g < 1 ? 1 : (g > EV_MAX_BLOCKS ? EV_MAX_BLOCKS : g);
}

__device__ __forceinline__ uint32_t ev_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ev_unkey(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ int ev_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int ev_nbins(int pass) { return pass == 2 ? 1024 : 2048; }

__device__ __forceinline__ uint32_t ev_ld(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ev_st(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ev_ldd(const double* p) {
    return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void ev_std(double* p, double v) {
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void ev_ld4(const float* p, int i0, int n, bool vec, float (&o)[4]) {
    if (vec && i0 + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(p + i0);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = i0 + k < n ? p[i0 + k] : 0.f;
    }
}
__device__ __forceinline__ void ev_st4(float* p, int i0, int n, bool vec, const float (&o)[4]) {
    if (vec && i0 + 4 <= n) {
        *reinterpret_cast<float4*>(p + i0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < n) p[i0 + k] = o[k];
    }
}

// what the metrics need of four consecutive pixels
struct EvQuad {
    float err[4];      // flow: end-point error; depth: |est - gt|
    float nll[4], unc[4];
    float e2a[4], ca[4], e2b[4], cb[4];   // recorder pairs (flow: u and v; depth: a only)
    bool mask[4];
};

template <bool FLOW>
__device__ __forceinline__ void ev_quad(const EvArgs& a, int lane, int i0, EvQuad& q) {
    const int n = a.n;
    const bool vec = a.vec != 0, has_cov = a.cov != nullptr;
    const float* est = a.est + (long long)lane * a.est_ls;
    const float* gt = a.gt + (long long)lane * a.gt_ls;
    const float* cov = has_cov ? a.cov + (long long)lane * a.cov_ls : nullptr;
    if constexpr (FLOW) {
        float ue[4], ve[4], ug[4], vg[4], cu[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0};
        uint8_t vm[4] = {1, 1, 1, 1};
        ev_ld4(est, i0, n, vec, ue);
        ev_ld4(est + n, i0, n, vec, ve);
        ev_ld4(gt, i0, n, vec, ug);
        ev_ld4(gt + n, i0, n, vec, vg);
        if (has_cov) {
            ev_ld4(cov, i0, n, vec, cu);
            ev_ld4(cov + a.cov_ps, i0, n, vec, cv);
        }
        if (a.valid) {
            const uint8_t* vp = a.valid + (long long)lane * a.valid_ls;
            if (vec && i0 + 4 <= n) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(vp + i0);
#pragma unroll
                for (int k = 0; k < 4; ++k) vm[k] = (uint8_t)(w >> (8 * k));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) vm[k] = i0 + k < n ? vp[i0 + k] : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float eu = ue[k] - ug[k], ev = ve[k] - vg[k];
            const float eu2 = eu * eu, ev2 = ev * ev;
            q.err[k] = sqrtf(eu2 + ev2);
            q.mask[k] = (!a.apply_max || (ue[k] < a.maxv && ve[k] < a.maxv)) && vm[k] != 0;
            const float det = cu[k] * cv[k];
            // Tensor.pinverse on diag(cu, cv): singular values below rcond * largest are dropped
            const float cut = 1e-15f * fmaxf(fabsf(cu[k]), fabsf(cv[k]));
            const float pu = fabsf(cu[k]) > cut ? 1.f / cu[k] : 0.f;
            const float pv = fabsf(cv[k]) > cut ? 1.f / cv[k] : 0.f;
            const float m = (eu * pu) * eu + (ev * pv) * ev;
            const float r = sqrtf(m);
            q.nll[k] = logf(det) + r * r;
            q.unc[k] = det;
            q.e2a[k] = eu2, q.ca[k] = cu[k], q.e2b[k] = ev2, q.cb[k] = cv[k];
        }
    } else {
        float de[4], dg[4], c[4] = {0, 0, 0, 0};
        ev_ld4(est, i0, n, vec, de);
        ev_ld4(gt, i0, n, vec, dg);
        if (has_cov) ev_ld4(cov, i0, n, vec, c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = de[k] - dg[k];
            q.err[k] = fabsf(e);
            q.mask[k] = de[k] < a.maxv;
            const float p = c[k] != 0.f ? 1.f / c[k] : 0.f;
            const float r = sqrtf((e * p) * e);
            q.nll[k] = logf(c[k]) + r * r;
            q.unc[k] = c[k];
            q.e2a[k] = e * e, q.ca[k] = c[k], q.e2b[k] = 0.f, q.cb[k] = 0.f;
        }
    }
}

// (int)(v * scale) as numpy's astype(int) bins it: truncation toward zero; NaN, +-inf and anything outside [0, 100) is not counted
__device__ __forceinline__ int ev_bin(float v, float scale) {
    const float s = v * scale;
    return (s > -1.f && s < (float)EV_GRID) ? (int)s : -1;
}

__device__ __forceinline__ double ev_block_sum(double v, double* s_red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return r;
}
// integer counters: wave sum -> the workgroup's LDS counters -> (ev_count_flush, after a barrier) one global atomic per counter and workgroup
__device__ __forceinline__ void ev_count(uint32_t* s_cnt, int which, int c) {
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(s_cnt + which, (uint32_t)c);
}
__device__ __forceinline__ void ev_count_flush(uint32_t* ctrl, const uint32_t* s_cnt) {
    if (threadIdx.x >= C_MASK && threadIdx.x < C_END) {
        const uint32_t c = s_cnt[threadIdx.x];
        if (c) atomicAdd(ctrl + threadIdx.x, c);
    }
}

// exclusive prefix of `v` over the workgroup's threads, and the total
__device__ __forceinline__ uint32_t ev_block_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (l >= o) inc += t;
    }
    if (l == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < w; ++i) base += s_w[i];
    total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    return base + inc - v;
}

// Arrive; true for the last workgroup of the lane.  Everything a workgroup hands over is an agent-scope atomic or an agent-scope atomic store
// (write-through): each wave waits until its own have been performed, the barrier collects the waves, then one lane takes the ticket.  The finishing
// workgroup reads what was handed over with agent-scope atomic loads only, which no cache of its own serves, so neither side needs a cache-wide
// release / acquire (a per-workgroup L2 write-back is what a full __threadfence() costs here).
__device__ __forceinline__ bool ev_arrive(uint32_t* ticket, int* s_last) {
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    __syncthreads();
    if (threadIdx.x == 0) *s_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    const bool last = *s_last != 0;
#ifdef __HIP_DEVICE_COMPILE__
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // keeps the finishing loads behind the ticket in program order
#endif
    return last;
}

// torch's fp32 quantile position: r = q * (n - 1), exact for n <= 2^22 and q in {1/4, 1/2, 3/4}
__device__ __forceinline__ void ev_ranks(uint32_t n, bool median_mid, uint32_t (&rk)[EV_SLOTS]) {
    const float nm1 = (float)(n ? n - 1 : 0);
    const float qs[3] = {0.25f, 0.5f, 0.75f};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float r = qs[i] * nm1;
        rk[2 * i] = (uint32_t)floorf(r);
        rk[2 * i + 1] = (uint32_t)ceilf(r);
    }
    if (median_mid) rk[2] = rk[3] = n ? (n - 1) / 2 : 0;   // nanmedian: the lower middle element
}
__device__ __forceinline__ float ev_lerp(float a, float b, float w) {
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.f - w);
}

// Last workgroup of a digit pass: per slot, the bin that holds its rank; new prefix / rank / leaders; after the third digit the quantile values.
// The lane's histograms are left zero for the next pass.
__device__ void ev_scan_pass(const EvArgs& a, int lane, int pop, int pass, uint32_t* s_w, uint32_t* s_res) {
    const int tid = threadIdx.x;
    EvSel* st = a.state + lane * EV_POPS + pop;
    uint32_t* H = a.hist + (size_t)(lane * EV_POPS + pop) * EV_SLOTS * EV_BINS;
    const bool median_mid = pop == 1;
    uint32_t n, rk[EV_SLOTS], lead[EV_SLOTS], pre[EV_SLOTS];
    if (pass == 0) {
        uint32_t s = 0;
        for (int b = 0; b < 8; ++b) s += ev_ld(H + tid * 8 + b);
        ev_block_scan(s, s_w, n);
        ev_ranks(n, median_mid, rk);
        for (int j = 0; j < EV_SLOTS; ++j) lead[j] = 0, pre[j] = 0;
    } else {
        n = st->n;
        for (int j = 0; j < EV_SLOTS; ++j) rk[j] = st->k[j], lead[j] = st->lead[j], pre[j] = st->prefix[j];
    }
    if (tid < 2 * EV_SLOTS) s_res[tid] = 0;
    __syncthreads();
    // every slot's eight bins first (one memory round trip for the lot; a slot that shares its leader with the one before it copies), then the scans
    uint32_t c[EV_SLOTS][8];
#pragma unroll
    for (int j = 0; j < EV_SLOTS; ++j) {
        if (j > 0 && lead[j] == lead[j - 1]) {
#pragma unroll
            for (int b = 0; b < 8; ++b) c[j][b] = c[j - 1][b];
        } else {
            const uint32_t* Hj = H + lead[j] * EV_BINS;
#pragma unroll
            for (int b = 0; b < 8; ++b) c[j][b] = ev_ld(Hj + tid * 8 + b);
        }
    }
#pragma unroll
    for (int j = 0; j < EV_SLOTS; ++j) {
        uint32_t s = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) s += c[j][b];
        uint32_t tot;
        uint32_t ex = ev_block_scan(s, s_w, tot);
        if (n && rk[j] >= ex && rk[j] < ex + s) {
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (rk[j] >= ex && rk[j] < ex + c[j][b]) {
                    s_res[j] = tid * 8 + b;
                    s_res[EV_SLOTS + j] = rk[j] - ex;
                }
                ex += c[j][b];
            }
        }
    }
    __syncthreads();
    const int bits = pass == 2 ? 10 : 11;
    for (int j = 0; j < EV_SLOTS; ++j) pre[j] = (pre[j] << bits) | s_res[j];
    // zero what this pass built
    for (int j = 0; j < EV_SLOTS; ++j)
        if (lead[j] == (uint32_t)j)
            for (int b = 0; b < 8; ++b) ev_st(H + j * EV_BINS + tid * 8 + b, 0u);
    if (tid == 0) {
        st->n = n;
        for (int j = 0; j < EV_SLOTS; ++j) {
            st->prefix[j] = pre[j];
            st->k[j] = s_res[EV_SLOTS + j];
            int l = j;
            for (int i = j - 1; i >= 0; --i)
                if (pre[i] == pre[j]) l = i;
            st->lead[j] = (uint32_t)l;
        }
        if (pass == 2) {
            float* t = a.thr + (lane * EV_POPS + pop) * 4;
            const float nanv = __uint_as_float(0x7fc00000u);
            const float nm1 = (float)(n ? n - 1 : 0);
            const float qs[3] = {0.25f, 0.5f, 0.75f};
            for (int i = 0; i < 3; ++i) {
                const float r = qs[i] * nm1;
                const float w = r - floorf(r);
                const float lo = ev_unkey(pre[2 * i]), hi = ev_unkey(pre[2 * i + 1]);
                t[i] = !n ? nanv : ((median_mid && i == 1) ? lo : ev_lerp(lo, hi, w));
            }
            t[3] = 0.f;
        }
    }
    __syncthreads();
}

// The call's last workgroup: partial sums in a fixed order (wave 0: two partials per lane of the wave, then the butterfly), counters, the row.
template <bool FLOW>
__device__ void ev_finalize(const EvArgs& a, int lane) {
    if (threadIdx.x >= 64) return;
    const int G = gridDim.x, l = threadIdx.x;
    const bool has_cov = a.cov != nullptr;
    double sA[3], sB[3];
    for (int c = 0; c < 3; ++c) {
        const double* pa = a.partA + ((size_t)lane * G) * EV_PART + c;
        double v = (l < G ? ev_ldd(pa + (size_t)l * EV_PART) : 0.0) + (l + 64 < G ? ev_ldd(pa + (size_t)(l + 64) * EV_PART) : 0.0);
        sA[c] = wave_sum(v);
        double u = 0.0;
        if (has_cov) {
            const double* pb = a.partB + ((size_t)lane * G) * EV_PART + c;
            u = (l < G ? ev_ldd(pb + (size_t)l * EV_PART) : 0.0) + (l + 64 < G ? ev_ldd(pb + (size_t)(l + 64) * EV_PART) : 0.0);
        }
        sB[c] = wave_sum(u);
    }
    if (l != 0) return;
    const uint32_t* ct = a.ctrl + lane * EV_CTRL_WORDS;
    uint32_t cn[C_END];
    for (int i = C_MASK; i < C_END; ++i) cn[i] = ev_ld(ct + i);
    const float nanv = __uint_as_float(0x7fc00000u);
    float* row = a.rows + ((size_t)lane * a.rows_per_lane + a.row_index) * a.ncols;
    const float* t0 = a.thr + (lane * EV_POPS + 0) * 4;
    const float* t1 = a.thr + (lane * EV_POPS + 1) * 4;
    auto mean = [](double s, uint32_t c) { return (float)(s / (double)c); };   // 0 / 0 = NaN: an empty population
    if constexpr (FLOW) {
        row[MV_EVAL_FLOW_MASKED_EPE] = mean(sA[0], cn[C_MASK_FIN]);
        row[MV_EVAL_FLOW_EPE] = mean(sA[1], cn[C_FIN]);
        row[MV_EVAL_FLOW_PX1] = (float)cn[C_PX1] / (float)cn[C_MASK];
        row[MV_EVAL_FLOW_PX3] = (float)cn[C_PX3] / (float)cn[C_MASK];
        row[MV_EVAL_FLOW_PX5] = (float)cn[C_PX5] / (float)cn[C_MASK];
        row[MV_EVAL_FLOW_MASKED_NLL] = has_cov ? mean(sA[2], cn[C_MASK_NLL]) : nanv;
        for (int i = 0; i < 3; ++i) {
            row[MV_EVAL_FLOW_Q25_NLL + i] = has_cov ? mean(sB[i], cn[C_CQ + i]) : nanv;
            row[MV_EVAL_FLOW_T25 + i] = has_cov ? t0[i] : nanv;
            row[MV_EVAL_FLOW_N_Q25 + i] = (float)cn[C_NQ + i];
        }
        row[MV_EVAL_FLOW_N_MASK] = (float)cn[C_MASK];
        row[MV_EVAL_FLOW_N_MASK_FINITE] = (float)cn[C_MASK_FIN];
        row[MV_EVAL_FLOW_N_FINITE] = (float)cn[C_FIN];
        row[MV_EVAL_FLOW_N_MASK_NLL] = (float)cn[C_MASK_NLL];
    } else {
        row[MV_EVAL_DEPTH_MASKED_ERR] = mean(sA[0], cn[C_MASK_FIN]);
        row[MV_EVAL_DEPTH_ERR_25] = t1[0];
        row[MV_EVAL_DEPTH_ERR_50] = t1[1];
        row[MV_EVAL_DEPTH_ERR_75] = t1[2];
        row[MV_EVAL_DEPTH_MASKED_NLL] = has_cov ? mean(sA[2], cn[C_MASK_NLL]) : nanv;
        for (int i = 0; i < 3; ++i) {
            row[MV_EVAL_DEPTH_Q25_NLL + i] = has_cov ? mean(sB[i], cn[C_CQ + i]) : nanv;
            row[MV_EVAL_DEPTH_T25 + i] = has_cov ? t0[i] : nanv;
            row[MV_EVAL_DEPTH_N_Q25 + i] = (float)cn[C_NQ + i];
        }
        row[MV_EVAL_DEPTH_N_MASK] = (float)cn[C_MASK];
        row[MV_EVAL_DEPTH_N_MASK_FINITE] = (float)cn[C_MASK_FIN];
        row[MV_EVAL_DEPTH_N_FINITE] = (float)cn[C_FIN];
        row[MV_EVAL_DEPTH_N_MASK_NLL] = (float)cn[C_MASK_NLL];
    }
}

template <bool FLOW>
__global__ __launch_bounds__(EV_NT) void eval_pixel_kernel(EvArgs a) {
    __shared__ uint32_t s_grid[(FLOW ? 2 : 1) * EV_GRID_WORDS];
    __shared__ uint32_t s_hist[EV_POPS * EV_BINS];
    __shared__ double s_red[4];
    __shared__ uint32_t s_w[4], s_res[2 * EV_SLOTS], s_cnt[EV_CTRL_WORDS];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = blockIdx.y, G = gridDim.x, n = a.n;
    const bool has_cov = a.cov != nullptr, do_grid = has_cov && a.grids != nullptr;
    if (tid < EV_CTRL_WORDS) s_cnt[tid] = 0;
    const bool pop0 = has_cov, pop1 = !FLOW;
    constexpr int NG = FLOW ? 2 : 1;
    const float gscale = FLOW ? 4.0f : 2.0f;
    for (int i = tid; i < NG * EV_GRID_WORDS; i += EV_NT) s_grid[i] = 0;
    for (int i = tid; i < EV_POPS * EV_BINS; i += EV_NT) s_hist[i] = 0;
    __syncthreads();

    uint32_t* ctrl = a.ctrl + lane * EV_CTRL_WORDS;
    double s_mask = 0.0, s_all = 0.0, s_nll = 0.0;
    int c_mask = 0, c_mask_fin = 0, c_fin = 0, c1 = 0, c3 = 0, c5 = 0, c_nll = 0;
    const int nquads = (n + 3) / 4;
    for (int qi = blockIdx.x * EV_NT + tid; qi < nquads; qi += G * EV_NT) {
        const int i0 = qi * 4;
        EvQuad q;
        ev_quad<FLOW>(a, lane, i0, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) continue;
            const float e = q.err[k];
            const bool fin = !isnan(e), m = q.mask[k];
            c_fin += fin;
            if (fin) s_all += (double)e;
            if (m) {
                ++c_mask;
                c_mask_fin += fin;
                if (fin) s_mask += (double)e;
                if (FLOW) c1 += e < 1.f, c3 += e < 3.f, c5 += e < 5.f;
                if (has_cov && !isnan(q.nll[k])) ++c_nll, s_nll += (double)q.nll[k];
                if (pop1 && fin) atomicAdd(&s_hist[EV_BINS + (ev_key(e) >> 21)], 1u);
            }
            if (pop0 && !isnan(q.unc[k])) atomicAdd(&s_hist[ev_key(q.unc[k]) >> 21], 1u);
            if (do_grid) {
                const int b0 = ev_bin(q.e2a[k], gscale), b1 = ev_bin(q.ca[k], gscale);
                if (b0 >= 0 && b1 >= 0) {
                    const int bin = b0 * EV_GRID + b1;
                    atomicAdd(&s_grid[bin >> 1], 1u << (16 * (bin & 1)));
                }
                if (FLOW) {
                    const int d0 = ev_bin(q.e2b[k], gscale), d1 = ev_bin(q.cb[k], gscale);
                    if (d0 >= 0 && d1 >= 0) {
                        const int bin = d0 * EV_GRID + d1;
                        atomicAdd(&s_grid[EV_GRID_WORDS + (bin >> 1)], 1u << (16 * (bin & 1)));
                    }
                }
            }
        }
        if (a.err_out) ev_st4(a.err_out + (size_t)lane * n, i0, n, a.vec != 0, q.err);
        if (a.nll_out && has_cov) ev_st4(a.nll_out + (size_t)lane * n, i0, n, a.vec != 0, q.nll);
    }
    const double t_mask = ev_block_sum(s_mask, s_red), t_all = ev_block_sum(s_all, s_red), t_nll = ev_block_sum(s_nll, s_red);
    if (tid == 0) {
        double* p = a.partA + ((size_t)lane * G + blockIdx.x) * EV_PART;
        ev_std(p + 0, t_mask), ev_std(p + 1, t_all), ev_std(p + 2, t_nll);
    }
    ev_count(s_cnt, C_MASK, c_mask), ev_count(s_cnt, C_MASK_FIN, c_mask_fin), ev_count(s_cnt, C_FIN, c_fin);
    if (FLOW) ev_count(s_cnt, C_PX1, c1), ev_count(s_cnt, C_PX3, c3), ev_count(s_cnt, C_PX5, c5);
    if (has_cov) ev_count(s_cnt, C_MASK_NLL, c_nll);
    __syncthreads();
    ev_count_flush(ctrl, s_cnt);
    if (do_grid) {
        uint32_t* g = a.grids + (size_t)lane * NG * EV_GRID * EV_GRID;
        for (int i = tid; i < NG * EV_GRID_WORDS; i += EV_NT) {
            const uint32_t w = s_grid[i];
            if (w & 0xffffu) atomicAdd(g + 2 * i, w & 0xffffu);
            if (w >> 16) atomicAdd(g + 2 * i + 1, w >> 16);
        }
    }
    for (int p = 0; p < EV_POPS; ++p) {
        if (!(p == 0 ? pop0 : pop1)) continue;
        uint32_t* H = a.hist + (size_t)(lane * EV_POPS + p) * EV_SLOTS * EV_BINS;
        for (int i = tid; i < EV_BINS; i += EV_NT) {
            const uint32_t w = s_hist[p * EV_BINS + i];
            if (w) atomicAdd(H + i, w);
        }
    }
    if (!ev_arrive(ctrl + T_PIXEL, &s_last)) return;
    if (pop0) ev_scan_pass(a, lane, 0, 0, s_w, s_res);
    if (pop1) ev_scan_pass(a, lane, 1, 0, s_w, s_res);
    if (FLOW && !has_cov) ev_finalize<FLOW>(a, lane);
}

// digit pass 1 or 2 of population pop_base + blockIdx.z
template <bool FLOW>
__global__ __launch_bounds__(EV_NT) void eval_select_kernel(EvArgs a, int pass, int pop_base) {
    __shared__ uint32_t s_hist[EV_SLOTS * EV_BINS];
    __shared__ uint32_t s_w[4], s_res[2 * EV_SLOTS];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = blockIdx.y, G = gridDim.x, n = a.n, pop = pop_base + blockIdx.z;
    const EvSel* st = a.state + lane * EV_POPS + pop;
    uint32_t pre[EV_SLOTS];
    bool own[EV_SLOTS];
    for (int j = 0; j < EV_SLOTS; ++j) pre[j] = st->prefix[j], own[j] = st->lead[j] == (uint32_t)j;
    const uint32_t np = st->n;
    for (int i = tid; i < EV_SLOTS * EV_BINS; i += EV_NT) s_hist[i] = 0;
    __syncthreads();
    const int sh_prev = ev_shift(pass - 1), sh = ev_shift(pass);
    const uint32_t dmask = (uint32_t)ev_nbins(pass) - 1u;
    const int nquads = (n + 3) / 4;
    if (np) {
        for (int qi = blockIdx.x * EV_NT + tid; qi < nquads; qi += G * EV_NT) {
            const int i0 = qi * 4;
            EvQuad q;
            ev_quad<FLOW>(a, lane, i0, q);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k >= n) continue;
                const float v = pop == 0 ? q.unc[k] : q.err[k];
                if (isnan(v) || (pop == 1 && !q.mask[k])) continue;
                const uint32_t key = ev_key(v), hi = key >> sh_prev, d = (key >> sh) & dmask;
#pragma unroll
                for (int j = 0; j < EV_SLOTS; ++j)
                    if (own[j] && hi == pre[j]) atomicAdd(&s_hist[j * EV_BINS + d], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* H = a.hist + (size_t)(lane * EV_POPS + pop) * EV_SLOTS * EV_BINS;
    for (int j = 0; j < EV_SLOTS; ++j) {
        if (!own[j]) continue;
        for (int i = tid; i < EV_BINS; i += EV_NT) {
            const uint32_t w = s_hist[j * EV_BINS + i];
            if (w) atomicAdd(H + j * EV_BINS + i, w);
        }
    }
    uint32_t* ctrl = a.ctrl + lane * EV_CTRL_WORDS;
    if (!ev_arrive(ctrl + T_SELECT + 2 * (pass - 1) + pop, &s_last)) return;
    ev_scan_pass(a, lane, pop, pass, s_w, s_res);
    if (!FLOW && pass == 2 && a.cov == nullptr) {   // (ev_scan_pass ends with a barrier: the thresholds it stored are visible to this workgroup's wave 0)
        ev_finalize<FLOW>(a, lane);
    }
}

// NLL means within `uncertainty < t_q` (strict; all pixels, the mask is not intersected), then the row
template <bool FLOW>
__global__ __launch_bounds__(EV_NT) void eval_qmean_kernel(EvArgs a) {
    __shared__ double s_red[4];
    __shared__ uint32_t s_cnt[EV_CTRL_WORDS];
    __shared__ int s_last;
    const int tid = threadIdx.x, lane = blockIdx.y, G = gridDim.x, n = a.n;
    if (tid < EV_CTRL_WORDS) s_cnt[tid] = 0;
    __syncthreads();
    const float* t = a.thr + (lane * EV_POPS + 0) * 4;
    const float t0 = t[0], t1 = t[1], t2 = t[2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int nq0 = 0, nq1 = 0, nq2 = 0, cq0 = 0, cq1 = 0, cq2 = 0;
    const int nquads = (n + 3) / 4;
    for (int qi = blockIdx.x * EV_NT + tid; qi < nquads; qi += G * EV_NT) {
        const int i0 = qi * 4;
        EvQuad q;
        ev_quad<FLOW>(a, lane, i0, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k >= n) continue;
            const float u = q.unc[k], v = q.nll[k];
            const bool f = !isnan(v);
            if (u < t0) { ++nq0; if (f) ++cq0, s0 += (double)v; }
            if (u < t1) { ++nq1; if (f) ++cq1, s1 += (double)v; }
            if (u < t2) { ++nq2; if (f) ++cq2, s2 += (double)v; }
        }
    }
    const double r0 = ev_block_sum(s0, s_red), r1 = ev_block_sum(s1, s_red), r2 = ev_block_sum(s2, s_red);
    if (tid == 0) {
        double* p = a.partB + ((size_t)lane * G + blockIdx.x) * EV_PART;
        ev_std(p + 0, r0), ev_std(p + 1, r1), ev_std(p + 2, r2);
    }
    uint32_t* ctrl = a.ctrl + lane * EV_CTRL_WORDS;
    ev_count(s_cnt, C_NQ + 0, nq0), ev_count(s_cnt, C_NQ + 1, nq1), ev_count(s_cnt, C_NQ + 2, nq2);
    ev_count(s_cnt, C_CQ + 0, cq0), ev_count(s_cnt, C_CQ + 1, cq1), ev_count(s_cnt, C_CQ + 2, cq2);
    __syncthreads();
    ev_count_flush(ctrl, s_cnt);
    if (!ev_arrive(ctrl + T_QMEAN, &s_last)) return;
    ev_finalize<FLOW>(a, lane);
}

// ---- workspace: [hist | ctrl] (zeroed per call) | state | thr | partA | partB
struct EvLayout {
    size_t hist, ctrl, zero_bytes, state, thr, partA, partB, total;
};
inline EvLayout ev_layout(int lanes, int n) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    EvLayout L;
    const size_t G = (size_t)ev_blocks(n);
    L.hist = 0;
    L.ctrl = L.hist + (size_t)lanes * EV_POPS * EV_SLOTS * EV_BINS * sizeof(uint32_t);
    L.zero_bytes = L.ctrl + (size_t)lanes * EV_CTRL_WORDS * sizeof(uint32_t);
    L.state = up(L.zero_bytes);
    L.thr = up(L.state + (size_t)lanes * EV_POPS * sizeof(EvSel));
    L.partA = up(L.thr + (size_t)lanes * EV_POPS * 4 * sizeof(float));
    L.partB = up(L.partA + (size_t)lanes * G * EV_PART * sizeof(double));
    L.total = up(L.partB + (size_t)lanes * G * EV_PART * sizeof(double));
    return L;
}

inline bool ev_aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

template <bool FLOW>
int ev_run(EvArgs a, int lanes, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const EvLayout L = ev_layout(lanes, a.n);
    MV_CHECK_ARG(workspace != nullptr && ev_aligned(workspace, 16));
    if (workspace_bytes < L.total) return MV_ERR_WORKSPACE;
    char* ws = (char*)workspace;
    a.hist = (uint32_t*)(ws + L.hist), a.ctrl = (uint32_t*)(ws + L.ctrl), a.state = (EvSel*)(ws + L.state), a.thr = (float*)(ws + L.thr);
    a.partA = (double*)(ws + L.partA), a.partB = (double*)(ws + L.partB);
    if (hipMemsetAsync(ws, 0, L.zero_bytes, st) != hipSuccess) return MV_ERR_LAUNCH;
    const bool has_cov = a.cov != nullptr;
    const dim3 grid(ev_blocks(a.n), lanes), block(EV_NT);
    hipLaunchKernelGGL(eval_pixel_kernel<FLOW>, grid, block, 0, st, a);
    const int pop_base = has_cov ? 0 : 1, npops = (has_cov ? 1 : 0) + (FLOW ? 0 : 1);
    if (npops) {
        const dim3 sgrid(grid.x, lanes, npops);
        hipLaunchKernelGGL(eval_select_kernel<FLOW>, sgrid, block, 0, st, a, 1, pop_base);
        hipLaunchKernelGGL(eval_select_kernel<FLOW>, sgrid, block, 0, st, a, 2, pop_base);
    }
    if (has_cov) hipLaunchKernelGGL(eval_qmean_kernel<FLOW>, grid, block, 0, st, a);
    return mv_launch_status();
}

}  // namespace

extern "C" size_t mv_eval_workspace_bytes(int lanes, int H, int W) {
    if (lanes < 1 || lanes > MV_MAX_LANES || H < 1 || W < 1 || (long long)H * W > (1ll << 22)) return 0;
    return ev_layout(lanes, H * W).total;
}

extern "C" int mv_eval_flow_lanes(int lanes, int H, int W, const float* est_flow, int64_t est_lane_stride, const float* gt_flow, int64_t gt_lane_stride,
                                  const float* est_cov, int64_t cov_plane_stride, int64_t cov_lane_stride, const uint8_t* valid,
                                  int64_t valid_lane_stride, float max_flow, int apply_max_flow, float* rows, int rows_per_lane, int row_index,
                                  uint32_t* grids, float* epe_out, float* nll_out, void* workspace, size_t workspace_bytes, mvStream_t stream) {
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES && H >= 1 && W >= 1 && (long long)H * W <= (1ll << 22));
    MV_CHECK_ARG(est_flow && gt_flow && rows && rows_per_lane >= 1 && row_index >= 0 && row_index < rows_per_lane);
    const int n = H * W;
    MV_CHECK_ARG(est_lane_stride >= 2ll * n && gt_lane_stride >= 2ll * n);
    MV_CHECK_ARG(!est_cov || (cov_plane_stride >= n && cov_lane_stride >= cov_plane_stride + n));
    MV_CHECK_ARG(!valid || valid_lane_stride >= n);
    EvArgs a{};
    a.est = est_flow, a.gt = gt_flow, a.cov = est_cov, a.valid = valid;
    a.est_ls = est_lane_stride, a.gt_ls = gt_lane_stride, a.cov_ls = cov_lane_stride, a.cov_ps = cov_plane_stride, a.valid_ls = valid_lane_stride;
    a.maxv = max_flow, a.apply_max = apply_max_flow != 0, a.n = n;
    // 16-byte loads: every plane of every lane starts on a 16-byte boundary (the v planes start n floats behind the u planes)
    a.vec = n % 4 == 0 && ev_aligned(est_flow, 16) && ev_aligned(gt_flow, 16) && ev_aligned(est_cov, 16) && ev_aligned(valid, 4) &&
            ev_aligned(epe_out, 16) && ev_aligned(nll_out, 16) && est_lane_stride % 4 == 0 && gt_lane_stride % 4 == 0 &&
            (!est_cov || (cov_plane_stride % 4 == 0 && cov_lane_stride % 4 == 0)) && (!valid || valid_lane_stride % 4 == 0);
    a.rows = rows, a.rows_per_lane = rows_per_lane, a.row_index = row_index, a.ncols = MV_EVAL_FLOW_COLS;
    a.grids = grids, a.err_out = epe_out, a.nll_out = nll_out;
    return ev_run<true>(a, lanes, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int mv_eval_depth_lanes(int lanes, int H, int W, const float* est_depth, int64_t est_lane_stride, const float* gt_depth,
                                   int64_t gt_lane_stride, const float* est_cov, int64_t cov_lane_stride, float max_depth, float* rows,
                                   int rows_per_lane, int row_index, uint32_t* grid, float* err_out, float* nll_out, void* workspace,
                                   size_t workspace_bytes, mvStream_t stream) {
    MV_CHECK_ARG(lanes >= 1 && lanes <= MV_MAX_LANES && H >= 1 && W >= 1 && (long long)H * W <= (1ll << 22));
    MV_CHECK_ARG(est_depth && gt_depth && rows && rows_per_lane >= 1 && row_index >= 0 && row_index < rows_per_lane);
    const int n = H * W;
    MV_CHECK_ARG(est_lane_stride >= n && gt_lane_stride >= n && (!est_cov || cov_lane_stride >= n));
    EvArgs a{};
    a.est = est_depth, a.gt = gt_depth, a.cov = est_cov;
    a.est_ls = est_lane_stride, a.gt_ls = gt_lane_stride, a.cov_ls = cov_lane_stride;
    a.maxv = max_depth, a.n = n;
    a.vec = n % 4 == 0 && ev_aligned(est_depth, 16) && ev_aligned(gt_depth, 16) && ev_aligned(est_cov, 16) && ev_aligned(err_out, 16) &&
            ev_aligned(nll_out, 16) && est_lane_stride % 4 == 0 && gt_lane_stride % 4 == 0 && (!est_cov || cov_lane_stride % 4 == 0);
    a.rows = rows, a.rows_per_lane = rows_per_lane, a.row_index = row_index, a.ncols = MV_EVAL_DEPTH_COLS;
    a.grids = grid, a.err_out = err_out, a.nll_out = nll_out;
    return ev_run<false>(a, lanes, workspace, workspace_bytes, (hipStream_t)stream);
}
