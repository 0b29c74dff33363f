// RandomSelector / GridSelector as stand-alone launches (kp_draw_dev.h holds the arithmetic; the frame driver draws inside its front launch instead):
//   mv_kp_random_lanes     one workgroup per lane: 2 * num_point words of the lane's device-resident MT19937 -> int64 (u, v) rows, generator advanced in place
//   mv_kp_random_emulated  host-only, no GPU: the SAME phase functions executed thread by thread — pins them against torch.randint
//   mv_kp_random_heads     host-only twin on std::mt19937 (what the host-seeded finish of the frame driver draws)
//   mv_kp_grid_count / mv_kp_grid
#include "common.h"
#include "kp_draw_dev.h"
#include <random>
#include <vector>

namespace {

__global__ __launch_bounds__(256) void kp_random_kernel(uint32_t* __restrict__ state, int k, int H, int W, int mask, int64_t* __restrict__ out_uv) {
    __shared__ mvkp::Scratch s;
    const int l = blockIdx.x;
    uint32_t* const st = state + (size_t)l * mvrp::MT_STRIDE;
    mv_kp_random_wg(st, st, k, s);
    mvkp::phase_rows(s.w, k, H, W, mask, out_uv + 2 * (size_t)l * k, threadIdx.x, blockDim.x);
}

__global__ __launch_bounds__(256) void kp_grid_kernel(mvkp::Grid g, int n, int64_t* __restrict__ out_uv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int u, v;
    mvkp::grid_row(g, i, u, v);
    out_uv[2 * i] = u;
    out_uv[2 * i + 1] = v;
}

}  // namespace

static inline bool random_shape_ok(int num_point, int H, int W, int mask) {
    return num_point >= 0 && mask >= 0 && H > 2 * mask && W > 2 * mask;
}

extern "C" int mv_kp_random_max_point(void) { return mvkp::MAX_POINT; }

extern "C" int mv_kp_random_lanes(uint32_t* state, int lanes, int num_point, int H, int W, int mask_width, int64_t* out_uv, mvStream_t stream) {
    MV_CHECK_ARG(state && lanes >= 1 && random_shape_ok(num_point, H, W, mask_width) && (out_uv || num_point == 0));
    if (num_point > mvkp::MAX_POINT) return MV_ERR_UNSUPPORTED;
    if (num_point == 0) return MV_OK;
    hipLaunchKernelGGL(kp_random_kernel, dim3(lanes), dim3(256), 0, (hipStream_t)stream, state, num_point, H, W, mask_width, out_uv);
    return mv_launch_status();
}

int mv_randperm_heads_emulated_state(uint32_t* state, const int64_t* n, int calls, int k, int threads, int64_t* out);   // (randperm.hip)

static int kp_random_emulated_state(uint32_t* state, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out);

extern "C" int mv_kp_random_emulated(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out) {
    std::vector<uint32_t> state(mvrp::MT_STRIDE);
    mvrp::mt_seed((uint32_t)(seed & 0xffffffffull), state.data());
    return kp_random_emulated_state(state.data(), calls, num_point, H, W, mask_width, threads, out);
}

// ... followed by one emulated torch.randperm(perm_n)[:perm_k] from the SAME generator state (the word stream continues: a frame's MappingPointSelector
// permutation is drawn behind its RandomSelector keypoints)
extern "C" int mv_kp_random_then_randperm_emulated(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out,
                                                   int64_t perm_n, int perm_k, int64_t* out_perm) {
    std::vector<uint32_t> state(mvrp::MT_STRIDE);
    mvrp::mt_seed((uint32_t)(seed & 0xffffffffull), state.data());
    const int rc = kp_random_emulated_state(state.data(), calls, num_point, H, W, mask_width, threads, out);
    return rc != MV_OK ? rc : mv_randperm_heads_emulated_state(state.data(), &perm_n, 1, perm_k, threads, out_perm);
}

static int kp_random_emulated_state(uint32_t* state, int calls, int num_point, int H, int W, int mask_width, int threads, int64_t* out) {
    using namespace mvkp;
    MV_CHECK_ARG(out && calls >= 0 && random_shape_ok(num_point, H, W, mask_width) && threads >= 1 && threads <= 4096);
    if (num_point > MAX_POINT) return MV_ERR_UNSUPPORTED;
    Scratch* s = new Scratch;
    const int nt = threads;
#define MV_KP_ALL(call) for (int tid = 0; tid < nt; ++tid) { call; }
    for (int c = 0; c < calls; ++c) {   // (the workgroup driver of kp_draw_dev.h, barriers replaced by the end of each thread loop)
        for (int i = 0; i < mvrp::MT_N; ++i) s->mt[0][i] = state[i];
        const Plan pl = plan_of(num_point, (int)state[mvrp::MT_N]);
        int cur = 0;
        for (int blk = 0; blk <= pl.steps; ++blk) {
            if (blk > 0) {
                MV_KP_ALL(mvrp::phase_step(s->mt[cur], s->mt[cur ^ 1], tid, nt));
                cur ^= 1;
            }
            MV_KP_ALL(phase_words(s->mt[cur], blk, pl, s->w, tid, nt));
        }
        for (int i = 0; i < mvrp::MT_N; ++i) state[i] = s->mt[cur][i];
        state[mvrp::MT_N] = (uint32_t)pl.pos_out;
        MV_KP_ALL(phase_rows(s->w, num_point, H, W, mask_width, out + 2 * (size_t)c * num_point, tid, nt));
    }
#undef MV_KP_ALL
    delete s;
    return MV_OK;
}

// one RandomSelector call of a std::mt19937 (= at::mt19937): k words of v, then k words of u
void mv_kp_random_draw_host(std::mt19937& eng, int k, int H, int W, int mask, int64_t* out_uv) {
    for (int n = 0; n < k; ++n) out_uv[2 * n + 1] = (int64_t)((uint32_t)eng() % (uint32_t)(H - 2 * mask)) + mask;
    for (int n = 0; n < k; ++n) out_uv[2 * n] = (int64_t)((uint32_t)eng() % (uint32_t)(W - 2 * mask)) + mask;
}

extern "C" int mv_kp_random_heads(uint64_t seed, int calls, int num_point, int H, int W, int mask_width, int64_t* out) {
    MV_CHECK_ARG(out && calls >= 0 && random_shape_ok(num_point, H, W, mask_width));
    std::mt19937 eng((uint32_t)(seed & 0xffffffffull));
    for (int c = 0; c < calls; ++c) mv_kp_random_draw_host(eng, num_point, H, W, mask_width, out + 2 * (size_t)c * num_point);
    return MV_OK;
}

extern "C" int mv_kp_grid_count(int H, int W, int mask_width, int num_point) { return mvkp::grid_of(H, W, mask_width, num_point, nullptr); }

extern "C" int mv_kp_grid(int H, int W, int mask_width, int num_point, int64_t* out_uv, mvStream_t stream) {
    mvkp::Grid g;
    const int n = mvkp::grid_of(H, W, mask_width, num_point, &g);
    MV_CHECK_ARG(n > 0 && out_uv);
    hipLaunchKernelGGL(kp_grid_kernel, dim3(mv_ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, g, n, out_uv);
    return mv_launch_status();
}
