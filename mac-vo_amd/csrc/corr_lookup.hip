// A6 — (2r+1)^2 bilinear window lookup in each query pixel's own H2 x W2 cost slice
//
// Replaces FlowFormer MemoryDecoder.encode_flow_token(cost_maps, coords1) called at
// Module/Network/FlowFormerCov/covhead.py:92 ("MUST run in fp32", :91): RAFT window
// delta[i][j] = (dy[i], dx[j]) added to (x, y)  =>  channel k = K*i + j samples (x + i - r, y + j - r),
// bilinear_sampler = grid_sample(align_corners=True, zeros) after normalising by (W2-1), (H2-1).
//
// gfx950 design.  One frame's lookup (9600 queries) is ~4 MB of traffic: neither HBM nor the texture path is the
// limit, the VALU instruction stream of the few resident waves is (measured: launch floor 3.4 us, staging + stores
// +1.6 us, and the per-tap coordinate arithmetic of a lane-per-tap formulation another +3.5 us).  Hence:
//   * a wave owns QPW queries; a workgroup QPB of them (QPB consecutive queries = one contiguous output segment per
//     channel).
//   * staging: per query the (K+3)^2 cell block that covers every tap (block origin floor(x)-r-1: one spare cell each
//     side absorbs the fp32 normalise/un-normalise round trip) is fetched with lane = (row-in-group, column): the
//     lane's (row, column) split is computed once, the query origin is wave-uniform (readlane -> SGPR), so a load costs
//     a handful of VALU ops; all loads are issued before LDS is touched; out-of-image cells are zero (= zero padding).
//   * per-AXIS coordinate math: RAFT's normalise + ATen's un-normalise + floor/weights depend only on (query, i) for x
//     and (query, j) for y: 2K values per query instead of 2*K*K.  Lanes [0, 2K) of an "axis pass" evaluate them for one
//     query, the next 2K lanes for the next query, ... (true division, same fp32 op order as grid_sample) and write the
//     (weight, cell) entries to LDS.  Results are bit-identical to the per-tap form.
//   * taps: the wave's QPW * K*K (tap, query) PAIRS are dealt over its lanes (four queries: 324 pairs in 6 rounds; "lane = tap, query
//     after query" took 8, every second one with 17 live lanes); a pair reads its two axis entries (two 8-byte LDS reads), 4 cells, and
//     forms the ATen bilinear sum.  For r = 4 the deal and the block strides are chosen so that a 32-lane group reads 32 different LDS
//     banks (tap_phase below; CPU model: profiles/probes/lookup_lds_bank_model.py — 34.5 % of the kernel's LDS-array cycles were
//     conflicts, 0 now for the row-major block, the rest of the tiled block's is its staging stores).
//   * output [B, K*K, H1, W1] is channel-major: results are transposed through LDS so every channel row is written as one QPB*4-byte
//     segment.  A wave parks its results in a strip that aliases ITS OWN staged blocks.
//   * ONE workgroup barrier, in front of the transposed store (the only place where a wave reads what another wave wrote).  Staging ->
//     taps and taps -> strip are hand-overs inside one wave (wave_lds_handover: in-order LDS, no instruction); before, every wave of
//     the workgroup waited at two more barriers for the slowest wave's cell loads and tap reads.
//   * static LDS per workgroup (r = 4): 11 648 B for 16 queries (8 waves x 2 blocks of 146 floats + 2 304 B of axis entries; 11 520 B
//     before), 23 680 B for 32; tiled blocks (16 x 20 + 18 floats): 23 936 B / 48 256 B.  Beside one f16x2 GEMM workgroup per CU
//     (304 of 512 registers per SIMD, 96 KB of LDS) the 16-query workgroup (31 registers -> 2 x 32 per SIMD) is limited by the 208 free
//     registers to three workgroups (64 registers per SIMD each; at the 33 -> 40 registers before: two) and by LDS to five.  Beside the 144-KB ring of the
//     bf16x3 GEMM (16 KB free) one workgroup fits, as before — which is why the strip aliases the blocks rather than adding
//     81 x 17 floats of its own.
#include "common.h"

namespace {

// One axis entry of a query — what RAFT's normalise + ATen's un-normalise make of (coordinate + offset): the bilinear weight and the clamped
// cell offset in the staged block | (1 << 8) when the tap's 2-cell span lies inside the block.  The axis passes write the 2 K entries of
// every query of the wave into LDS; the tap phase reads them back per (tap, query) PAIR (8-byte aligned: one ds_read_b64 each).
struct alignas(8) AxisEntry { float w; int c; };

// Hand-over of LDS contents between the lanes of ONE wave: the LDS unit executes a wave's operations in order, so all that is needed is
// that the compiler keeps the order too (it reasons per thread and would otherwise be free to move a read above another lane's write).
// Emits no instruction and no wait; NOT a workgroup barrier.
__device__ __forceinline__ void wave_lds_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One tap: the ATen bilinear sum, term for term (every expression and its order as in every earlier form of this file)
template <int K, int STRIDE>
__device__ __forceinline__ float tap_one(const float* qblk, const AxisEntry* qax, int ti, int tj) {
    const AxisEntry X = qax[ti], Y = qax[K + tj];
    const float w = X.w, n = Y.w;
    const bool inblk = ((X.c & Y.c) & 256) != 0;
    const float* p = &qblk[(Y.c & 255) * STRIDE + (X.c & 255)];
    const float e = 1.f - w, so = 1.f - n;
    const float vnw = inblk ? p[0] : 0.f, vne = inblk ? p[1] : 0.f;
    const float vsw = inblk ? p[STRIDE] : 0.f, vse = inblk ? p[STRIDE + 1] : 0.f;
    // ATen: (nw_val*nw + ne_val*ne) + sw_val*sw + se_val*se with nw = s*e, ne = s*w, sw = n*e, se = n*w
    float r0 = vnw * (so * e);
    r0 = r0 + vne * (so * w);
    r0 = r0 + vsw * (n * e);
    r0 = r0 + vse * (n * w);
    return r0;
}

// A wave's output strip holds the results of its query s at strip[s * strip_pitch + u], u < K K; the strips of the workgroup's waves are
// wave_floats apart.  For K = 9 the pitch and the distance are chosen so that the transposed store's LDS reads — 32 lanes = 32 queries of
// one row u (four-query waves) or 16 queries of two rows (two-query waves) — touch 32 different banks: 8 waves x 20 (resp. 4) banks apart,
// queries 83 (resp. 82) floats apart.
template <int K, int QPW>
constexpr int strip_pitch() { return K * K + ((K == 9 && QPW == 4) ? 2 : 1); }
template <int K, int QPW, int CELLS>
constexpr int wave_floats() { return QPW * CELLS + ((K == 9 && QPW == 4) ? 12 : 0); }

// Row u of a wave's output strip holds channel tap_channel(u).  K = 9: u enumerates the 8 x 9 body of the window (u = 8 ti + tj,
// tj < 8), then the row tj = 8 (u = 72 + ti) — the order the taps are dealt in; any other K: u = channel.
template <int K>
__device__ __forceinline__ int tap_channel(int u) {
    if constexpr (K == 9) return u < 72 ? u + (u >> 3) : 9 * (u - 72) + 8;
    else return u;
}

// Tap phase shared by the lookup kernels: the wave's QPW * K * K (tap, query) pairs are dealt over its lanes, a pair reads its two axis
// entries (two 8-byte LDS reads) and 4 cells and forms the bilinear sum; the sums then go to the wave's OWN output strip
// strip[s * strip_pitch + u], which aliases the wave's staged blocks — only this wave ever read those, so the hand-over is wave-local.
// (s, ti, tj) and the strip address are derived once per round, without a division.
//
// K = 9 (radius 4, every hot path).  The cell of tap (ti, tj) sits at STRIDE * (tj + cy) + ti + cx of its query's block; with
// STRIDE = 12 (row-major) or 20 (tiled) that is bank 4 * (3 tj mod 8) + ti resp. 4 * (5 tj mod 8) + ti (+ a per-query constant): the 4 x 8
// taps ti0 .. ti0 + 3, tj 0 .. 7 of ONE query cover the 32 banks exactly once.  Hence (profiles/probes/lookup_lds_bank_model.py):
//   * rounds 0 .. QPW - 1: round r = query r, lane = 8 ti + tj over ti, tj in 0 .. 7: each 32-lane group is one such 4 x 8 patch — the
//     four cell reads and both axis reads are conflict-free, and (s, ti, tj) cost one shift and one mask for all rounds;
//   * QPW / 2 rounds for what is left of two queries each (17 taps per query): lanes 0 .. 15 the column ti = 8 (tj 0 .. 7) of both,
//     lanes 32 .. 49 the row tj = 8 (ti 0 .. 8) of both.  A query's block starts CELLS = 18 mod 32 banks behind its neighbour's, which
//     keeps the two columns (banks 0 mod 4 | 2 mod 4) and the two rows (9 consecutive banks each, 18 apart) disjoint as long as both
//     queries sit at the same offset in their blocks (always in the row-major block; the tiled block adds (x mod 4, y mod 4)).
//   The same number of rounds as dealing 64 consecutive pairs per round (3 for two queries, 6 for four), which put rows tj = 0 and
//   tj = 8 of every column on one bank: two-way conflicts in every group of every cell read.
// Any other K: 64 consecutive pairs per round, (s, ti, tj) advanced by 64 as a three-digit number in base K.
template <int K, int QPW, int STRIDE, int CELLS>
__device__ __forceinline__ void tap_phase(float* blk, const AxisEntry (*ax)[2 * K], int lane) {
    constexpr int KK = K * K, P = strip_pitch<K, QPW>();
    static_assert(P <= CELLS, "the output strip must fit in the wave's staged blocks");
    if constexpr (K == 9) {
        static_assert(QPW % 2 == 0, "the leftover rounds pair queries");
        constexpr int NL = QPW / 2;
        float res[QPW + NL];
        const int ti0 = lane >> 3, tj0 = lane & 7;
#pragma unroll
        for (int r = 0; r < QPW; ++r) res[r] = tap_one<K, STRIDE>(blk + r * CELLS, ax[r], ti0, tj0);
        const int l = lane & 31;
        const bool rowh = lane >= 32;                                   // upper half: the row tj = 8; lower half: the column ti = 8
        const int sl = rowh ? (l >= 9 ? 1 : 0) : ((l >> 3) & 1);        // which query of the pair
        const int ti = rowh ? min(l - 9 * sl, 8) : 8, tj = rowh ? 8 : (l & 7);   // (idle lanes repeat a live lane's tap)
        const bool live = rowh ? l < 18 : l < 16;
        const int ul = sl * P + (rowh ? 72 + ti : 64 + tj);
#pragma unroll
        for (int m = 0; m < NL; ++m) res[QPW + m] = tap_one<K, STRIDE>(blk + (2 * m + sl) * CELLS, ax[2 * m + sl], ti, tj);
        wave_lds_handover();   // every read of the staged blocks precedes the strip that overwrites them
#pragma unroll
        for (int r = 0; r < QPW; ++r) blk[r * P + lane] = res[r];
#pragma unroll
        for (int m = 0; m < NL; ++m)
            if (live) blk[2 * m * P + ul] = res[QPW + m];
    } else {
        constexpr int NPAIR = QPW * KK, NR = (NPAIR + 63) / 64;
        constexpr int D0 = 64 % K, D1 = (64 / K) % K, D2 = 64 / KK;     // 64 in base K
        float res[NR];
        int oaddr[NR];
        int s = lane / KK, ti = (lane - s * KK) / K, tj = lane - s * KK - ti * K;   // round 0 (constant divisors, lane < 64)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int sc = min(s, QPW - 1);                            // (lanes past the last pair repeat a tap of the last query)
            res[r] = tap_one<K, STRIDE>(blk + sc * CELLS, ax[sc], ti, tj);
            oaddr[r] = s < QPW ? s * P + ti * K + tj : -1;
            tj += D0;
            const int c0 = tj >= K ? 1 : 0;
            tj -= c0 * K;
            ti += D1 + c0;
            const int c1 = ti >= K ? 1 : 0;
            ti -= c1 * K;
            s += D2 + c1;
        }
        wave_lds_handover();
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (oaddr[r] >= 0) blk[oaddr[r]] = res[r];
    }
}

// ... and the transposed store: every channel row of the workgroup = QPB consecutive queries = one contiguous segment; the value of
// (row u, query c) is read from the strip of the wave that owns query c
template <int K, int QPW, int QPB, int BLK_STRIDE>
__device__ __forceinline__ void store_tokens(const float* smem, float* __restrict__ out, int b, int q0, int N1, int t) {
    constexpr int KK = K * K, P = strip_pitch<K, QPW>(), NTHR = 64 * (QPB / QPW);
    for (int idx = t; idx < KK * QPB; idx += NTHR) {
        const int u = idx / QPB, c = idx - u * QPB;
        if (q0 + c < N1) out[((size_t)b * KK + tap_channel<K>(u)) * N1 + q0 + c] = smem[(c / QPW) * BLK_STRIDE + (c % QPW) * P + u];
    }
}

// VT = float, or _Float16 for the Fast-mode volume that is STORED in the encoder's 16-bit type (mv_corr_volume_out16: what
// `einsum` returns when the encoder runs in fp16, Config/Experiment/MACVO/MACVO_Fast.yaml:73-74; flownet.py:27 only widens it): the cells
// are widened on load — exactly `cost_maps.float()` — and everything behind the load is the fp32 arithmetic of the fp32 form.
template <int R, int QPW, int QPB, typename VT = float>
__global__ __launch_bounds__(64 * (QPB / QPW)) void corr_lookup_kernel(const VT* __restrict__ vol,
                                                                        const float* __restrict__ coords,
                                                                        float* __restrict__ out, int N1, int H2, int W2) {
    constexpr int K = 2 * R + 1;
    constexpr int BS = K + 3;            // staged block edge (12 for r = 4)
    constexpr int CELLS = BS * BS + (K == 9 ? 2 : 0);   // floats per staged block: 144 cells (+ 2 for r = 4: consecutive blocks 18 banks apart, see tap_phase)
    constexpr int NWAVE = QPB / QPW;     // waves per workgroup, QPW queries each
    constexpr int RPR = 64 / BS;         // block rows one wave-wide load covers (5 for r = 4)
    constexpr int LPR = RPR * BS;        // active lanes of such a load (60)
    constexpr int NROUND = (BS + RPR - 1) / RPR;    // loads per query (3)
    // Round 3: the two MARGIN rows / columns of the block (index 0 and BS - 1) are read by a tap only when the fp32 normalise /
    // un-normalise round trip moves a sample across an integer, i.e. when the coordinate's fraction is within ~1e-4 of 0 (first
    // row / column) or of 1 (last).  They are fetched only then (threshold 1e-2, two orders of magnitude of slack); otherwise
    // the block's inner (BS - 2)^2 cells are everything a tap touches.  For r = 4 that is 10 rows = exactly two wave-wide loads
    // instead of three and 10-float row segments instead of 12: ~25 % fewer 32-B sectors per query for the HBM-bound batched
    // lookup (configs[4]: 882 -> ~680 B per query), one load round less for the latency-bound one.  Results unchanged bit for bit.
    constexpr bool TRIM = (BS - 2) % RPR == 0;      // inner rows are a whole number of wave-wide loads (r = 4: 10 = 2 x 5)
    constexpr int NINNER = (BS - 2) / RPR;          // ... this many
    constexpr int QPA = 64 / (2 * K);               // queries one axis pass covers (3 for r = 4)
    constexpr int APASS = (QPW + QPA - 1) / QPA;
    static_assert(QPW <= 32 && (QPW & (QPW - 1)) == 0 && QPB % QPW == 0, "bad lookup tiling");

    // one LDS region per WAVE, two lives: the wave's staged cell blocks (written and read by this wave only), then its output strip
    constexpr int BLK_STRIDE = wave_floats<K, QPW, CELLS>();
    __shared__ float smem[NWAVE * BLK_STRIDE];
    float* blk = smem + (threadIdx.x >> 6) * BLK_STRIDE;

    MV_SMALL_KERNEL_PRIO();
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * QPB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int slice = H2 * W2;

    // lane s < QPW owns query s of this wave: load its coords, derive the block origin
    const int qmine = q0 + wave * QPW + (lane & (QPW - 1));
    float x = 0.f, y = 0.f;
    if (qmine < N1) {
        x = coords[((size_t)b * 2 + 0) * N1 + qmine];
        y = coords[((size_t)b * 2 + 1) * N1 + qmine];
    }
    // clamp only the integer origin (NaN / huge coords must not produce wild addresses)
    const float xc = fminf(fmaxf(x, -1.0e6f), 1.0e6f), yc = fminf(fmaxf(y, -1.0e6f), 1.0e6f);
    const int bx = ((xc == xc) ? (int)floorf(xc) : 0) - R - 1;
    const int by = ((yc == yc) ? (int)floorf(yc) : 0) - R - 1;
    // margin flags of this lane's query: bit 0 first column, 1 last column, 2 first row, 3 last row (NaN: none — all taps are zero)
    const float frx = xc - floorf(xc), fry = yc - floorf(yc);
    const int margin = ((frx < 0.01f) ? 1 : 0) | ((frx > 0.99f) ? 2 : 0) | ((fry < 0.01f) ? 4 : 0) | ((fry > 0.99f) ? 8 : 0);

    // ---- stage QPW x CELLS cells: issue every load before touching LDS
    const int cyl = lane / BS, cxl = lane - cyl * BS;
    float v[QPW][NROUND];
#pragma unroll
    for (int s = 0; s < QPW; ++s) {
        const int sbx = __builtin_amdgcn_readlane(bx, s), sby = __builtin_amdgcn_readlane(by, s);
        const int q = q0 + wave * QPW + s;
        const VT* __restrict__ base = vol + ((size_t)b * N1 + q) * slice;
        const int gx = sbx + cxl;
        if (TRIM) {
            const int mg = __builtin_amdgcn_readlane(margin, s);                 // wave-uniform
            const bool okx = lane < LPR && q < N1 && gx >= 0 && gx < W2 && (cxl != 0 || (mg & 1)) && (cxl != BS - 1 || (mg & 2));
#pragma unroll
            for (int k = 0; k < NINNER; ++k) {                                   // inner rows 1 .. BS - 2
                const int row = 1 + k * RPR + cyl, gy = sby + row;
                const bool ok = okx && gy >= 0 && gy < H2;
                v[s][k] = ok ? (float)base[gy * W2 + gx] : 0.f;
            }
            v[s][NROUND - 1] = 0.f;
            if (mg & 12) {                                                       // rare: the margin rows, lanes [0, BS) row 0, [BS, 2 BS) row BS - 1
                const int row = cyl == 0 ? 0 : BS - 1, gy = sby + row;
                const bool ok = okx && cyl < 2 && ((mg >> (cyl == 0 ? 2 : 3)) & 1) && gy >= 0 && gy < H2;
                v[s][NROUND - 1] = ok ? (float)base[gy * W2 + gx] : 0.f;
            }
        } else {
            const bool okx = lane < LPR && q < N1 && gx >= 0 && gx < W2;
#pragma unroll
            for (int k = 0; k < NROUND; ++k) {
                const int row = k * RPR + cyl, gy = sby + row;
                const bool ok = okx && row < BS && gy >= 0 && gy < H2;
                v[s][k] = ok ? (float)base[gy * W2 + gx] : 0.f;
            }
        }
    }

    // ---- per-axis coordinate math (overlaps the loads in flight): lane -> (query sq of the pass, axis, offset)
    const float wm1 = (float)(W2 - 1), hm1 = (float)(H2 - 1);
    const int asq = lane / (2 * K), aa = lane - asq * (2 * K);
    const bool a_is_y = aa >= K;
    const int aoff = (a_is_y ? aa - K : aa) - R;
    const float adim = a_is_y ? hm1 : wm1;
    __shared__ AxisEntry ax_all[NWAVE][QPW][2 * K];
    AxisEntry (*ax)[2 * K] = ax_all[wave];
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
        const int s = ps * QPA + asq;   // lanes with s >= QPW compute garbage nobody keeps
        const float qx = __shfl(x, s, 64), qy = __shfl(y, s, 64);
        const int obx = __shfl(bx, s, 64), oby = __shfl(by, s, 64);
        const float cs = (a_is_y ? qy : qx) + (float)aoff;
        const float g = (2.f * cs) / adim - 1.f;          // RAFT bilinear_sampler normalisation
        const float ic = (g + 1.f) * (adim / 2.f);        // ATen grid_sampler_unnormalize, align_corners=True
        const float f0 = floorf(ic);
        const int c = (int)fminf(fmaxf(f0, -2.0e6f), 2.0e6f) - (a_is_y ? oby : obx);
        const bool inb = c >= 0 && c <= BS - 2;
        if (asq < QPA && s < QPW) ax[s][aa] = AxisEntry{ic - f0, min(max(c, 0), BS - 2) | (inb ? 256 : 0)};
    }

#pragma unroll
    for (int s = 0; s < QPW; ++s) {
        if (TRIM) {
#pragma unroll
            for (int k = 0; k < NINNER; ++k)
                if (lane < LPR) blk[s * CELLS + BS + k * LPR + lane] = v[s][k];                        // rows 1 + 5 k ..
            if (lane < 2 * BS) blk[s * CELLS + (lane < BS ? lane : (BS - 2) * BS + lane)] = v[s][NROUND - 1];   // rows 0 and BS - 1 (zeros unless fetched)
        } else {
#pragma unroll
            for (int k = 0; k < NROUND; ++k)
                if (lane < LPR && k * LPR + lane < BS * BS) blk[s * CELLS + k * LPR + lane] = v[s][k];
        }
    }
    // no workgroup barrier: the tap phase of a wave reads the blocks and axis entries that this same wave wrote
    wave_lds_handover();

    // ---- taps: (tap, query) pairs over the lanes, results into the wave's output strip
    tap_phase<K, QPW, BS, CELLS>(blk, ax, lane);
    __syncthreads();   // the kernel's only barrier: the transposed store reads every wave's strip

    // ---- transposed store: each channel row = QPB consecutive queries
    store_tokens<K, QPW, QPB, BLK_STRIDE>(smem, out, b, q0, N1, t);
}


// ---- the same lookup in a TILED volume (round 3): query q's slice is stored as 4 x 4-cell tiles,
//      vol[(b N1 + q) H2 W2 + (ty * W2/4 + tx) * 16 + (y % 4) * 4 + x % 4]   — what mv_corr_volume_packed writes when operand 2 was packed by
// mv_volume_pack_tiled (the GEMM itself is unchanged: only the order of its columns is).  A tile is one aligned 64-byte line, so the
// 10 x 10 (12 x 12 with margins) cell block of a query costs (10 + 3) / 4 = 3.25 tiles per axis = ~10.6 lines = 676 B instead of
// 10 row segments x 2.1 sectors of 32 B = 680 B in 21 separately addressed pieces: the same bytes in half as many, aligned, fully
// used DRAM bursts.  Staging: a wave-wide load = one tile row of the 4 x 4 tile grid that covers the block (lane = tile column x 16
// cells); tiles outside the needed cell range or the image are skipped / zero.  The staged block is 16 x 16 cells anchored at the
// first tile; axis math, tap phase and the transposed store are those of corr_lookup_kernel (r = 4 only), results bit-identical.
//
// VT = _Float16 (round 6): the Fast-mode volume's 2-byte cells in the same tile order (mv_fmap_tile_rows16 permutes operand 2's
// pixel rows in front of mv_corr_volume_out16).  A tile is then ONE aligned 32-byte sector: a query's block costs ~10.6 sectors = 338 B where
// the row-major fp16 volume costs 10 row segments of 20 B that straddle sectors (1.6 each: ~512 B).  Staging: a lane fetches two
// neighbouring cells as one dword, so a wave-wide load covers two tile rows and a query needs two loads; the cells are widened on load
// (`cost_maps.float()`, exact) and everything behind the load is the fp32 arithmetic above — tokens bit-identical to
// mv_corr_lookup_vol16 on the row-major volume.
template <int QPW, int QPB, typename VT = float>
__global__ __launch_bounds__(64 * (QPB / QPW)) void corr_lookup_tiled_kernel(const VT* __restrict__ vol,
                                                                              const float* __restrict__ coords,
                                                                              float* __restrict__ out, int N1, int H2, int W2) {
    constexpr int R = 4, K = 9;
    constexpr int BS = 16;                     // staged block: 4 x 4 tiles of 4 x 4 cells ...
    constexpr int BSP = 20, CELLS = BS * BSP + 18;  // ... at a row stride of 20 floats, blocks 18 banks apart: 4 x 8 taps of a query cover the 32 banks once (tap_phase)
    constexpr int NWAVE = QPB / QPW;
    constexpr int QPA = 64 / (2 * K);
    constexpr int APASS = (QPW + QPA - 1) / QPA;
    constexpr int BLK_STRIDE = wave_floats<K, QPW, CELLS>();
    __shared__ __attribute__((aligned(16))) float smem[NWAVE * BLK_STRIDE];   // per wave: its staged blocks, then its output strip
    float* blk = smem + (threadIdx.x >> 6) * BLK_STRIDE;

    MV_SMALL_KERNEL_PRIO();
    const int b = blockIdx.y;
    const int q0 = blockIdx.x * QPB;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tpr = W2 >> 2, tpc = (H2 + 3) >> 2, slice = tpc * tpr * 16;   // (fp16 cells: H2 need not be a multiple of 4 — the last tile row is padded with zero cells)

    const int qmine = q0 + wave * QPW + (lane & (QPW - 1));
    float x = 0.f, y = 0.f;
    if (qmine < N1) {
        x = coords[((size_t)b * 2 + 0) * N1 + qmine];
        y = coords[((size_t)b * 2 + 1) * N1 + qmine];
    }
    const float xc = fminf(fmaxf(x, -1.0e6f), 1.0e6f), yc = fminf(fmaxf(y, -1.0e6f), 1.0e6f);
    const int bx = ((xc == xc) ? (int)floorf(xc) : 0) - R - 1;      // origin of the 12 x 12 cell block of corr_lookup_kernel
    const int by = ((yc == yc) ? (int)floorf(yc) : 0) - R - 1;
    const float frx = xc - floorf(xc), fry = yc - floorf(yc);
    const int x_lo = bx + ((frx < 0.01f) ? 0 : 1), x_hi = bx + ((frx > 0.99f) ? K + 2 : K + 1);   // cells a tap can touch (see TRIM above)
    const int y_lo = by + ((fry < 0.01f) ? 0 : 1), y_hi = by + ((fry > 0.99f) ? K + 2 : K + 1);
    const int tox = bx >> 2, toy = by >> 2;                          // first tile (floor division: arithmetic shift)

    // ---- stage.  fp32 cells: per query four wave-wide loads (tile rows), lane = (tile column, cell).  fp16 cells: two loads of two tile
    //      rows each, lane = (tile row of the pair, tile column, cell pair)
    constexpr bool H16 = sizeof(VT) == 2;
    constexpr int NLD = H16 ? 2 : 4;
    const int ti = H16 ? (lane >> 3) & 3 : lane >> 4, cell = H16 ? (lane & 7) * 2 : lane & 15;
    const int half_row = H16 ? lane >> 5 : 0;
    float v[QPW][4];
#pragma unroll
    for (int s = 0; s < QPW; ++s) {
        const int stx = __builtin_amdgcn_readlane(tox, s), sty = __builtin_amdgcn_readlane(toy, s);
        const int sxl = __builtin_amdgcn_readlane(x_lo, s), sxh = __builtin_amdgcn_readlane(x_hi, s);
        const int syl = __builtin_amdgcn_readlane(y_lo, s), syh = __builtin_amdgcn_readlane(y_hi, s);
        const int q = q0 + wave * QPW + s;
        const VT* __restrict__ base = vol + ((size_t)b * N1 + q) * slice;
        const int tx = stx + ti;
        const bool okx = q < N1 && tx >= 0 && tx < tpr && 4 * tx + 3 >= sxl && 4 * tx <= sxh;
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            const int ty = sty + (H16 ? 2 * k + half_row : k);
            const bool ok = okx && ty >= 0 && ty < tpc && 4 * ty + 3 >= syl && 4 * ty <= syh;
            if constexpr (H16) {
                union { uint32_t u; _Float16 h[2]; } two;
                two.u = ok ? *reinterpret_cast<const uint32_t*>(base + ((ty * tpr + tx) << 4) + cell) : 0u;
                v[s][2 * k] = (float)two.h[0];
                v[s][2 * k + 1] = (float)two.h[1];
            } else {
                v[s][k] = ok ? (float)base[((ty * tpr + tx) << 4) + cell] : 0.f;
            }
        }
    }

    // ---- per-axis coordinate math (as corr_lookup_kernel; cell offsets relative to the first tile)
    const float wm1 = (float)(W2 - 1), hm1 = (float)(H2 - 1);
    const int asq = lane / (2 * K), aa = lane - asq * (2 * K);
    const bool a_is_y = aa >= K;
    const int aoff = (a_is_y ? aa - K : aa) - R;
    const float adim = a_is_y ? hm1 : wm1;
    __shared__ AxisEntry ax_all[NWAVE][QPW][2 * K];
    AxisEntry (*ax)[2 * K] = ax_all[wave];
#pragma unroll
    for (int ps = 0; ps < APASS; ++ps) {
        const int s = ps * QPA + asq;
        const float qx = __shfl(x, s, 64), qy = __shfl(y, s, 64);
        const int obx = __shfl(tox, s, 64) * 4, oby = __shfl(toy, s, 64) * 4;
        const float cs = (a_is_y ? qy : qx) + (float)aoff;
        const float g = (2.f * cs) / adim - 1.f;
        const float ic = (g + 1.f) * (adim / 2.f);
        const float f0 = floorf(ic);
        const int c = (int)fminf(fmaxf(f0, -2.0e6f), 2.0e6f) - (a_is_y ? oby : obx);
        const bool inb = c >= 0 && c <= BS - 2;
        if (asq < QPA && s < QPW) ax[s][aa] = AxisEntry{ic - f0, min(max(c, 0), BS - 2) | (inb ? 256 : 0)};
    }

#pragma unroll
    for (int s = 0; s < QPW; ++s)
#pragma unroll
        for (int k = 0; k < NLD; ++k) {
            if constexpr (H16)      // the pair sits in one cell row of the tile, at an even column: one 8-byte LDS write
                *reinterpret_cast<float2*>(&blk[s * CELLS + (4 * (2 * k + half_row) + (cell >> 2)) * BSP + 4 * ti + (cell & 3)]) =
                    make_float2(v[s][2 * k], v[s][2 * k + 1]);
            else
                blk[s * CELLS + (4 * k + (cell >> 2)) * BSP + 4 * ti + (cell & 3)] = v[s][k];
        }
    wave_lds_handover();   // (wave-local, as in corr_lookup_kernel)

    tap_phase<K, QPW, BSP, CELLS>(blk, ax, lane);
    __syncthreads();
    store_tokens<K, QPW, QPB, BLK_STRIDE>(smem, out, b, q0, N1, t);
}

}  // namespace

// queries-per-launch at or below which the 16-wave variant is used; MV_LOOKUP_SMALL=<n> overrides it for A/B runs
// (tools/kernel_bench.py), e.g. 0 forces the 4-wave variant
#include <stdlib.h>
static int lookup_small_threshold() {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("MV_LOOKUP_SMALL");
        v = e ? atoi(e) : 65536;
    }
    return v;
}

// small launches (one frame: 9600 queries for 256 CUs) are latency-bound -> 16-query workgroups of 8 waves (600
// workgroups, 5.96 us vs 7.15 us for 32-query ones); large batches (B = 32: 58.5 us, ~2.4 TB/s) are throughput-bound ->
// 4 queries per wave amortise the per-wave setup, 32-query (128-B) output segments
template <auto SMALL, auto LARGE, typename VT>
static void launch_lookup(bool small, const VT* vol, const float* coords, float* out, int B, int N1, int H2, int W2, hipStream_t s) {
    if (small)
        hipLaunchKernelGGL(SMALL, dim3(mv_ceil_div(N1, 16), B), dim3(512), 0, s, vol, coords, out, N1, H2, W2);
    else
        hipLaunchKernelGGL(LARGE, dim3(mv_ceil_div(N1, 32), B), dim3(512), 0, s, vol, coords, out, N1, H2, W2);
}

static int lookup_small_qpb() {
    static int small_qpb = -1;   // MV_LOOKUP_QPB=8: 256-thread workgroups of 8 queries (A/B knob for the co-running case)
    if (small_qpb < 0) { const char* e = getenv("MV_LOOKUP_QPB"); small_qpb = (e && atoi(e) == 8) ? 8 : 16; }
    return small_qpb;
}

// row-major fp32 cells, any radius
template <int R>
static void launch_lookup_f32(bool small, const float* vol, const float* coords, float* out, int B, int N1, int H2, int W2, hipStream_t s) {
    if (small && lookup_small_qpb() == 8)
        hipLaunchKernelGGL((corr_lookup_kernel<R, 2, 8>), dim3(mv_ceil_div(N1, 8), B), dim3(256), 0, s, vol, coords, out, N1, H2, W2);
    else
        launch_lookup<corr_lookup_kernel<R, 2, 16>, corr_lookup_kernel<R, 4, 32>>(small, vol, coords, out, B, N1, H2, W2, s);
}

// The window lookup on any of the four volume forms.  cells16: the volume is stored as fp16 (mv_corr_volume_out16): half the bytes per cell; tokens are
// fp32.  tiled: its slices are stored in 4 x 4-cell tiles (fp32: mv_volume_pack_tiled + mv_corr_volume_packed; fp16: mv_fmap_tile_rows16 on operand 2 +
// mv_corr_volume_out16).  Row-major fp32 takes radius 1..4, the other forms radius 4; tiles need W2 (fp32: and H2) a multiple of 4.
int mv_lookup(const void* vol, bool cells16, bool tiled, const float* coords, float* out, int B, int H1, int W1, int H2, int W2, int radius,
              mvStream_t stream) {
    MV_CHECK_ARG(vol && coords && out);
    MV_CHECK_ARG(B > 0 && H1 > 0 && W1 > 0 && H2 > 1 && W2 > 1);
    MV_CHECK_ARG(!(tiled && cells16) || ((uintptr_t)vol & 31) == 0);     // a tile = one 32-byte sector
    if (radius > 4 || radius < (cells16 || tiled ? 4 : 1) || B > 65535) return MV_ERR_UNSUPPORTED;
    if (tiled && ((W2 % 4) || (!cells16 && (H2 % 4)))) return MV_ERR_UNSUPPORTED;
    const int N1 = H1 * W1;
    hipStream_t s = (hipStream_t)stream;
    const bool small = (size_t)B * N1 <= (size_t)lookup_small_threshold();
    const float* v32 = reinterpret_cast<const float*>(vol);
    const _Float16* v16 = reinterpret_cast<const _Float16*>(vol);
    if (!cells16 && !tiled) {
        switch (radius) {
            case 1: launch_lookup_f32<1>(small, v32, coords, out, B, N1, H2, W2, s); break;
            case 2: launch_lookup_f32<2>(small, v32, coords, out, B, N1, H2, W2, s); break;
            case 3: launch_lookup_f32<3>(small, v32, coords, out, B, N1, H2, W2, s); break;
            default: launch_lookup_f32<4>(small, v32, coords, out, B, N1, H2, W2, s); break;
        }
    } else if (!tiled) {
        launch_lookup<corr_lookup_kernel<4, 2, 16, _Float16>, corr_lookup_kernel<4, 4, 32, _Float16>>(small, v16, coords, out, B, N1, H2, W2, s);
    } else if (!cells16) {
        launch_lookup<corr_lookup_tiled_kernel<2, 16>, corr_lookup_tiled_kernel<4, 32>>(small, v32, coords, out, B, N1, H2, W2, s);
    } else {
        launch_lookup<corr_lookup_tiled_kernel<2, 16, _Float16>, corr_lookup_tiled_kernel<4, 32, _Float16>>(small, v16, coords, out, B, N1, H2, W2, s);
    }
    return mv_launch_status();
}

extern "C" int mv_corr_lookup(const float* vol, const float* coords, float* out, int B, int H1, int W1,
                              int H2, int W2, int radius, mvStream_t stream) {
    return mv_lookup(vol, false, false, coords, out, B, H1, W1, H2, W2, radius, stream);
}

extern "C" int mv_corr_lookup_vol16(const void* vol, const float* coords, float* out, int B, int H1, int W1, int H2, int W2, int radius,
                                    mvStream_t stream) {
    return mv_lookup(vol, true, false, coords, out, B, H1, W1, H2, W2, radius, stream);
}

extern "C" int mv_corr_lookup_tiled(const float* vol, const float* coords, float* out, int B, int H1, int W1, int H2, int W2,
                                    int radius, mvStream_t stream) {
    return mv_lookup(vol, false, true, coords, out, B, H1, W1, H2, W2, radius, stream);
}

extern "C" int mv_corr_lookup_tiled_vol16(const void* vol, const float* coords, float* out, int B, int H1, int W1, int H2, int W2, int radius,
                                          mvStream_t stream) {
    return mv_lookup(vol, true, true, coords, out, B, H1, W1, H2, W2, radius, stream);
}

// The pixel rows of a 16-bit HWC feature map [B, H, W, C] in 4 x 4-tile order: out[b][(ty * W/4 + tx) * 16 + (y % 4) * 4 + x % 4][:] =
// f[b][y * W + x][:], ceil(H / 4) tile rows — rows y >= H of the last one are ZERO pixels, so out is [B, mv_tiled_slice_cells(H, W), C].  As
// operand 2 of mv_corr_volume_out16 (N2 = that many) it makes the unchanged GEMM write every query's slice tiled (each output element is the
// same k-ordered sum wherever its column sits; the padding cells come out as exact zeros = the lookup's zero padding) — the 16-bit twin of
// mv_volume_pack_tiled's permutation.  One 16-byte chunk per thread.
namespace {
__global__ __launch_bounds__(256) void fmap_tile_rows16_kernel(const uint4* __restrict__ f, uint4* __restrict__ out, int H, int W, int n_out, int cpr, size_t total) {
    const int tpr = W >> 2;
    const size_t n_in = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t rowi = i / cpr;
        const int ch = (int)(i - rowi * cpr);
        const size_t b = rowi / n_out;
        const int j = (int)(rowi - b * n_out);
        const int tile = j >> 4, cell = j & 15;
        const int ty = tile / tpr, tx = tile - ty * tpr;
        const int y = 4 * ty + (cell >> 2);
        out[i] = y < H ? f[(b * n_in + (size_t)y * W + 4 * tx + (cell & 3)) * cpr + ch] : make_uint4(0u, 0u, 0u, 0u);
    }
}
}  // namespace

extern "C" int mv_tiled_slice_cells(int H, int W) { return (H > 0 && W > 0 && (W % 4) == 0) ? ((H + 3) / 4) * 4 * W : 0; }

extern "C" int mv_fmap_tile_rows16(const void* f, void* out, int B, int C, int H, int W, mvStream_t stream) {
    MV_CHECK_ARG(f && out && f != out && B > 0 && C > 0 && H > 0 && W > 0);
    MV_CHECK_ARG(((uintptr_t)f & 15) == 0 && ((uintptr_t)out & 15) == 0);
    if ((C % 8) || (W % 4)) return MV_ERR_UNSUPPORTED;
    const int cpr = C / 8, n_out = mv_tiled_slice_cells(H, W);
    const size_t total = (size_t)B * n_out * cpr;
    const int blocks = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(fmap_tile_rows16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const uint4*)f, (uint4*)out, H, W, n_out, cpr, total);
    return mv_launch_status();
}
