// Training form of the fused flow embedding (include/deepclr_amd_flow_train.h), f32, layers 2 and 3 on
// v_mfma_f32_16x16x4_f32.
//
// The composed training path gathers every neighbourhood into a (B, 131, P0, k) tensor and keeps the layer input and all
// three activations for autograd. The max over the k neighbours passes gradient to one slot per (template point,
// channel), so the backward needs only that slot and can rebuild the rest:
//
//   pre       pt = W1t feat0, ps = W1s feat1 per point (layer 1 by linearity, as csrc/flow.hip), kept for the backward.
//   forward   flow.hip's f32 layout: 4 template points per workgroup, MFMA row tile t holds neighbours 4t..4t+3 of the
//             4 points, so lane-quarter p holds point p and the max over the neighbours is a register maximum; here it
//             also keeps the first slot that reaches it. Output: pooled (B, 256, P0) and that slot per channel.
//   backward  one workgroup per 160th of the blocks of template points (G = floor(80 / k) points, G * k <= 80 rows per
//             block, five 16-row tiles). Per block: rebuild a1 and a2 with the forward's operations; dA2 = dZ3 W3 from
//             the sparse dZ3 (grad_pooled at the argmax rows); dZ2; dW2 += dZ2^T a1 and dA1 = dZ2 W2 on MFMA; dZ1;
//             dW1 += dZ1^T [pos_diff | feat0 | feat1 | 1] on MFMA (the ones column is db1); then, when the clouds
//             need gradients, E = dZ1 W1 on MFMA: the template terms summed over the block's slots, the source terms
//             stored per (p, j). dW3 += g a2[argmax] runs in a kernel of its own over the same blocks (on the VALU;
//             its 128 accumulators per thread beside the MFMA ones would spill). Every workgroup writes its partial
//             weight gradients; a third kernel adds them in workgroup order. Source points: a counting sort of idx
//             (integer atomics that only count), each bucket sorted ascending, then summed in that order.
// No float atomics: the same inputs give bit-identical gradients on every run. The layer-1 chain and the MFMA calls of
// the backward's rebuild are the forward's (-ffp-contract=off, explicit fmaf), so it sees exactly the forward's a1, a2.
#include "mma.h"
#include "../../include/deepclr_amd_flow_train.h"

namespace {

constexpr int FT_F = 64;                        // features per cloud row
constexpr int FT_ROW = 3 + FT_F;                // 67: cloud row [x y z | features]
constexpr int FT_IN = 3 + 2 * FT_F;             // 131
constexpr int FT_C = 128;                       // width of layers 1 and 2
constexpr int FT_OUT = 256;
constexpr int O_W1 = 0;
constexpr int O_B1 = O_W1 + FT_C * FT_IN;       // 16768
constexpr int O_W2 = O_B1 + FT_C;               // 16896
constexpr int O_B2 = O_W2 + FT_C * FT_C;        // 33280
constexpr int O_W3 = O_B2 + FT_C;               // 33408
constexpr int O_B3 = O_W3 + FT_OUT * FT_C;      // 66176
constexpr int O_GRAD = O_B3 + FT_OUT;           // 66432
constexpr int O_W2T = O_GRAD;
constexpr int FT_XP = 144;                      // X columns padded to 9 tiles of 16 (column 131: the ones of db1)
constexpr int O_W1T = O_W2T + FT_C * FT_C;      // 82816
constexpr int O_MLP = O_W1T + FT_XP * FT_C;     // 101248
static_assert(O_GRAD == DCLR_FLOW_TRAIN_GRAD_FLOATS && O_MLP == DCLR_FLOW_TRAIN_MLP_FLOATS, "weight packing");

constexpr int FW_G = 4;                         // forward: template points per workgroup
constexpr int FW_STRIDE = dclr_lds_stride(FT_C);   // 132

constexpr int BW_T = 5;                         // backward: row tiles per block
constexpr int BW_R = BW_T * 16;                 // 80 rows
constexpr int BW_S = dclr_lds_stride(FT_XP);    // 148
constexpr int BW_MAX_WG = 160;
constexpr int E_W = 68;                         // per (p, j) source term: W1a^T dZ1 (3), W1s^T dZ1 (64), pad

__device__ __forceinline__ int clamp_src(int s, int n) { return s < 0 ? 0 : (s >= n ? n - 1 : s); }

// Weights of 16-column tiles u (columns n0 + u * nstep + c16) of a row-major (N x ld) matrix for k-group g, in the
// operand order of dclr_mma16_step: the float4 at row n, columns 16g + 4kq .. + 3.
template <int NT>
__device__ __forceinline__ void load_b(float4 (&b)[NT], const float *w, int ld, int n0, int nstep, int g, int c16,
                                       int kq) {
#pragma unroll
    for (int u = 0; u < NT; ++u)
        b[u] = *reinterpret_cast<const float4 *>(w + (size_t)(n0 + u * nstep + c16) * ld + 16 * g + 4 * kq);
}

// acc[t][u] (rows 16t.., columns n0 + u * nstep ..) = a_tile (rows x 128) times W^T, W row-major (N x 128): the call
// sequence the forward and the backward's rebuild share.
template <int T, int NT>
__device__ __forceinline__ void mma_rows_wt(dclr_f32x4 (&acc)[T][NT], const float *tile, int stride, const float *w,
                                            int n0, int nstep, int lane) {
    const int kq = lane >> 4, c16 = lane & 15;
    const float *a_lds = tile + c16 * stride + 4 * kq;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = 0.f;
#pragma unroll 1                                // rolled: the backward keeps its gradient accumulators live
    for (int g = 0; g < FT_C / 16; ++g) {
        float4 b[NT];
        load_b<NT>(b, w, FT_C, n0, nstep, g, c16, kq);
        dclr_mma16_step<T, NT>(acc, a_lds, stride, g, b);
    }
}

// Layer 1 of one (template, source) row for this lane's two channels: the order of operations of csrc/flow.hip.
__device__ __forceinline__ float2 layer1(float2 ptv, float2 bv, float2 psv, float wa0, float wa1, float wa2, float wb0,
                                         float wb1, float wb2, float dx, float dy, float dz) {
    const float base0 = ptv.x + bv.x, base1 = ptv.y + bv.y;
    float v0 = base0 + psv.x, v1 = base1 + psv.y;
    v0 = fmaf(wa0, dx, v0); v0 = fmaf(wa1, dy, v0); v0 = fmaf(wa2, dz, v0);
    v1 = fmaf(wb0, dx, v1); v1 = fmaf(wb1, dy, v1); v1 = fmaf(wb2, dz, v1);
    return make_float2(fmaxf(v0, 0.f), fmaxf(v1, 0.f));
}

// pt (rows of cloud0) and ps (rows of cloud1): thread = (row, channel), an fmaf chain over the 64 features.
__global__ __launch_bounds__(256) void flow_train_pre_kernel(long long rows0, long long rows1,
                                                             const float *__restrict__ cloud0,
                                                             const float *__restrict__ cloud1,
                                                             const float *__restrict__ weights, float *__restrict__ pt,
                                                             float *__restrict__ ps) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = e >> 7;
    const int c = (int)(e & (FT_C - 1));
    if (row >= rows0 + rows1) return;
    const bool tmpl = row < rows0;
    const long long r = tmpl ? row : row - rows0;
    const float *x = (tmpl ? cloud0 : cloud1) + r * FT_ROW + 3;
    const float *w = weights + O_W1 + (size_t)c * FT_IN + (tmpl ? 3 : 3 + FT_F);
    float z = 0.f;
#pragma unroll 16
    for (int i = 0; i < FT_F; ++i) z = fmaf(w[i], x[i], z);
    (tmpl ? pt : ps)[r * FT_C + c] = z;
}

// T = ceil(k / 4) row tiles of 16 rows.
template <int T>
__global__ __launch_bounds__(256) void flow_train_fwd_kernel(int pairs, int n0, int n1, int k, float radius,
                                                             const float *__restrict__ cloud0,
                                                             const float *__restrict__ cloud1,
                                                             const int32_t *__restrict__ idx,
                                                             const float *__restrict__ weights,
                                                             const float *__restrict__ pt,
                                                             const float *__restrict__ ps, float *__restrict__ pooled,
                                                             int32_t *__restrict__ arg) {
    __shared__ __attribute__((aligned(16))) float tile[T * 16 * FW_STRIDE];
    __shared__ uint32_t vbits[FW_G];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, c16 = lane & 15;
    const size_t total = (size_t)pairs * n0;
    const size_t g0 = (size_t)blockIdx.x * FW_G;
    const float *w1 = weights + O_W1;

    // ---- phase A: wave w builds the layer-1 rows of template point g0 + w ---------------------------
    {
        const int p = wave;
        const size_t gp = g0 + p;
        uint32_t bits = 0;
        int s_done = 0;
        if (gp < total) {                                               // wave-uniform
            const size_t pair = gp / n0;
            const float *trow = cloud0 + gp * FT_ROW;
            const float tx = trow[0], ty = trow[1], tz = trow[2];
            const float2 ptv = *reinterpret_cast<const float2 *>(pt + gp * FT_C + 2 * lane);
            const float2 bv = *reinterpret_cast<const float2 *>(weights + O_B1 + 2 * lane);
            const float wa0 = w1[(2 * lane) * FT_IN + 0], wa1 = w1[(2 * lane) * FT_IN + 1],
                        wa2 = w1[(2 * lane) * FT_IN + 2];
            const float wb0 = w1[(2 * lane + 1) * FT_IN + 0], wb1 = w1[(2 * lane + 1) * FT_IN + 1],
                        wb2 = w1[(2 * lane + 1) * FT_IN + 2];
            const int raw_nb = lane < k ? idx[gp * k + lane] : 0;
            const uint32_t filled = (uint32_t)__ballot(lane < k && raw_nb >= 0 && raw_nb < n1);
            const int my_nb = clamp_src(raw_nb, n1);
            const size_t src0 = pair * (size_t)n1;
            for (int s = 0; s < k; ++s) {
                const int nb = __builtin_amdgcn_readlane(my_nb, s);
                const float *srow = cloud1 + (src0 + nb) * FT_ROW;
                const float dx = srow[0] - tx, dy = srow[1] - ty, dz = srow[2] - tz;
                const float2 psv = *reinterpret_cast<const float2 *>(ps + (src0 + nb) * FT_C + 2 * lane);
                const int row = (s >> 2) * 16 + 4 * p + (s & 3);
                *reinterpret_cast<float2 *>(&tile[row * FW_STRIDE + 2 * lane]) =
                    layer1(ptv, bv, psv, wa0, wa1, wa2, wb0, wb1, wb2, dx, dy, dz);
                const float norm = sqrtf(dx * dx + dy * dy + dz * dz);
                if (!(radius > 0.f) || norm < radius) bits |= 1u << s;
            }
            bits &= filled;
            s_done = k;
        }
        for (int s = s_done; s < 4 * T; ++s) {                          // padding rows (k % 4 != 0, or no point)
            const int row = (s >> 2) * 16 + 4 * p + (s & 3);
            *reinterpret_cast<float2 *>(&tile[row * FW_STRIDE + 2 * lane]) = make_float2(0.f, 0.f);
        }
        if (lane == 0) vbits[p] = bits;
    }
    __syncthreads();

    // ---- phase B: layer 2 (128 -> 128), wave w owns channels 32w .. 32w + 31 ------------------------
    {
        dclr_f32x4 acc[T][2];
        mma_rows_wt<T, 2>(acc, tile, FW_STRIDE, weights + O_W2, 32 * wave, 16, lane);
        __syncthreads();                                   // every wave has consumed the layer-1 rows
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = 32 * wave + 16 * u + c16;
            const float bv = weights[O_B2 + col];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) tile[(t * 16 + 4 * kq + i) * FW_STRIDE + col] = fmaxf(acc[t][u][i] + bv, 0.f);
        }
    }
    __syncthreads();

    // ---- phase C: layer 3 (128 -> 256) + mask + max and first argmax; wave w owns channels 64w .. 64w + 63
    {
        dclr_f32x4 acc[T][4];
        mma_rows_wt<T, 4>(acc, tile, FW_STRIDE, weights + O_W3, 64 * wave, 16, lane);
        const uint32_t vb = vbits[kq];                     // lane-quarter kq holds template point kq
        const size_t gp = g0 + kq;
        const size_t pair = gp / n0, p = gp % n0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = 64 * wave + 16 * u + c16;
            const float bv = weights[O_B3 + col];
            float mx = 0.f;                                // ReLU floor; masked rows contribute 0
            int slot = 0;
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = acc[t][u][i] + bv;     // row 4 * kq + i of tile t: neighbour 4t + i (ascending)
                    if (((vb >> (4 * t + i)) & 1u) && v > mx) {
                        mx = v;
                        slot = 4 * t + i;
                    }
                }
            if (gp < total) {
                const size_t o = (pair * FT_OUT + col) * n0 + p;
                pooled[o] = mx;
                arg[o] = slot;
            }
        }
    }
}

struct BwdArgs {
    int pairs, n0, n1, k, g, chunks_per_pair, chunks, input_grads;
};

// Rows r = pl * k + j of a block (template p0 + pl, slot j; rows past G * k or past n0 are zero): a1 into `a1t` with
// the forward's layer-1 chain, the global template / source row and pos_diff of each row into the bookkeeping arrays.
__device__ __forceinline__ void rebuild_a1(const BwdArgs &a, int pair, int p0, const float *cloud0, const float *cloud1,
                                           const int32_t *idx, const float *weights, const float *pt, const float *ps,
                                           float *a1t, long long *rowp, long long *rows_src, float *posd, int wave,
                                           int lane) {
    const int k = a.k, n0 = a.n0, n1 = a.n1, R = a.g * k;
    const float *w1 = weights + O_W1;
    const float2 bv = *reinterpret_cast<const float2 *>(weights + O_B1 + 2 * lane);
    const float wa0 = w1[(2 * lane) * FT_IN + 0], wa1 = w1[(2 * lane) * FT_IN + 1], wa2 = w1[(2 * lane) * FT_IN + 2];
    const float wb0 = w1[(2 * lane + 1) * FT_IN + 0], wb1 = w1[(2 * lane + 1) * FT_IN + 1],
                wb2 = w1[(2 * lane + 1) * FT_IN + 2];
    for (int r = wave; r < BW_R; r += 4) {
        const int pl = r / k, j = r % k, p = p0 + pl;
        float2 v = make_float2(0.f, 0.f);
        if (r < R && p < n0) {                                         // wave-uniform
            const size_t gp = (size_t)pair * n0 + p;
            const int nb = clamp_src(idx[gp * k + j], n1);
            const size_t src = (size_t)pair * n1 + nb;
            const float *trow = cloud0 + gp * FT_ROW, *srow = cloud1 + src * FT_ROW;
            const float dx = srow[0] - trow[0], dy = srow[1] - trow[1], dz = srow[2] - trow[2];
            const float2 ptv = *reinterpret_cast<const float2 *>(pt + gp * FT_C + 2 * lane);
            const float2 psv = *reinterpret_cast<const float2 *>(ps + src * FT_C + 2 * lane);
            v = layer1(ptv, bv, psv, wa0, wa1, wa2, wb0, wb1, wb2, dx, dy, dz);
            if (lane == 0) {
                rowp[r] = (long long)gp;
                rows_src[r] = (long long)src;
                posd[r * 3 + 0] = dx;
                posd[r * 3 + 1] = dy;
                posd[r * 3 + 2] = dz;
            }
        } else if (lane == 0) {
            rowp[r] = -1;
            rows_src[r] = 0;
            posd[r * 3 + 0] = posd[r * 3 + 1] = posd[r * 3 + 2] = 0.f;
        }
        *reinterpret_cast<float2 *>(&a1t[r * BW_S + 2 * lane]) = v;
    }
}

// a2 = ReLU(W2 a1 + b2) of the block, wave w channels 32w .. 32w + 31; a2t may be a1t (then after a barrier).
__device__ __forceinline__ void rebuild_a2(const float *weights, const float *a1t, float *a2t, int wave, int lane) {
    const int kq = lane >> 4, c16 = lane & 15;
    dclr_f32x4 acc[BW_T][2];
    mma_rows_wt<BW_T, 2>(acc, a1t, BW_S, weights + O_W2, 32 * wave, 16, lane);
    if (a2t == a1t) __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int col = 32 * wave + 16 * u + c16;
        const float b2 = weights[O_B2 + col];
#pragma unroll
        for (int t = 0; t < BW_T; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) a2t[(t * 16 + 4 * kq + i) * BW_S + col] = fmaxf(acc[t][u][i] + b2, 0.f);
    }
}

// dW3 += g a2[argmax row]^T and db3 over the same blocks and workgroups as flow_train_bwd_kernel: thread = channel,
// written to the W3 / b3 part of this workgroup's partial (the other kernel writes the rest).
__global__ __launch_bounds__(256) void flow_train_bwd3_kernel(BwdArgs a, const float *__restrict__ cloud0,
                                                              const float *__restrict__ cloud1,
                                                              const int32_t *__restrict__ idx,
                                                              const float *__restrict__ weights,
                                                              const float *__restrict__ pt,
                                                              const float *__restrict__ ps,
                                                              const float *__restrict__ pooled,
                                                              const int32_t *__restrict__ arg,
                                                              const float *__restrict__ gpool,
                                                              float *__restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float L[BW_R * BW_S];
    __shared__ long long rowp[BW_R], rows_src[BW_R];
    __shared__ float posd[BW_R * 3];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = a.k, n0 = a.n0, G = a.g, c = tid;
    float acc3[FT_C];
    float db3 = 0.f;
#pragma unroll
    for (int n = 0; n < FT_C; ++n) acc3[n] = 0.f;
    for (int ch = blockIdx.x; ch < a.chunks; ch += gridDim.x) {
        const int pair = ch / a.chunks_per_pair, p0 = (ch % a.chunks_per_pair) * G;
        rebuild_a1(a, pair, p0, cloud0, cloud1, idx, weights, pt, ps, L, rowp, rows_src, posd, wave, lane);
        __syncthreads();
        rebuild_a2(weights, L, L, wave, lane);
        __syncthreads();
        for (int pl = 0; pl < G && p0 + pl < n0; ++pl) {
            const size_t o = ((size_t)pair * FT_OUT + c) * n0 + p0 + pl;
            if (pooled[o] > 0.f) {
                const float g = gpool[o];
                const float *a2 = &L[(pl * k + min(max(arg[o], 0), k - 1)) * BW_S];
#pragma unroll
                for (int n4 = 0; n4 < FT_C / 4; ++n4) {
                    const float4 v = *reinterpret_cast<const float4 *>(a2 + 4 * n4);
                    acc3[4 * n4 + 0] = fmaf(g, v.x, acc3[4 * n4 + 0]);
                    acc3[4 * n4 + 1] = fmaf(g, v.y, acc3[4 * n4 + 1]);
                    acc3[4 * n4 + 2] = fmaf(g, v.z, acc3[4 * n4 + 2]);
                    acc3[4 * n4 + 3] = fmaf(g, v.w, acc3[4 * n4 + 3]);
                }
                db3 += g;
            }
        }
        __syncthreads();
    }
    float *out = partial + (size_t)blockIdx.x * O_GRAD;
#pragma unroll
    for (int n = 0; n < FT_C; ++n) out[O_W3 + c * FT_C + n] = acc3[n];
    out[O_B3 + c] = db3;
}

__global__ __launch_bounds__(256, 1) void flow_train_bwd_kernel(BwdArgs a, const float *__restrict__ cloud0,
                                                                const float *__restrict__ cloud1,
                                                                const int32_t *__restrict__ idx,
                                                                const float *__restrict__ weights,
                                                                const float *__restrict__ pt,
                                                                const float *__restrict__ ps,
                                                                const float *__restrict__ pooled,
                                                                const int32_t *__restrict__ arg,
                                                                const float *__restrict__ gpool,
                                                                float *__restrict__ partial, float *__restrict__ erows,
                                                                float *__restrict__ grad0) {
    __shared__ __attribute__((aligned(16))) float L1[BW_R * BW_S];   // a1, then X = [pos_diff | feat0 | feat1 | 1]
    __shared__ __attribute__((aligned(16))) float L2[BW_R * BW_S];   // a2, then dZ1
    __shared__ __attribute__((aligned(16))) float L3[BW_R * BW_S];   // dA2 -> dZ2, then E = dZ1 W1
    __shared__ long long rowp[BW_R];                                 // global template row of each block row, -1: none
    __shared__ long long rows_src[BW_R];                             // global source row
    __shared__ float posd[BW_R * 3];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kq = lane >> 4, c16 = lane & 15;
    const int k = a.k, n0 = a.n0, G = a.g, R = G * k;

    dclr_f32x4 acc2[2][8];                      // dW2: rows (2 * wave + m) * 16 .., columns t * 16 ..
    dclr_f32x4 acc1[2][9];                      // dW1 | db1: rows (2 * wave + m) * 16 .., X columns t * 16 ..
    float db2 = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int t = 0; t < 8; ++t) acc2[m][t] = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) acc1[m][t] = 0.f;
    }

    for (int ch = blockIdx.x; ch < a.chunks; ch += gridDim.x) {
        const int pair = ch / a.chunks_per_pair, p0 = (ch % a.chunks_per_pair) * G;
        const size_t plane = (size_t)pair * FT_OUT * n0;           // first element of this pair in pooled / arg / gpool

        // ---- 1, 2: a1 and a2 of every row as the forward computed them; dA2 cleared --------------------------
        rebuild_a1(a, pair, p0, cloud0, cloud1, idx, weights, pt, ps, L1, rowp, rows_src, posd, wave, lane);
        for (int e = tid; e < BW_R * FT_C; e += 256) L3[(e >> 7) * BW_S + (e & (FT_C - 1))] = 0.f;
        __syncthreads();
        rebuild_a2(weights, L1, L2, wave, lane);
        __syncthreads();

        // ---- 3: dA2 = dZ3 W3 (sparse: per point and channel one row) ---------------------------------------
        {
            const int n = tid & (FT_C - 1), half = tid >> 7;
            for (int pl = half; pl < G; pl += 2) {                     // the two halves own different rows
                const int p = p0 + pl;
                if (p >= n0) break;
                const size_t base = plane + p;
                for (int c0 = 0; c0 < FT_OUT; c0 += 16) {               // 16 channels' loads in flight at once
                    float pv[16], gv[16], wv[16];
                    int av[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) {
                        const size_t o = base + (size_t)(c0 + u) * n0;
                        pv[u] = pooled[o];
                        gv[u] = gpool[o];
                        av[u] = arg[o];
                        wv[u] = weights[O_W3 + (c0 + u) * FT_C + n];
                    }
#pragma unroll
                    for (int u = 0; u < 16; ++u)
                        if (pv[u] > 0.f) {
                            const int row = pl * k + min(max(av[u], 0), k - 1);
                            L3[row * BW_S + n] = fmaf(gv[u], wv[u], L3[row * BW_S + n]);
                        }
                }
            }
        }
        __syncthreads();

        // ---- 4: dZ2 = dA2 where a2 > 0 ------------------------------------------------------------------------
        for (int e = tid; e < BW_R * FT_C; e += 256) {
            const int r = e >> 7, n = e & (FT_C - 1);
            if (!(L2[r * BW_S + n] > 0.f)) L3[r * BW_S + n] = 0.f;
        }
        __syncthreads();

        // ---- 5: dW2 += dZ2^T a1, db2, dA1 = dZ2 W2 -> dZ1 = dA1 where a1 > 0 (into L2) -------------------------
        for (int g = 0; g < BW_T; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * g + 4 * kq + q;
                float av[2], bw[8];
#pragma unroll
                for (int m = 0; m < 2; ++m) av[m] = L3[r * BW_S + (2 * wave + m) * 16 + c16];
#pragma unroll
                for (int t = 0; t < 8; ++t) bw[t] = L1[r * BW_S + t * 16 + c16];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int t = 0; t < 8; ++t) acc2[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bw[t], acc2[m][t], 0, 0, 0);
            }
        if (tid < FT_C)
            for (int r = 0; r < R; ++r) db2 += L3[r * BW_S + tid];
        {
            dclr_f32x4 acc[BW_T][2];
            mma_rows_wt<BW_T, 2>(acc, L3, BW_S, weights + O_W2T, 32 * wave, 16, lane);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int col = 32 * wave + 16 * u + c16;
#pragma unroll
                for (int t = 0; t < BW_T; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = t * 16 + 4 * kq + i;
                        L2[r * BW_S + col] = L1[r * BW_S + col] > 0.f ? acc[t][u][i] : 0.f;
                    }
            }
        }
        __syncthreads();

        // ---- 6: X = [pos_diff | feat0 | feat1 | 1 | 0...] into L1 ---------------------------------------------
        for (int e = tid; e < BW_R * FT_XP; e += 256) {
            const int r = e / FT_XP, col = e % FT_XP;
            const long long gp = rowp[r];
            float v = 0.f;
            if (gp >= 0) {
                if (col < 3) v = posd[r * 3 + col];
                else if (col < 3 + FT_F) v = cloud0[gp * FT_ROW + col];
                else if (col < FT_IN) v = cloud1[rows_src[r] * FT_ROW + (col - FT_F)];
                else if (col == FT_IN) v = 1.f;
            }
            L1[r * BW_S + col] = v;
        }
        __syncthreads();

        // ---- 7: dW1 | db1 += dZ1^T X; E = dZ1 W1 (into L3) when the clouds need gradients ----------------------
        for (int g = 0; g < BW_T; ++g)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * g + 4 * kq + q;
                float av[2], bw[9];
#pragma unroll
                for (int m = 0; m < 2; ++m) av[m] = L2[r * BW_S + (2 * wave + m) * 16 + c16];
#pragma unroll
                for (int t = 0; t < 9; ++t) bw[t] = L1[r * BW_S + t * 16 + c16];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int t = 0; t < 9; ++t) acc1[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bw[t], acc1[m][t], 0, 0, 0);
            }
        if (a.input_grads) {
            for (int ct = wave; ct < FT_XP / 16; ct += 4) {
                dclr_f32x4 acc[BW_T][1];
                mma_rows_wt<BW_T, 1>(acc, L2, BW_S, weights + O_W1T, 16 * ct, 16, lane);
#pragma unroll
                for (int t = 0; t < BW_T; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) L3[(t * 16 + 4 * kq + i) * BW_S + 16 * ct + c16] = acc[t][0][i];
            }
            __syncthreads();

            // ---- 8: template terms summed over the block's slots (ascending j); source terms per (p, j) ---------
            for (int e = tid; e < G * FT_ROW; e += 256) {
                const int pl = e / FT_ROW, col = e % FT_ROW;
                if (p0 + pl >= n0) continue;
                float s = 0.f;
                for (int j = 0; j < k; ++j) s += L3[(pl * k + j) * BW_S + col];
                grad0[((size_t)pair * n0 + p0 + pl) * FT_ROW + col] = col < 3 ? -s : s;
            }
            for (int e = tid; e < R * E_W; e += 256) {
                const int r = e / E_W, col = e % E_W;
                const long long gp = rowp[r];
                if (gp < 0) continue;
                const float v = col < 3 ? L3[r * BW_S + col] : (col < FT_ROW ? L3[r * BW_S + col + FT_F] : 0.f);
                erows[((size_t)gp * k + r % k) * E_W + col] = v;
            }
        }
        __syncthreads();
    }

    // ---- this workgroup's partial weight gradients, in the layout of grad_weights ---------------------------
    float *out = partial + (size_t)blockIdx.x * O_GRAD;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                out[O_W2 + ((2 * wave + m) * 16 + 4 * kq + i) * FT_C + t * 16 + c16] = acc2[m][t][i];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (2 * wave + m) * 16 + 4 * kq + i, col = t * 16 + c16;
                if (col < FT_IN) out[O_W1 + row * FT_IN + col] = acc1[m][t][i];
                else if (col == FT_IN) out[O_B1 + row] = acc1[m][t][i];
            }
    }
    if (tid < FT_C) out[O_B2 + tid] = db2;
}

// grad[e] = sum over the workgroups (in order) of their partials.
__global__ __launch_bounds__(256) void flow_train_reduce_kernel(int wgs, const float *__restrict__ partial,
                                                                float *__restrict__ grad) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= O_GRAD) return;
    float acc = 0.f;
    for (int w = 0; w < wgs; ++w) acc += partial[(size_t)w * O_GRAD + e];
    grad[e] = acc;
}

// ---- source points: counting sort of idx by source, buckets sorted ascending, summed in that order -------------
__global__ __launch_bounds__(256) void flow_train_count_kernel(long long entries, int n0k, int n1,
                                                               const int32_t *__restrict__ idx, int *__restrict__ cnt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const long long pair = e / n0k;
    atomicAdd(&cnt[pair * n1 + clamp_src(idx[e], n1)], 1);
}

// One workgroup per pair: exclusive scan of the counts (offsets into the pair's n0 * k entries); cursor = offsets.
__global__ __launch_bounds__(256) void flow_train_scan_kernel(int n0k, int n1, const int *__restrict__ cnt,
                                                              int *__restrict__ offs, int *__restrict__ cursor) {
    __shared__ long long part[256];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * n1;
    const int per = (n1 + 255) / 256, s0 = min(n1, t * per), s1 = min(n1, s0 + per);
    long long sum = 0;
    for (int s = s0; s < s1; ++s) sum += cnt[base + s];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long run = (long long)blockIdx.x * n0k;
        for (int i = 0; i < 256; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
    }
    __syncthreads();
    long long run = part[t];
    for (int s = s0; s < s1; ++s) {
        offs[base + s] = (int)run;
        cursor[base + s] = (int)run;
        run += cnt[base + s];
    }
}

__global__ __launch_bounds__(256) void flow_train_fill_kernel(long long entries, int n0k, int n1,
                                                              const int32_t *__restrict__ idx,
                                                              int *__restrict__ cursor, int *__restrict__ list) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= entries) return;
    const long long pair = e / n0k;
    const int pos = atomicAdd(&cursor[pair * n1 + clamp_src(idx[e], n1)], 1);
    list[pos] = (int)e;
}

// Thread per source point: insertion sort of its bucket (the fill's order depends on timing; this one does not).
__global__ __launch_bounds__(256) void flow_train_sort_kernel(long long sources, const int *__restrict__ cnt,
                                                              const int *__restrict__ offs, int *__restrict__ list) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= sources) return;
    int *b = list + offs[s];
    const int n = cnt[s];
    for (int i = 1; i < n; ++i) {
        const int v = b[i];
        int j = i - 1;
        while (j >= 0 && b[j] > v) {
            b[j + 1] = b[j];
            --j;
        }
        b[j + 1] = v;
    }
}

// Thread per (source point, column): the sum of its (p, j) terms in ascending order.
__global__ __launch_bounds__(256) void flow_train_src_kernel(long long sources, const int *__restrict__ cnt,
                                                             const int *__restrict__ offs, const int *__restrict__ list,
                                                             const float *__restrict__ erows,
                                                             float *__restrict__ grad1) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= sources * FT_ROW) return;
    const long long s = e / FT_ROW;
    const int col = (int)(e % FT_ROW);
    const int *b = list + offs[s];
    const int n = cnt[s];
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += erows[(size_t)b[i] * E_W + col];
    grad1[e] = acc;
}

long long round256(long long v) { return (v + 255) / 256 * 256; }

int blocks_per_pair(int n0, int k) { return (n0 + BW_R / k - 1) / (BW_R / k); }

struct Layout {
    long long partial, erows, cnt, offs, cursor, list, total;
    int wgs;
};

Layout layout(int pairs, int n0, int n1, int k) {
    Layout l;
    const long long chunks = (long long)pairs * blocks_per_pair(n0, k);
    l.wgs = (int)(chunks < BW_MAX_WG ? chunks : BW_MAX_WG);
    const long long entries = (long long)pairs * n0 * k, sources = (long long)pairs * n1;
    l.partial = 0;
    l.erows = l.partial + round256((long long)l.wgs * O_GRAD * 4);
    l.cnt = l.erows + round256(entries * E_W * 4);
    l.offs = l.cnt + round256(sources * 4);
    l.cursor = l.offs + round256(sources * 4);
    l.list = l.cursor + round256(sources * 4);
    l.total = l.list + round256(entries * 4);
    return l;
}

int check_sizes(int pairs, int n0, int n1, int k, int f) {
    DCLR_REQUIRE(pairs > 0 && n0 > 0 && n1 > 0);
    if (k < 1 || k > 32 || f != FT_F) return DCLR_E_UNSUPPORTED;
    DCLR_REQUIRE(n1 >= k);
    DCLR_REQUIRE((long long)pairs * n0 * k * E_W < (1ll << 31) && (long long)pairs * n1 * FT_ROW < (1ll << 31) &&
                 (long long)pairs * n0 * FT_OUT < (1ll << 31) && (long long)pairs * (n0 + n1) * FT_C < (1ll << 31));
    return DCLR_OK;
}

}  // namespace

extern "C" int dclr_flow_train_version(void) { return 1000 * 0 + 1; }

extern "C" long long dclr_flow_train_workspace_bytes(int pairs, int n0, int n1, int k) {
    const int rc = check_sizes(pairs, n0, n1, k, FT_F);
    if (rc != DCLR_OK) return rc;
    return layout(pairs, n0, n1, k).total;
}

extern "C" int dclr_flow_train_forward(int pairs, int n0, int n1, int k, int f, float radius, const float *cloud0,
                                       const float *cloud1, const int32_t *idx, const float *weights, float *pt,
                                       float *ps, float *pooled, int32_t *arg, dclr_stream_t stream) {
    const int rc = check_sizes(pairs, n0, n1, k, f);
    if (rc != DCLR_OK) return rc;
    DCLR_REQUIRE(cloud0 && cloud1 && idx && weights && pt && ps && pooled && arg);
    DCLR_REQUIRE(((uintptr_t)weights & 15) == 0 && ((uintptr_t)pt & 7) == 0 && ((uintptr_t)ps & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    const long long rows0 = (long long)pairs * n0, rows1 = (long long)pairs * n1;
    hipLaunchKernelGGL(flow_train_pre_kernel, dim3((unsigned)(((rows0 + rows1) * FT_C + 255) / 256)), dim3(256), 0, st,
                       rows0, rows1, cloud0, cloud1, weights, pt, ps);
    int s = dclr_launch_status();
    if (s != DCLR_OK) return s;
    const unsigned blocks = (unsigned)((rows0 + FW_G - 1) / FW_G);
#define DCLR_FT_CASE(T) case T: hipLaunchKernelGGL((flow_train_fwd_kernel<T>), dim3(blocks), dim3(256), 0, st, pairs, n0, n1, k, radius, cloud0, cloud1, idx, weights, pt, ps, pooled, arg); break
    switch ((k + 3) / 4) {
        DCLR_FT_CASE(1); DCLR_FT_CASE(2); DCLR_FT_CASE(3); DCLR_FT_CASE(4);
        DCLR_FT_CASE(5); DCLR_FT_CASE(6); DCLR_FT_CASE(7); DCLR_FT_CASE(8);
        default: return DCLR_E_UNSUPPORTED;
    }
#undef DCLR_FT_CASE
    return dclr_launch_status();
}

extern "C" int dclr_flow_train_backward(int pairs, int n0, int n1, int k, int f, const float *cloud0,
                                        const float *cloud1, const int32_t *idx, const float *weights, const float *pt,
                                        const float *ps, const float *pooled, const int32_t *arg,
                                        const float *grad_pooled, float *grad_weights, int input_grads,
                                        float *grad_cloud0, float *grad_cloud1, void *workspace,
                                        long long workspace_bytes, dclr_stream_t stream) {
    const int rc = check_sizes(pairs, n0, n1, k, f);
    if (rc != DCLR_OK) return rc;
    DCLR_REQUIRE(cloud0 && cloud1 && idx && weights && pt && ps && pooled && arg && grad_pooled && grad_weights &&
                 workspace);
    DCLR_REQUIRE(!input_grads || (grad_cloud0 && grad_cloud1));
    DCLR_REQUIRE(((uintptr_t)weights & 15) == 0 && ((uintptr_t)pt & 7) == 0 && ((uintptr_t)ps & 7) == 0);
    const Layout l = layout(pairs, n0, n1, k);
    DCLR_REQUIRE(((uintptr_t)workspace & 255) == 0 && workspace_bytes >= l.total);
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    float *partial = reinterpret_cast<float *>(ws + l.partial), *erows = reinterpret_cast<float *>(ws + l.erows);
    int *cnt = reinterpret_cast<int *>(ws + l.cnt), *offs = reinterpret_cast<int *>(ws + l.offs);
    int *cursor = reinterpret_cast<int *>(ws + l.cursor), *list = reinterpret_cast<int *>(ws + l.list);

    BwdArgs prm;
    prm.pairs = pairs;
    prm.n0 = n0;
    prm.n1 = n1;
    prm.k = k;
    prm.g = BW_R / k;
    prm.chunks_per_pair = blocks_per_pair(n0, k);
    prm.chunks = pairs * prm.chunks_per_pair;
    prm.input_grads = input_grads ? 1 : 0;
    hipLaunchKernelGGL(flow_train_bwd_kernel, dim3((unsigned)l.wgs), dim3(256), 0, st, prm, cloud0, cloud1, idx,
                       weights, pt, ps, pooled, arg, grad_pooled, partial, erows, input_grads ? grad_cloud0 : nullptr);
    int s = dclr_launch_status();
    if (s != DCLR_OK) return s;
    hipLaunchKernelGGL(flow_train_bwd3_kernel, dim3((unsigned)l.wgs), dim3(256), 0, st, prm, cloud0, cloud1, idx,
                       weights, pt, ps, pooled, arg, grad_pooled, partial);
    s = dclr_launch_status();
    if (s != DCLR_OK) return s;
    hipLaunchKernelGGL(flow_train_reduce_kernel, dim3((O_GRAD + 255) / 256), dim3(256), 0, st, l.wgs, partial,
                       grad_weights);
    s = dclr_launch_status();
    if (s != DCLR_OK || !input_grads) return s;

    const long long entries = (long long)pairs * n0 * k, sources = (long long)pairs * n1;
    const int n0k = n0 * k;
    if (hipMemsetAsync(cnt, 0, (size_t)sources * 4, st) != hipSuccess) return dclr_launch_status();
    hipLaunchKernelGGL(flow_train_count_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, entries, n0k,
                       n1, idx, cnt);
    hipLaunchKernelGGL(flow_train_scan_kernel, dim3((unsigned)pairs), dim3(256), 0, st, n0k, n1, cnt, offs, cursor);
    hipLaunchKernelGGL(flow_train_fill_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, entries, n0k,
                       n1, idx, cursor, list);
    hipLaunchKernelGGL(flow_train_sort_kernel, dim3((unsigned)((sources + 255) / 256)), dim3(256), 0, st, sources, cnt,
                       offs, list);
    hipLaunchKernelGGL(flow_train_src_kernel, dim3((unsigned)((sources * FT_ROW + 255) / 256)), dim3(256), 0, st,
                       sources, cnt, offs, list, erows, grad_cloud1);
    return dclr_launch_status();
}
