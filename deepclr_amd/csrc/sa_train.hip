// Training form of the fused multi-scale set abstraction (include/deepclr_amd_train.h), f32 on the VALU.
//
// The composed training path groups every neighbourhood into a (B, 4, npoint, nsample) tensor and keeps every activation
// of the 4 -> 16 -> 16 -> 32 shared MLP for autograd (~0.43 GB per KITTI cloud). A max-pool passes gradient to one
// neighbour per (centroid, output channel), so the backward only needs that neighbour's point index:
//
//   forward   one wave per (cloud, centroid, scale): lane = ball-query slot (slot, slot + 64, ...), the MLP with weights as
//             scalar operands, per channel a running maximum and the first slot reaching it; the 32 channels are then
//             folded across the wave by halving exchanges (16 + 8 + 4 + 2 + 1 + 1 shuffles of a 64-bit key). Output: the
//             pooled features and the argmax POINT index (the ball-query indices can be freed once this returns).
//   backward  one workgroup per (cloud, scale, block of 32 centroids), chunks of 4 centroids x 32 channels = 128 items,
//             thread = item: recompute the argmax neighbour's activations, push grad_out through layers 3 -> 1 with
//             the ReLU masks, stage the per-item vectors in LDS; then thread = weight-gradient element sums its outer-
//             product terms over the chunk's items in a fixed order. Partial sums per workgroup go to the workspace; a
//             second kernel adds them in a fixed order. No atomics: the result is bit-identical from run to run.
// The forward's z3 and the backward's recomputation use the same operations in the same order (explicit fmaf, the
// library is built with -ffp-contract=off), so the backward sees exactly the maximum the forward stored.
#include "common.h"
#include "../../include/deepclr_amd_train.h"

namespace {

constexpr int T_IN = 4, T_H1 = 16, T_H2 = 16, T_OUT = 32;
constexpr int T_W1 = 0;
constexpr int T_B1 = T_W1 + T_H1 * T_IN;        // 64
constexpr int T_W2 = T_B1 + T_H1;               // 80
constexpr int T_B2 = T_W2 + T_H2 * T_H1;        // 336
constexpr int T_W3 = T_B2 + T_H2;               // 352
constexpr int T_B3 = T_W3 + T_OUT * T_H2;       // 864
constexpr int T_MLP = T_B3 + T_OUT;             // 896
static_assert(T_MLP == DCLR_TRAIN_MLP_FLOATS, "weight packing");

constexpr int T_MAX_SCALES = 2;
constexpr int FWD_WAVES = 4;

constexpr int BW_THREADS = 128;                 // items per chunk: 4 centroids x 32 channels
constexpr int BW_CHUNK_CENT = BW_THREADS / T_OUT;
constexpr int BW_BLOCK_CENT = 32;               // centroids per workgroup (one partial sum each)
// LDS row per item: x (4), 1, a1 (16), a2 (16), dz1 (16), dz2 (16), dz3 of the item's channel
constexpr int R_X = 0, R_ONE = 4, R_A1 = 5, R_A2 = R_A1 + T_H1, R_DZ1 = R_A2 + T_H2, R_DZ2 = R_DZ1 + T_H1,
              R_G = R_DZ2 + T_H2, ROW = R_G + 2;                               // 71: odd stride
constexpr int BW_OUT_PER_THREAD = (T_MLP + BW_THREADS - 1) / BW_THREADS;     // 7

struct TrainArgs {
    int n, f, npoint, scales;
    int nsample[T_MAX_SCALES];
    const int32_t *idx[T_MAX_SCALES];
};

__device__ __forceinline__ int clamp_point(int k, int n) { return (unsigned)k < (unsigned)n ? k : (k < 0 ? 0 : n - 1); }
__device__ __forceinline__ float relu(float z) { return z > 0.f ? z : 0.f; }      // +0 for z <= 0 (and for -0)

// Layers 1 and 2 of one neighbour: x -> z1, a1 -> z2, a2 (W as scalar operands: wave-uniform `w`).
__device__ __forceinline__ void mlp12(dclr_const_f32p w, const float x[T_IN], float z1[T_H1], float a1[T_H1],
                                      float z2[T_H2], float a2[T_H2]) {
#pragma unroll
    for (int i = 0; i < T_H1; ++i) {
        float z = w[T_B1 + i];
#pragma unroll
        for (int k = 0; k < T_IN; ++k) z = fmaf(w[T_W1 + i * T_IN + k], x[k], z);
        z1[i] = z;
        a1[i] = relu(z);
    }
#pragma unroll
    for (int j = 0; j < T_H2; ++j) {
        float z = w[T_B2 + j];
#pragma unroll
        for (int i = 0; i < T_H1; ++i) z = fmaf(w[T_W2 + j * T_H1 + i], a1[i], z);
        z2[j] = z;
        a2[j] = relu(z);
    }
}

__device__ __forceinline__ void load_input(const float *cloud, const float *fcl, int k, float cx, float cy, float cz,
                                           float x[T_IN]) {
    x[0] = cloud[(size_t)k * 3 + 0] - cx;
    x[1] = cloud[(size_t)k * 3 + 1] - cy;
    x[2] = cloud[(size_t)k * 3 + 2] - cz;
    x[3] = fcl ? fcl[k] : 0.f;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
    const int lo = __shfl_xor((int)(uint32_t)v, mask), hi = __shfl_xor((int)(uint32_t)(v >> 32), mask);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

// One halving step over the wave: lanes with bit log2(2 * HALF) clear keep channels [0, HALF) of `key`, the others
// [HALF, 2 * HALF); each takes the maximum with its partner's copy of the same channels.
template <int HALF>
__device__ __forceinline__ void fold(uint64_t *key, int lane) {
    const bool hi = (lane & (2 * HALF)) != 0;
#pragma unroll
    for (int j = 0; j < HALF; ++j) {
        const uint64_t keep = hi ? key[HALF + j] : key[j];
        const uint64_t send = hi ? key[j] : key[HALF + j];
        key[j] = umax64(keep, shfl_xor_u64(send, 2 * HALF));
    }
}

__global__ __launch_bounds__(FWD_WAVES * 64) void sa_train_fwd_kernel(TrainArgs a, int b, const float *__restrict__ xyz,
                                                                      const float *__restrict__ feats,
                                                                      const float *__restrict__ new_xyz,
                                                                      const float *__restrict__ weights,
                                                                      float *__restrict__ features,
                                                                      int32_t *__restrict__ arg) {
    const long long wave = (long long)blockIdx.x * FWD_WAVES + dclr_uniform((int)(threadIdx.x >> 6));
    if (wave >= (long long)b * a.npoint * a.scales) return;
    const int lane = dclr_lane();
    const int s = (int)(wave % a.scales);
    const long long cp = wave / a.scales;                       // cloud * npoint + centroid
    const int bb = (int)(cp / a.npoint), p = (int)(cp % a.npoint);
    const int ns = s ? a.nsample[1] : a.nsample[0];
    const int32_t *idx = (s ? a.idx[1] : a.idx[0]) + (size_t)cp * ns;
    const dclr_const_f32p w = dclr_as_const(weights + (size_t)s * T_MLP);
    const float cx = new_xyz[(size_t)cp * 3 + 0], cy = new_xyz[(size_t)cp * 3 + 1], cz = new_xyz[(size_t)cp * 3 + 2];
    const float *cloud = xyz + (size_t)bb * a.n * 3;
    const float *fcl = a.f ? feats + (size_t)bb * a.n : nullptr;

    float best[T_OUT];
    int bslot[T_OUT];
#pragma unroll
    for (int c = 0; c < T_OUT; ++c) {
        best[c] = -1.f;
        bslot[c] = 0;
    }
    for (int slot = lane; slot < ns; slot += 64) {
        float x[T_IN], z1[T_H1], a1[T_H1], z2[T_H2], a2[T_H2];
        load_input(cloud, fcl, clamp_point(idx[slot], a.n), cx, cy, cz, x);
        mlp12(w, x, z1, a1, z2, a2);
#pragma unroll
        for (int c = 0; c < T_OUT; ++c) {
            float z = w[T_B3 + c];
#pragma unroll
            for (int j = 0; j < T_H2; ++j) z = fmaf(w[T_W3 + c * T_H2 + j], a2[j], z);
            const float v = relu(z);
            if (v > best[c]) {                                  // slots ascend per lane: keeps the first maximum
                best[c] = v;
                bslot[c] = slot;
            }
        }
    }
    // key = (value bits, ~slot): values are >= +0, so the u32 order of the bits is the value order; a larger key is a
    // larger value or, on a tie, an earlier slot. Lanes without a slot hold 0, below every real key.
    uint64_t key[T_OUT];
#pragma unroll
    for (int c = 0; c < T_OUT; ++c)
        key[c] = best[c] < 0.f ? 0ull : ((uint64_t)__float_as_uint(best[c]) << 32) | (0xFFFFFFFFu - (uint32_t)bslot[c]);
    fold<16>(key, lane);
    fold<8>(key, lane);
    fold<4>(key, lane);
    fold<2>(key, lane);
    fold<1>(key, lane);
    const uint64_t k = umax64(key[0], shfl_xor_u64(key[0], 1));  // lanes 2c, 2c + 1: channel c
    if ((lane & 1) == 0) {
        const int c = lane >> 1;
        const uint32_t sl = 0xFFFFFFFFu - (uint32_t)k;
        const int slot = sl < (uint32_t)ns ? (int)sl : 0;
        const size_t o = ((size_t)bb * (T_OUT * a.scales) + (size_t)s * T_OUT + c) * a.npoint + p;
        features[o] = __uint_as_float((uint32_t)(k >> 32));
        arg[o] = clamp_point(idx[slot], a.n);
    }
}

__global__ __launch_bounds__(BW_THREADS) void sa_train_bwd_kernel(TrainArgs a, int nblk, const float *__restrict__ xyz,
                                                                  const float *__restrict__ feats,
                                                                  const float *__restrict__ new_xyz,
                                                                  const float *__restrict__ weights,
                                                                  const float *__restrict__ grad_out,
                                                                  const int32_t *__restrict__ arg,
                                                                  float *__restrict__ partial) {
    __shared__ float rows[BW_THREADS * ROW];
    __shared__ float w3s[T_OUT * (T_H2 + 1)];                   // W3 rows by lane-varying channel: padded against conflicts
    const int t = threadIdx.x;
    const int wg = blockIdx.x;                                  // (cloud * scales + scale) * nblk + block
    const int blk = wg % nblk, s = (wg / nblk) % a.scales, bb = wg / (nblk * a.scales);
    const float *wg_w = weights + (size_t)s * T_MLP;
    const dclr_const_f32p w = dclr_as_const(wg_w);
    for (int e = t; e < T_OUT * T_H2; e += BW_THREADS) w3s[(e / T_H2) * (T_H2 + 1) + e % T_H2] = wg_w[T_W3 + e];
    const float *cloud = xyz + (size_t)bb * a.n * 3;
    const float *fcl = a.f ? feats + (size_t)bb * a.n : nullptr;

    // the weight-gradient elements this thread sums: o = t + BW_THREADS * r; term = row[ia] * row[ib] over the items
    // it0, it0 + step, ... (dW3 / db3: the items of their own channel only)
    int ia[BW_OUT_PER_THREAD], ib[BW_OUT_PER_THREAD], it0[BW_OUT_PER_THREAD], step[BW_OUT_PER_THREAD];
    float acc[BW_OUT_PER_THREAD];
#pragma unroll
    for (int r = 0; r < BW_OUT_PER_THREAD; ++r) {
        const int o = t + BW_THREADS * r;
        acc[r] = 0.f;
        it0[r] = 0;
        step[r] = 1;
        if (o < T_B1) {
            ia[r] = R_DZ1 + o / T_IN;
            ib[r] = R_X + o % T_IN;
        } else if (o < T_W2) {
            ia[r] = R_DZ1 + (o - T_B1);
            ib[r] = R_ONE;
        } else if (o < T_B2) {
            ia[r] = R_DZ2 + (o - T_W2) / T_H1;
            ib[r] = R_A1 + (o - T_W2) % T_H1;
        } else if (o < T_W3) {
            ia[r] = R_DZ2 + (o - T_B2);
            ib[r] = R_ONE;
        } else if (o < T_B3) {
            ia[r] = R_G;
            ib[r] = R_A2 + (o - T_W3) % T_H2;
            it0[r] = (o - T_W3) / T_H2;
            step[r] = T_OUT;
        } else if (o < T_MLP) {
            ia[r] = R_G;
            ib[r] = R_ONE;
            it0[r] = o - T_B3;
            step[r] = T_OUT;
        } else {
            ia[r] = ib[r] = 0;
            it0[r] = BW_THREADS;                                // nothing to sum
        }
    }
    __syncthreads();

    const int c = t % T_OUT;
    float *row = rows + t * ROW;
    for (int chunk = 0; chunk < BW_BLOCK_CENT / BW_CHUNK_CENT; ++chunk) {
        const int p = blk * BW_BLOCK_CENT + chunk * BW_CHUNK_CENT + t / T_OUT;
        float x[T_IN] = {0.f, 0.f, 0.f, 0.f}, z1[T_H1], a1[T_H1], z2[T_H2], a2[T_H2], dz1[T_H1], dz2[T_H2];
        float gz3 = 0.f;
#pragma unroll
        for (int i = 0; i < T_H1; ++i) z1[i] = a1[i] = dz1[i] = 0.f;
#pragma unroll
        for (int j = 0; j < T_H2; ++j) z2[j] = a2[j] = dz2[j] = 0.f;
        if (p < a.npoint) {
            const size_t cp = (size_t)bb * a.npoint + p;
            const size_t o = ((size_t)bb * (T_OUT * a.scales) + (size_t)s * T_OUT + c) * a.npoint + p;
            load_input(cloud, fcl, clamp_point(arg[o], a.n), new_xyz[cp * 3 + 0], new_xyz[cp * 3 + 1],
                       new_xyz[cp * 3 + 2], x);
            mlp12(w, x, z1, a1, z2, a2);
            float z = w[T_B3 + c];
#pragma unroll
            for (int j = 0; j < T_H2; ++j) z = fmaf(w3s[c * (T_H2 + 1) + j], a2[j], z);
            if (z > 0.f) {                                      // ReLU of the pooled output: else no gradient
                gz3 = grad_out[o];
#pragma unroll
                for (int j = 0; j < T_H2; ++j) dz2[j] = z2[j] > 0.f ? gz3 * w3s[c * (T_H2 + 1) + j] : 0.f;
#pragma unroll
                for (int i = 0; i < T_H1; ++i) {
                    float d = 0.f;
#pragma unroll
                    for (int j = 0; j < T_H2; ++j) d = fmaf(w[T_W2 + j * T_H1 + i], dz2[j], d);
                    dz1[i] = z1[i] > 0.f ? d : 0.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < T_IN; ++k) x[k] = 0.f;       // an item without gradient adds exact zeros
#pragma unroll
                for (int i = 0; i < T_H1; ++i) a1[i] = 0.f;
#pragma unroll
                for (int j = 0; j < T_H2; ++j) a2[j] = 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < T_IN; ++k) row[R_X + k] = x[k];
        row[R_ONE] = 1.f;
#pragma unroll
        for (int i = 0; i < T_H1; ++i) {
            row[R_A1 + i] = a1[i];
            row[R_DZ1 + i] = dz1[i];
        }
#pragma unroll
        for (int j = 0; j < T_H2; ++j) {
            row[R_A2 + j] = a2[j];
            row[R_DZ2 + j] = dz2[j];
        }
        row[R_G] = gz3;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < BW_OUT_PER_THREAD; ++r)
            for (int it = it0[r]; it < BW_THREADS; it += step[r])
                acc[r] = fmaf(rows[it * ROW + ia[r]], rows[it * ROW + ib[r]], acc[r]);
        __syncthreads();
    }
    float *out = partial + (size_t)wg * T_MLP;
#pragma unroll
    for (int r = 0; r < BW_OUT_PER_THREAD; ++r) {
        const int o = t + BW_THREADS * r;
        if (o < T_MLP) out[o] = acc[r];
    }
}

// grad[s * 896 + e] = sum over clouds and centroid blocks (in that order) of the partial sums of scale s.
__global__ __launch_bounds__(256) void sa_train_reduce_kernel(int b, int scales, int nblk, const float *__restrict__ partial,
                                                              float *__restrict__ grad) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= scales * T_MLP) return;
    const int s = o / T_MLP, e = o % T_MLP;
    float acc = 0.f;
    for (int bb = 0; bb < b; ++bb) {
        const float *src = partial + ((size_t)(bb * scales + s) * nblk) * T_MLP + e;
        for (int k = 0; k < nblk; ++k) acc += src[(size_t)k * T_MLP];
    }
    grad[o] = acc;
}

int check_common(int b, int n, int f, int npoint, int scales, const float *xyz, const float *feats, const float *new_xyz,
                 const float *weights) {
    DCLR_REQUIRE(b > 0 && n > 0 && npoint > 0 && scales > 0 && f >= 0);
    DCLR_REQUIRE(xyz && new_xyz && weights);
    if (scales > T_MAX_SCALES || f > 1) return DCLR_E_UNSUPPORTED;
    DCLR_REQUIRE(f == 0 || feats);
    DCLR_REQUIRE((long long)b * n * 3 < (1ll << 40) && (long long)b * npoint * scales * 64 < (1ll << 40));
    return DCLR_OK;
}

long long workspace_bytes(int b, int npoint, int scales) {
    const long long nblk = (npoint + BW_BLOCK_CENT - 1) / BW_BLOCK_CENT;
    const long long bytes = (long long)b * scales * nblk * T_MLP * (long long)sizeof(float);
    return (bytes + 255) / 256 * 256;
}

}  // namespace

extern "C" int dclr_train_version(void) { return 1000 * 0 + 1; }

extern "C" long long dclr_sa_msg_train_workspace_bytes(int b, int npoint, int scales) {
    if (b <= 0 || npoint <= 0 || scales <= 0) return DCLR_E_INVALID;
    if (scales > T_MAX_SCALES) return DCLR_E_UNSUPPORTED;
    return workspace_bytes(b, npoint, scales);
}

extern "C" int dclr_sa_msg_train_forward(int b, int n, int f, int npoint, int scales, const int *nsample_host,
                                         const float *xyz, const float *feats, const float *new_xyz,
                                         const int32_t *const *idx_host, const float *weights, float *features,
                                         int32_t *arg, dclr_stream_t stream) {
    const int rc = check_common(b, n, f, npoint, scales, xyz, feats, new_xyz, weights);
    if (rc != DCLR_OK) return rc;
    DCLR_REQUIRE(nsample_host && idx_host && features && arg);
    TrainArgs prm = {};
    prm.n = n;
    prm.f = f;
    prm.npoint = npoint;
    prm.scales = scales;
    for (int s = 0; s < scales; ++s) {
        DCLR_REQUIRE(nsample_host[s] > 0 && idx_host[s]);
        prm.nsample[s] = nsample_host[s];
        prm.idx[s] = idx_host[s];
    }
    const long long waves = (long long)b * npoint * scales;
    const long long blocks = (waves + FWD_WAVES - 1) / FWD_WAVES;
    DCLR_REQUIRE(blocks < (1ll << 31));
    hipLaunchKernelGGL(sa_train_fwd_kernel, dim3((unsigned)blocks), dim3(FWD_WAVES * 64), 0, (hipStream_t)stream, prm, b,
                       xyz, f ? feats : nullptr, new_xyz, weights, features, arg);
    return dclr_launch_status();
}

extern "C" int dclr_sa_msg_train_backward(int b, int n, int f, int npoint, int scales, const float *xyz, const float *feats,
                                          const float *new_xyz, const float *weights, const float *grad_out,
                                          const int32_t *arg, float *grad_weights, void *workspace,
                                          long long workspace_bytes_, dclr_stream_t stream) {
    const int rc = check_common(b, n, f, npoint, scales, xyz, feats, new_xyz, weights);
    if (rc != DCLR_OK) return rc;
    DCLR_REQUIRE(grad_out && arg && grad_weights && workspace);
    DCLR_REQUIRE(((uintptr_t)workspace & 15) == 0 && workspace_bytes_ >= workspace_bytes(b, npoint, scales));
    const int nblk = (npoint + BW_BLOCK_CENT - 1) / BW_BLOCK_CENT;
    const long long wgs = (long long)b * scales * nblk;
    DCLR_REQUIRE(wgs < (1ll << 31) && (long long)b * scales * T_MLP < (1ll << 31));
    TrainArgs prm = {};
    prm.n = n;
    prm.f = f;
    prm.npoint = npoint;
    prm.scales = scales;
    float *partial = static_cast<float *>(workspace);
    hipLaunchKernelGGL(sa_train_bwd_kernel, dim3((unsigned)wgs), dim3(BW_THREADS), 0, (hipStream_t)stream, prm, nblk, xyz,
                       f ? feats : nullptr, new_xyz, weights, grad_out, arg, partial);
    int st = dclr_launch_status();
    if (st != DCLR_OK) return st;
    hipLaunchKernelGGL(sa_train_reduce_kernel, dim3((scales * T_MLP + 255) / 256), dim3(256), 0, (hipStream_t)stream, b,
                       scales, nblk, partial, grad_weights);
    return dclr_launch_status();
}
