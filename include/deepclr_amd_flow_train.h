/*
 * deepclr_amd_flow_train.h -- C ABI of libdeepclr_amd_flow_train.so (gfx950 / MI355X): the training form of the fused
 * flow embedding (kNN neighbourhoods of a template cloud in a source cloud, shared MLP 131 -> 128 -> 128 -> 256 on
 * [xyz1[idx] - xyz0[p] | feat0[p] | feat1[idx]], radius mask, max over the neighbours): a forward with a per-channel
 * argmax and the backward of the weights and of both input clouds.
 *
 * A library of its own, next to the inference ABI (deepclr_amd.h, version 0.2) and the set-abstraction training library
 * (deepclr_amd_train.h), both unchanged. Conventions as there: device pointers unless a name ends in _host, the caller
 * allocates every output and workspace, nothing synchronises, work is enqueued on `stream`; 0 = enqueued, DCLR_E_* < 0
 * = rejected before any launch, -(1000 + hipError_t) = the HIP runtime refused a launch. Every size and pointer is
 * checked before the first launch.
 *
 * Clouds are POINT-major: cloud0 (pairs, n0, 67) templates, cloud1 (pairs, n1, 67) sources, each row [x y z | 64
 * features]. idx (pairs, n0, k) i32: the source point (0 <= idx < n1) of neighbour slot j of template point p.
 *
 * Weights: DCLR_FLOW_TRAIN_MLP_FLOATS f32, row-major (out, in), at these float offsets:
 *   W1 (128 x 131)   0       columns [0, 3) pos_diff (W1a), [3, 67) template features (W1t), [67, 131) source (W1s)
 *   b1 (128)         16768
 *   W2 (128 x 128)   16896
 *   b2 (128)         33280
 *   W3 (256 x 128)   33408
 *   b3 (256)         66176
 *   W2^T (128 x 128) 66432   W2 transposed
 *   W1^T (144 x 128) 82816   W1 transposed, rows 131..143 zero
 * The first DCLR_FLOW_TRAIN_GRAD_FLOATS (66432) floats are the parameters; grad_weights has exactly that layout.
 *
 * Layer 1 is split by linearity: pt = W1t feat0 and ps = W1s feat1 (pairs, n, 128), each an fmaf chain over the 64
 * features in ascending order, come out of the forward and go back into the backward, so that the backward rebuilds
 * the forward's activations bit for bit. Layers 2 and 3 run on v_mfma_f32_16x16x4_f32. Radius: a neighbour with
 * sqrtf(dx*dx + dy*dy + dz*dz) >= radius contributes 0 to the maximum; radius <= 0 disables the mask.
 *
 * LDS per workgroup (gfx950 allows 160 KiB): forward at most 67600 bytes (k = 32: 8 * 16 * 132 * 4 + 16), backward at
 * most 144320 bytes (three 80 x 148 f32 tiles + 2240 bytes of row bookkeeping), the other kernels at most 2048 bytes.
 */
#ifndef DEEPCLR_AMD_FLOW_TRAIN_H
#define DEEPCLR_AMD_FLOW_TRAIN_H

#include "deepclr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCLR_FLOW_TRAIN_GRAD_FLOATS 66432
#define DCLR_FLOW_TRAIN_MLP_FLOATS 101248

int dclr_flow_train_version(void);              /* 1000*major + minor */

/* cloud0, cloud1, idx as above, 1 <= k <= n1, k <= 32, f = 64 features per row (others: DCLR_E_UNSUPPORTED),
 * weights packed as above ->
 * pt (pairs, n0, 128), ps (pairs, n1, 128) f32: the layer-1 feature products (kept for the backward);
 * pooled (pairs, 256, n0) f32: channel c of template p is max over the unmasked slots of ReLU(z3_c), 0 if none;
 * arg (pairs, 256, n0) i32: the first slot j (not the point) that reaches that maximum; 0 where the maximum is 0.
 * Slot indices outside [0, n1) are clamped for reading and count as masked. */
int dclr_flow_train_forward(int pairs, int n0, int n1, int k, int f, float radius, const float *cloud0,
                            const float *cloud1, const int32_t *idx, const float *weights, float *pt, float *ps, float *pooled,
                            int32_t *arg, dclr_stream_t stream);

/* Bytes of the workspace dclr_flow_train_backward needs: a multiple of 256, monotone in every argument;
 * DCLR_E_* for invalid sizes. With C = pairs * ceil(n0 / floor(80 / k)) blocks of template points and
 * W = min(C, 160) workgroups it is the sum, each rounded up to 256 bytes, of
 *   W * 66432 * 4                (per-workgroup partial weight gradients)
 *   pairs * n0 * k * 68 * 4      (per (p, j): W1a^T dZ1 and W1s^T dZ1, the source-gradient terms)
 *   3 * pairs * n1 * 4           (per source point: count, offset, cursor)
 *   pairs * n0 * k * 4           (the (p, j) of every source point, sorted ascending) */
long long dclr_flow_train_workspace_bytes(int pairs, int n0, int n1, int k);

/* grad_pooled (pairs, 256, n0) f32 and pt / ps / pooled / arg from dclr_flow_train_forward on the same inputs ->
 * grad_weights (66432) f32, overwritten; with input_grads != 0 also grad_cloud0 (pairs, n0, 67) and grad_cloud1
 * (pairs, n1, 67), overwritten (NULL otherwise). grad_cloud0's xyz columns hold only the pos_diff term,
 * -W1a^T sum_j dZ1[p, j]: the caller adds the gradient of the xyz rows it copies into its output.
 * dZ3 is grad_pooled at (arg, c) where pooled > 0 and 0 elsewhere; ReLU masks as torch (a unit passes gradient only
 * where its output is > 0). Per-workgroup partial sums are reduced in a fixed order and every source point sums its
 * (p, j) terms in ascending order: no float atomics, the same inputs give bit-identical gradients on every run.
 * workspace: 256-byte aligned, >= dclr_flow_train_workspace_bytes(pairs, n0, n1, k). */
int dclr_flow_train_backward(int pairs, int n0, int n1, int k, int f, const float *cloud0, const float *cloud1,
                             const int32_t *idx, const float *weights, const float *pt, const float *ps,
                             const float *pooled, const int32_t *arg, const float *grad_pooled, float *grad_weights,
                             int input_grads, float *grad_cloud0, float *grad_cloud1, void *workspace,
                             long long workspace_bytes, dclr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEEPCLR_AMD_FLOW_TRAIN_H */
