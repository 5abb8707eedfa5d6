/*
 * deepclr_amd_train.h -- C ABI of libdeepclr_amd_train.so (gfx950 / MI355X): the training form of the fused
 * multi-scale set abstraction (xyz + <= 1 feature in, shared MLP 4 -> 16 -> 16 -> 32 per scale, max over the
 * neighbourhood), forward with an argmax and the backward of the shared MLP's weights.
 *
 * A library of its own so that the inference ABI (deepclr_amd.h, version 0.2) stays as it is. It keeps that ABI's
 * conventions: device pointers unless a name ends in _host, the caller allocates every output and workspace, nothing
 * synchronises, work is enqueued on `stream`; 0 = enqueued, DCLR_E_* < 0 = rejected before any launch,
 * -(1000 + hipError_t) = the HIP runtime refused the launch. Every size and pointer is checked before the first launch.
 *
 * Weights: per scale s, DCLR_TRAIN_MLP_FLOATS f32 at weights + s * DCLR_TRAIN_MLP_FLOATS, packed as
 *   W1 (16 x 4) b1 (16) W2 (16 x 16) b2 (16) W3 (32 x 16) b3 (32), row-major (out, in);
 * column 3 of W1 is the feature's weight (f = 1); with f = 0 it is read as if the feature were 0.
 * The network input of scale s for neighbour k of centroid p is (xyz[k] - new_xyz[p], feats[k]), each layer
 * z = W a + b followed by ReLU, the output the maximum over the ball-query slots of the centroid.
 */
#ifndef DEEPCLR_AMD_TRAIN_H
#define DEEPCLR_AMD_TRAIN_H

#include "deepclr_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DCLR_TRAIN_MLP_FLOATS 896

int dclr_train_version(void);                   /* 1000*major + minor */

/* xyz (b,n,3), feats (b,f,n) or NULL when f = 0, new_xyz (b,npoint,3) f32; idx_host[s] (b,npoint,nsample_host[s]) i32
 * from the ball query of deepclr_amd.h (indices outside [0, n) are clamped); weights (scales * 896) f32.
 * features (b, 32*scales, npoint) f32: channel 32*s + c of centroid p is max over the slots of ReLU(z3_c);
 * arg (b, 32*scales, npoint) i32: the POINT index of the first slot that reaches that maximum.
 * scales in {1, 2}, f in {0, 1}. */
int dclr_sa_msg_train_forward(int b, int n, int f, int npoint, int scales, const int *nsample_host,
                              const float *xyz, const float *feats, const float *new_xyz,
                              const int32_t *const *idx_host, const float *weights,
                              float *features, int32_t *arg, dclr_stream_t stream);

/* Bytes of the workspace dclr_sa_msg_train_backward needs (a multiple of 256); DCLR_E_* for invalid sizes. */
long long dclr_sa_msg_train_workspace_bytes(int b, int npoint, int scales);

/* grad_out (b, 32*scales, npoint) f32 and arg from dclr_sa_msg_train_forward on the same xyz / feats / new_xyz /
 * weights -> grad_weights (scales * 896) f32 in the layout of `weights`, overwritten. Per (cloud, centroid, scale,
 * channel) the argmax neighbour's activations are recomputed and grad_out is propagated through layers 3 -> 1 (ReLU
 * masks as torch: a unit contributes only where its output is > 0). The terms are summed per workgroup into the workspace
 * (16-byte aligned, >= dclr_sa_msg_train_workspace_bytes) and the partial sums reduced in a fixed order: no atomics,
 * the same inputs give bit-identical gradients on every run. */
int dclr_sa_msg_train_backward(int b, int n, int f, int npoint, int scales,
                               const float *xyz, const float *feats, const float *new_xyz, const float *weights,
                               const float *grad_out, const int32_t *arg, float *grad_weights,
                               void *workspace, long long workspace_bytes, dclr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DEEPCLR_AMD_TRAIN_H */
