"""Operator-level API: the functions the reference imports from its native extensions.

Level 1 mirrors, name for name and argument for argument, what
``deepclr/models/deepclr.py`` obtains from the absent third-party packages:
``pointnet2`` (``furthest_point_sample``, ``gather_operation``, ``ball_query``,
``grouping_operation``; exported by /root/reference/extern/pointnet2.patch:37-40) and
``torch_cluster.knn`` (call site deepclr.py:164-166). Level 2 exposes the fused
kernels the model forward uses. Everything runs on the current torch stream.
"""
import ctypes
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import lib

F_STRIDE = 68
E_STRIDE = 264
FUSED_MAX_POINTS = 65536        # points per cloud the fused sampler / set-abstraction kernels take (16-bit point indices)

# Optional launch timer (bench.py): an object with begin(name) -> token and end(token), called on the
# stream the kernel is enqueued on. None in normal operation.
TIMER = None

# Matrix path of the fused flow-embedding and pose-head kernels: 'f16x2' = f32 operands split into f16 hi/lo
# halves on the f16 matrix instructions (f32-accurate, csrc/mma16f.h), 'f32' = the f32 matrix instructions.
PRECISION = os.environ.get('DCLR_PRECISION', 'f16x2')

# Split-f16 operands saturate at +-65504 (csrc/mma16f.h clamps instead of producing inf). Weights are checked when they
# are packed; activations cannot be checked inside the fused kernels for free. CHECK_RANGE (DCLR_CHECK_RANGE):
#   'first' (default)  the FIRST forward after the weights changed (load_state_dict, .to(), an optimizer step) also runs
#                      the dense stages on the f32 matrix instructions, on that call's own activations, and raises if the
#                      two disagree or an activation leaves the range: a new checkpoint cannot clamp silently on first use;
#   'always' (or '1')  every forward does (debugging; halves throughput);
#   'never' (or '0')   no check.
CHECK_RANGE = {'1': 'always', '0': 'never'}.get(os.environ.get('DCLR_CHECK_RANGE', 'first'),
                                                os.environ.get('DCLR_CHECK_RANGE', 'first'))
if CHECK_RANGE not in ('first', 'always', 'never'):
    raise RuntimeError("DCLR_CHECK_RANGE must be one of first, always, never, 1, 0 (got '{}')".format(CHECK_RANGE))
if PRECISION not in ('f16x2', 'f32'):
    raise RuntimeError("DCLR_PRECISION must be f16x2 or f32 (got '{}')".format(PRECISION))
F16_MAX = 65504.0


def check_f16_range(t: torch.Tensor, what: str) -> None:
    """Raise if a tensor about to be packed as split-f16 operands leaves the f16 range (one host sync, pack time only)."""
    peak = float(t.detach().abs().max()) if t.numel() else 0.0
    if not peak < F16_MAX:
        raise RuntimeError("{}: |value| reaches {:.4g}, outside the split-f16 operand range (+-65504); run with "
                           "DCLR_PRECISION=f32 (f32 matrix instructions) for this checkpoint".format(what, peak))



def _call(name: str, what: str, *args) -> None:
    fn = getattr(lib.load(), name)
    if TIMER is None:
        lib.check(fn(*args), what)
        return
    token = TIMER.begin(what)
    code = fn(*args)
    TIMER.end(token)
    lib.check(code, what)


# ------------------------------------------------------------------------------------------------
# level 1
# ------------------------------------------------------------------------------------------------
def furthest_point_sample(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    """xyz (B, N, 3) -> (B, npoint) int32 indices."""
    xyz = lib.dev_f32(xyz, 'xyz')
    b, n, c = xyz.shape
    assert c == 3
    idx = torch.empty(b, npoint, dtype=torch.int32, device=xyz.device)
    temp = torch.full((b, n), 1e10, dtype=torch.float32, device=xyz.device)
    _call('dclr_furthest_point_sampling', 'furthest_point_sample', b, n, npoint, xyz.data_ptr(), temp.data_ptr(),
                                                      idx.data_ptr(), lib.stream_ptr())
    return idx


def gather_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """features (B, C, N), idx (B, npoint) int32 -> (B, C, npoint)."""
    features = lib.dev_f32(features, 'features')
    b, c, n = features.shape
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()
    npoint = idx.shape[1]
    out = torch.empty(b, c, npoint, dtype=torch.float32, device=features.device)
    _call('dclr_gather_points', 'gather_operation', b, c, n, npoint, features.data_ptr(), idx.data_ptr(), out.data_ptr(),
                                            lib.stream_ptr())
    return out


def ball_query(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
    """xyz (B, N, 3), new_xyz (B, npoint, 3) -> (B, npoint, nsample) int32."""
    xyz, new_xyz = lib.dev_f32(xyz, 'xyz'), lib.dev_f32(new_xyz, 'new_xyz')
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.zeros(b, m, nsample, dtype=torch.int32, device=xyz.device)
    _call('dclr_ball_query', 'ball_query', b, n, m, float(radius), nsample, new_xyz.data_ptr(), xyz.data_ptr(),
                                         idx.data_ptr(), lib.stream_ptr())
    return idx


def grouping_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """features (B, C, N), idx (B, npoint, nsample) int32 -> (B, C, npoint, nsample)."""
    features = lib.dev_f32(features, 'features')
    b, c, n = features.shape
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous()
    _, npoint, nsample = idx.shape
    out = torch.empty(b, c, npoint, nsample, dtype=torch.float32, device=features.device)
    _call('dclr_group_points', 'grouping_operation', b, c, n, npoint, nsample, features.data_ptr(), idx.data_ptr(),
                                           out.data_ptr(), lib.stream_ptr())
    return out


def gather_operation_grad(grad_out: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """Backward of gather_operation: grad_out (B, C, npoint), idx (B, npoint) int32 -> grad_features (B, C, n)."""
    grad_out = lib.dev_f32(grad_out, 'grad_out')
    b, c, npoint = grad_out.shape
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape == (b, npoint)
    grad = torch.zeros(b, c, n, dtype=torch.float32, device=grad_out.device)
    _call('dclr_gather_points_grad', 'gather_operation_grad', b, c, n, npoint, grad_out.data_ptr(), idx.data_ptr(),
          grad.data_ptr(), lib.stream_ptr())
    return grad


def grouping_operation_grad(grad_out: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """Backward of grouping_operation: grad_out (B, C, npoint, nsample), idx (B, npoint, nsample) int32 ->
    grad_features (B, C, n)."""
    grad_out = lib.dev_f32(grad_out, 'grad_out')
    b, c, npoint, nsample = grad_out.shape
    assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.shape == (b, npoint, nsample)
    grad = torch.zeros(b, c, n, dtype=torch.float32, device=grad_out.device)
    _call('dclr_group_points_grad', 'grouping_operation_grad', b, c, n, npoint, nsample, grad_out.data_ptr(), idx.data_ptr(),
          grad.data_ptr(), lib.stream_ptr())
    return grad


def knn(x: torch.Tensor, y: torch.Tensor, k: int, batch_x: Optional[torch.Tensor] = None,
        batch_y: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> torch.Tensor:
    """``torch_cluster.knn`` for equally sized sorted batches: (2, len(y)*k) int64 = [y index; x index] (fewer columns when
    a query has fewer than k candidates within a squared distance of 1e10: upstream's slots start there and stay -1).
    The batch count has to be known on the host (it sizes the launch): one device-to-host read of the two batch
    vectors' last entries, none when the caller passes ``batch_size`` (torch_cluster >= 1.6 takes the same argument)."""
    x, y = lib.dev_f32(x, 'x'), lib.dev_f32(y, 'y')
    if x.dim() != 2 or x.shape[1] != 3 or y.shape[1] != 3:
        raise RuntimeError("knn: only 3-d points are supported")
    b = 1
    if batch_x is not None or batch_y is not None:
        if batch_x is None or batch_y is None:
            raise RuntimeError("knn: give both batch vectors or neither")
        if batch_size is not None:
            b = int(batch_size)
        else:
            last = torch.stack((batch_x[-1], batch_y[-1])).cpu()         # ONE host synchronisation
            b = int(last[0]) + 1
            if int(last[1]) + 1 != b:
                raise RuntimeError("knn: batch_x and batch_y disagree on the batch size")
    nx, ny = x.shape[0] // b, y.shape[0] // b
    if nx * b != x.shape[0] or ny * b != y.shape[0]:
        raise RuntimeError("knn: only equally sized batch items are supported")
    if nx < k:
        raise RuntimeError("knn: fewer candidates per batch item than k")
    row = torch.empty(b * ny * k, dtype=torch.int64, device=x.device)
    col = torch.empty(b * ny * k, dtype=torch.int64, device=x.device)
    _call('dclr_knn', 'knn', b, nx, ny, k, x.data_ptr(), y.data_ptr(), row.data_ptr(), col.data_ptr(),
                                  lib.stream_ptr())
    # upstream (torch-cluster 1.5.9, knn_cuda.cu) drops the slots no candidate was inserted into (squared distance
    # >= 1e10, the slots' initial value): `mask = col != -1` -- a host synchronisation there as here
    mask = col != -1
    return torch.stack((row[mask], col[mask]), dim=0)


# ------------------------------------------------------------------------------------------------
# level 2
# ------------------------------------------------------------------------------------------------
def fps_clouds(clouds: torch.Tensor, npoint: int) -> torch.Tensor:
    """clouds (B, N, C>=3) interleaved -> (B, npoint) int32. Clouds of 16385..65536 points go through the
    workspace variant (sorted points + running minima in a scratch buffer, only ~10 % of it touched per round)."""
    clouds = lib.dev_f32(clouds, 'clouds')
    b, n, c = clouds.shape
    if n > FUSED_MAX_POINTS:
        # beyond the fused samplers (65536 points per cloud): the level-1 operator, which takes any n (running minima in
        # global memory), on a packed copy of the coordinates
        return furthest_point_sample(clouds[:, :, :3].contiguous(), npoint)
    idx = torch.empty(b, npoint, dtype=torch.int32, device=clouds.device)
    need = lib.load().dclr_fps_workspace_bytes(b, n)
    if need > 0 and npoint * 4 <= 32 * 1024:
        ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=clouds.device)
        _call('dclr_fps_clouds_ws', 'fps_clouds[%dx%d]' % (b, n), b, n, c, npoint, clouds.data_ptr(), idx.data_ptr(), ws.data_ptr(),
              need, lib.stream_ptr())
        return idx
    _call('dclr_fps_clouds', 'fps_clouds[%dx%d]' % (b, n), b, n, c, npoint, clouds.data_ptr(), idx.data_ptr(), lib.stream_ptr())
    return idx


def fps_group_layout(n: int):
    """(n_groups, group_size) of the spatial partition the sampling kernel can export, or None."""
    ng, gs = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.load().dclr_fps_group_layout(n, ctypes.addressof(ng), ctypes.addressof(gs))
    return (ng.value, gs.value) if rc == 0 else None


def batch_view(batches) -> Optional[Tuple[int, int, int]]:
    """(pairs per batch, number of batches, stride in floats) when the (2B, N, C) batches of one launch lie at a constant
    stride in memory (the same tensor every time: stride 0; views of one staging chunk; a ring) -- then the grouped sampler
    and set abstraction read them in place (dclr_*_batched) -- else None (the caller concatenates)."""
    first = batches[0]
    if len(batches) < 2 or not first.is_contiguous() or first.dtype != torch.float32 or first.shape[0] % 2:
        return None
    if first.dim() != 3 or fps_group_layout(first.shape[1]) is None:
        return None                 # no grouped sampler at this cloud size (n <= 1024, n > 65536): those launches concatenate
    stride = batches[1].data_ptr() - first.data_ptr()
    if stride < 0 or stride % 4 or (0 < stride < first.numel() * 4):
        return None
    for i, t in enumerate(batches):
        if t.shape != first.shape or t.dtype != first.dtype or t.device != first.device or not t.is_contiguous() \
                or t.data_ptr() != first.data_ptr() + i * stride:
            return None
    return first.shape[0] // 2, len(batches), stride // 4


def fps_clouds_grouped(clouds: torch.Tensor, npoint: int, view: Optional[Tuple[int, int, int]] = None):
    """Sampling plus the kernel's spatial groups: (idx, group_pts, group_box, slice_box); the last three are None when
    the cloud size has no grouped kernel (then set abstraction sweeps exhaustively), slice_box alone where the groups are
    single 64-point slices or come from the workspace kernel (n > 16384).
    view = batch_view([...]): `clouds` is the FIRST of several batches read in place; results cover all of them in the
    concatenated order [templates of every batch | sources of every batch]."""
    clouds = lib.dev_f32(clouds, 'clouds')
    b, n, c = clouds.shape
    layout = fps_group_layout(n)
    if view is not None:
        per, nb, stride = view
        if layout is None or b != 2 * per or (n > 16384 and npoint * 4 > 32 * 1024):
            raise RuntimeError("batch view: no grouped sampler for these clouds (concatenate the batches instead)")
        b = 2 * per * nb
    elif layout is None or (n > 16384 and npoint * 4 > 32 * 1024):
        return fps_clouds(clouds, npoint), None, None, None
    else:
        # one batch: the plain call is the batched one with a single batch (odd cloud counts: no template / source halves)
        per, nb, stride = (b // 2, 1, 0) if b % 2 == 0 else (0, 0, 0)
    ng, gs = layout
    idx = torch.empty(b, npoint, dtype=torch.int32, device=clouds.device)
    gpts = torch.empty(b, ng * gs, 4, dtype=torch.float32, device=clouds.device)
    gbox = torch.empty(b, ng, 8, dtype=torch.float32, device=clouds.device)
    what = 'fps_clouds[%dx%d]' % (b, n)
    if nb == 0:                           # odd number of clouds: the older entry points (no slice boxes)
        if n > 16384:
            need = lib.load().dclr_fps_workspace_bytes(b, n)
            ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=clouds.device)
            _call('dclr_fps_clouds_grouped_ws', what, b, n, c, npoint, clouds.data_ptr(), idx.data_ptr(), gpts.data_ptr(),
                  gbox.data_ptr(), ws.data_ptr(), need, lib.stream_ptr())
        else:
            _call('dclr_fps_clouds_grouped', what, b, n, c, npoint, clouds.data_ptr(), idx.data_ptr(), gpts.data_ptr(),
                  gbox.data_ptr(), lib.stream_ptr())
        return idx, gpts, gbox, None
    sbox = None
    if n <= 16384 and gs > 64:
        sbox = torch.empty(b, ng * (gs // 64), 8, dtype=torch.float32, device=clouds.device)
    need = lib.load().dclr_fps_workspace_bytes(b, n) if n > 16384 else 0
    ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=clouds.device) if need else None
    _call('dclr_fps_clouds_grouped_batched', what, b, n, c, npoint, clouds.data_ptr(), per, nb, stride, idx.data_ptr(),
          gpts.data_ptr(), gbox.data_ptr(), lib.ptr(sbox), lib.ptr(ws), need, lib.stream_ptr())
    return idx, gpts, gbox, sbox


def pack_sa_mlp(weights: Sequence[torch.Tensor], biases: Sequence[torch.Tensor]) -> torch.Tensor:
    """[W1 b1 W2 b2 W3 b3] flat f32 buffer for dclr_sa_msg_fused (1x1 conv weights (out,in,1,1))."""
    parts = []
    for w, bias in zip(weights, biases):
        parts += [w.detach().reshape(w.shape[0], -1).reshape(-1), bias.detach().reshape(-1)]
    return torch.cat(parts).to(torch.float32).contiguous()


def sa_msg_fused(clouds: torch.Tensor, fps_idx: torch.Tensor, radii: Sequence[float], nsamples: Sequence[int],
                 mlps: List[torch.Tensor], want_counts: bool = False, groups=None, precision: Optional[str] = None,
                 view: Optional[Tuple[int, int, int]] = None, overflow: Optional[int] = None):
    """clouds (B,N,C), fps_idx (B,npoint) -> rows F (B*npoint, 68) [, counts (B,npoint,scales)].
    groups: (group_pts, group_box[, slice_box]) from fps_clouds_grouped for the same clouds, or None.
    precision: 'f16x2' (layers 2, 3 of the shared MLP on split-f16 operands) or 'f32'; default ops.PRECISION.
    view: as fps_clouds_grouped (clouds = the first batch, fps_idx / groups cover all batches).
    overflow: device address of the word the split-f16 layers set when an activation is clamped (lib.MappedFlag.dev_ptr),
    for any number of clouds."""
    clouds = lib.dev_f32(clouds, 'clouds')
    b, n, c = clouds.shape
    if view is not None:
        b = 2 * view[0] * view[1]
        if fps_idx.shape[0] != b or clouds.shape[0] != 2 * view[0]:
            raise RuntimeError("batch view: fps_idx must cover all batches of the view")
    npoint = fps_idx.shape[1]
    ns = len(radii)
    out = torch.empty(b * npoint, F_STRIDE, dtype=torch.float32, device=clouds.device)
    counts = torch.empty(b, npoint, ns, dtype=torch.int32, device=clouds.device) if want_counts else None
    radii_h = (ctypes.c_float * ns)(*[float(r) for r in radii])
    nsamp_h = (ctypes.c_int * ns)(*[int(s) for s in nsamples])
    mlp_h = (ctypes.c_void_p * ns)(*[lib.dev_f32(m, 'mlp').data_ptr() for m in mlps])
    sbox = groups[2] if groups is not None and len(groups) > 2 else None
    f16 = int((precision or PRECISION) == 'f16x2')
    if view is None and overflow is not None:
        # one call, any number of clouds (the batched entry below needs an even one: templates | sources)
        _call('dclr_sa_msg_fused_ov', 'sa_msg_fused[%dx%d]' % (b, n), f16, b, n, c, npoint, clouds.data_ptr(), fps_idx.data_ptr(),
              ns, ctypes.cast(radii_h, ctypes.c_void_p), ctypes.cast(nsamp_h, ctypes.c_void_p),
              ctypes.cast(mlp_h, ctypes.c_void_p), out.data_ptr(), lib.ptr(counts),
              None if groups is None else groups[0].data_ptr(), None if groups is None else groups[1].data_ptr(),
              lib.ptr(sbox), overflow, lib.stream_ptr())
        return (out, counts) if want_counts else out
    if view is None and sbox is not None and b % 2 == 0:
        view = (b // 2, 1, 0)                                     # the batched entry with one batch = the plain call
    if view is not None:
        _call('dclr_sa_msg_fused_batched_ov', 'sa_msg_fused[%dx%d]' % (b, n), f16, b, n, c,
              npoint, clouds.data_ptr(), view[0], view[1], view[2], fps_idx.data_ptr(), ns,
              ctypes.cast(radii_h, ctypes.c_void_p), ctypes.cast(nsamp_h, ctypes.c_void_p),
              ctypes.cast(mlp_h, ctypes.c_void_p), out.data_ptr(), lib.ptr(counts),
              None if groups is None else groups[0].data_ptr(), None if groups is None else groups[1].data_ptr(),
              lib.ptr(sbox), overflow, lib.stream_ptr())
        return (out, counts) if want_counts else out
    entry = 'dclr_sa_msg_fused_f16' if f16 else 'dclr_sa_msg_fused'
    _call(entry, 'sa_msg_fused[%dx%d]' % (b, n), b, n, c, npoint, clouds.data_ptr(), fps_idx.data_ptr(), ns,
                                           ctypes.cast(radii_h, ctypes.c_void_p), ctypes.cast(nsamp_h, ctypes.c_void_p),
                                           ctypes.cast(mlp_h, ctypes.c_void_p), out.data_ptr(), lib.ptr(counts),
          None if groups is None else groups[0].data_ptr(), None if groups is None else groups[1].data_ptr(),
          lib.stream_ptr())
    return (out, counts) if want_counts else out


# Size classes of the ragged launches: (1024, 2048], (2048, 4096], ..., (32768, 65536] -- one kernel instance and group
# layout each (fps_group_layout); every buffer of a launch is sized by its class maximum.
RAGGED_CLASSES = (2048, 4096, 8192, 16384, 32768, 65536)


def ragged_class(n: int, npoint: int = 1) -> Optional[int]:
    """Largest point count of the size class a cloud of n points joins in a ragged launch, or None: n <= 1024 or
    n > 65536 (no grouped sampler), or npoint beyond the class's sample buffer in LDS -- such clouds take the per-cloud
    calls."""
    if n <= 1024 or n > FUSED_MAX_POINTS or npoint * 4 > (32 if n > 16384 else 64) * 1024:
        return None
    return next(c for c in RAGGED_CLASSES if n <= c)


def check_cloud_list(clouds) -> Tuple[torch.device, int]:
    """Host-side validation of a list of (N_i, C) clouds (nothing touches the device): (device, C)."""
    if not isinstance(clouds, (list, tuple)) or not clouds:
        raise ValueError("expected a non-empty list of (N_i, C) clouds")
    first = clouds[0]
    for i, x in enumerate(clouds):
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError("cloud {}: expected a 2-D (N, C) tensor, got {}".format(
                i, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if not x.is_cuda:
            raise RuntimeError("cloud {} must be a GPU tensor (deepclr_amd has no CPU path)".format(i))
        if x.dtype != torch.float32:
            raise RuntimeError("cloud {} must be float32".format(i))
        if x.device != first.device:
            raise ValueError("cloud {} is on {}, cloud 0 on {}".format(i, x.device, first.device))
        if x.shape[1] != first.shape[1] or x.shape[1] < 3:
            raise ValueError("cloud {}: {} columns; every cloud needs the same number, at least 3 (cloud 0: {})".format(
                i, x.shape[1], first.shape[1]))
        if x.shape[0] < 1:
            raise ValueError("cloud {} has no points".format(i))
    return first.device, first.shape[1]


def cloud_rows_ragged(clouds: Sequence[torch.Tensor], npoint: int, radii: Sequence[float], nsamples: Sequence[int],
                      mlps: List[torch.Tensor], precision: Optional[str] = None, overflow: Optional[int] = None,
                      single=None, want_counts: bool = False):
    """Sampling + set abstraction of clouds of DIFFERENT sizes: a list of B (N_i, C) GPU tensors -> rows F
    (B*npoint, 68) in input order [, idx (B, npoint) int32, counts (B, npoint, scales) with want_counts].
    The clouds of each size class (RAGGED_CLASSES) go through one sampler launch and one set-abstraction launch
    (dclr_fps_clouds_grouped_ragged / dclr_sa_msg_fused_ragged: per-cloud records, read where the clouds lie); a cloud
    gets exactly the samples, rows and counts it gets alone. Clouds outside the classes take the per-cloud calls:
    `single((1, N, C)) -> rows` where given (the module's own forward_rows, which also covers N > 65536), else the fused
    calls (N <= 65536). precision / overflow: as sa_msg_fused."""
    device, c = check_cloud_list(clouds)
    b = len(clouds)
    classes = [ragged_class(x.shape[0], npoint) for x in clouds]
    if (single is None or want_counts) and any(x.shape[0] > FUSED_MAX_POINTS for x in clouds):
        raise RuntimeError("clouds of more than {} points need the composed set abstraction (pass `single`; no counts)"
                           .format(FUSED_MAX_POINTS))
    clouds = [x.contiguous() for x in clouds]
    # launch order: class by class (ascending), then the per-cloud rest; stable in the input order
    order = sorted(range(b), key=lambda i: (classes[i] is None, classes[i] or 0, i))
    identity = order == list(range(b))
    n_ragged = sum(cl is not None for cl in classes)
    # one pinned host buffer, one copy: the records (pts, n | reserved = 0) of the ragged clouds in launch order, then
    # (only when the launch order is not the input order) the input position of every launched cloud
    recs = torch.empty(2 * n_ragged + (0 if identity else b), dtype=torch.int64, pin_memory=True)
    rv = recs.numpy()
    for k, i in enumerate(order[:n_ragged]):
        rv[2 * k], rv[2 * k + 1] = clouds[i].data_ptr(), clouds[i].shape[0]
    if not identity:
        rv[2 * n_ragged:] = order
    dev = recs.to(device, non_blocking=True) if recs.numel() else None
    ns = len(radii)
    rows = torch.empty(b * npoint, F_STRIDE, dtype=torch.float32, device=device)
    out_rows = rows if identity else torch.empty_like(rows)            # launch order
    idx_all = torch.empty(b, npoint, dtype=torch.int32, device=device) if want_counts else None
    cnt_all = torch.empty(b, npoint, ns, dtype=torch.int32, device=device) if want_counts else None
    radii_h = (ctypes.c_float * ns)(*[float(r) for r in radii])
    nsamp_h = (ctypes.c_int * ns)(*[int(s) for s in nsamples])
    mlp_h = (ctypes.c_void_p * ns)(*[lib.dev_f32(m, 'mlp').data_ptr() for m in mlps])
    f16 = int((precision or PRECISION) == 'f16x2')
    k = 0
    while k < n_ragged:
        cls = classes[order[k]]
        e = k
        while e < n_ragged and classes[order[e]] == cls:
            e += 1
        nb = e - k
        ng, gs = fps_group_layout(cls)
        refs = dev.data_ptr() + 16 * k
        idx = idx_all[k:e] if want_counts else torch.empty(nb, npoint, dtype=torch.int32, device=device)
        gpts = torch.empty(nb, ng * gs, 4, dtype=torch.float32, device=device)
        gbox = torch.empty(nb, ng, 8, dtype=torch.float32, device=device)
        sbox = torch.empty(nb, ng * (gs // 64), 8, dtype=torch.float32, device=device) if cls <= 16384 and gs > 64 else None
        need = lib.load().dclr_fps_workspace_bytes(nb, cls) if cls > 16384 else 0
        ws = torch.empty((need + 3) // 4, dtype=torch.int32, device=device) if need else None
        _call('dclr_fps_clouds_grouped_ragged', 'fps_ragged[%dx%d]' % (nb, cls), nb, cls, c, npoint, refs, idx.data_ptr(),
              gpts.data_ptr(), gbox.data_ptr(), lib.ptr(sbox), lib.ptr(ws), need, lib.stream_ptr())
        _call('dclr_sa_msg_fused_ragged', 'sa_msg_ragged[%dx%d]' % (nb, cls), f16, nb, cls, c, npoint, refs, idx.data_ptr(), ns,
              ctypes.cast(radii_h, ctypes.c_void_p), ctypes.cast(nsamp_h, ctypes.c_void_p), ctypes.cast(mlp_h, ctypes.c_void_p),
              out_rows[k * npoint:e * npoint].data_ptr(), lib.ptr(cnt_all[k:e] if want_counts else None), gpts.data_ptr(),
              gbox.data_ptr(), lib.ptr(sbox), overflow, lib.stream_ptr())
        k = e
    for k in range(n_ragged, b):                                       # outside the classes: one cloud per call
        x1 = clouds[order[k]].unsqueeze(0)
        dst = out_rows[k * npoint:(k + 1) * npoint]
        if single is not None and not want_counts:
            dst.copy_(single(x1))
            continue
        fps, gpts, gbox, sbox = fps_clouds_grouped(x1, npoint)
        groups = None if gpts is None else (gpts, gbox) + (() if sbox is None else (sbox,))
        got = sa_msg_fused(x1, fps, radii, nsamples, mlps, want_counts=want_counts, groups=groups, precision=precision,
                           overflow=overflow)
        if want_counts:
            got, cnt = got
            idx_all[k].copy_(fps[0])
            cnt_all[k].copy_(cnt[0])
        dst.copy_(got)
    if not identity:                                                   # launch order -> input order: one scatter
        perm = dev[2 * n_ragged:]
        rows.view(b, npoint, F_STRIDE).index_copy_(0, perm, out_rows.view(b, npoint, F_STRIDE))
        if want_counts:
            idx_all = torch.empty_like(idx_all).index_copy_(0, perm, idx_all)
            cnt_all = torch.empty_like(cnt_all).index_copy_(0, perm, cnt_all)
    return (rows, idx_all, cnt_all) if want_counts else rows


def _xyz_col(stride: int) -> int:
    return {F_STRIDE: 64, E_STRIDE: 256}[stride]


def rows_to_channels(rows: torch.Tensor, b: int, npoint: int, nfeat: int) -> torch.Tensor:
    """rows F / E (b*npoint, stride) -> reference layout (b, 3 + nfeat, npoint) [xyz | first nfeat features]."""
    rows = lib.dev_f32(rows, 'rows')
    out = torch.empty(b, 3 + nfeat, npoint, dtype=torch.float32, device=rows.device)
    _call('dclr_rows_to_channels', 'rows_to_channels', b, npoint, nfeat, _xyz_col(rows.shape[1]), rows.shape[1],
                                               rows.data_ptr(), out.data_ptr(), lib.stream_ptr())
    return out


def channels_to_rows(channels: torch.Tensor, stride: int) -> torch.Tensor:
    """reference layout (b, 3 + nfeat, npoint) -> rows (b*npoint, stride)."""
    channels = lib.dev_f32(channels, 'channels')
    b, ch, npoint = channels.shape
    rows = torch.empty(b * npoint, stride, dtype=torch.float32, device=channels.device)
    _call('dclr_channels_to_rows', 'channels_to_rows', b, npoint, ch - 3, _xyz_col(stride), stride, channels.data_ptr(),
                                               rows.data_ptr(), lib.stream_ptr())
    return rows


def pack_weight(w: torch.Tensor, kp: int, kmap: Optional[torch.Tensor] = None, tile16: bool = False) -> torch.Tensor:
    """Row-major (n_out, k_in) -> MFMA fragment order, K padded to kp, N padded to a multiple of 32
    (tile16: the 16-column layout of the fused flow-embedding kernel, N padded to a multiple of 16)."""
    w = lib.dev_f32(w.detach().reshape(w.shape[0], -1).contiguous(), 'w')
    n_out, k_in = w.shape
    if tile16:
        np_ = (n_out + 15) // 16 * 16
        packed = torch.empty(np_ * kp, dtype=torch.float32, device=w.device)
        _call('dclr_pack_weight16', 'pack_weight16', n_out, k_in, w.data_ptr(), lib.ptr(kmap), kp, np_,
              packed.data_ptr(), lib.stream_ptr())
        return packed
    np_ = (n_out + 31) // 32 * 32
    packed = torch.empty(np_ * kp, dtype=torch.float32, device=w.device)
    if kmap is not None:
        assert kmap.dtype == torch.int32 and kmap.numel() == kp and kmap.is_cuda
    _call('dclr_pack_weight', 'pack_weight', n_out, k_in, w.data_ptr(), lib.ptr(kmap), kp, np_, packed.data_ptr(),
                                          lib.stream_ptr())
    return packed


def linear(x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], n: int, kp: int, relu: bool,
           ldy: Optional[int] = None, colmax_groups: Optional[int] = None) -> torch.Tensor:
    """rows x (m, ldx) -> rows y (m, ldy) = act(x[:, :kp] W^T + b), or, with colmax_groups = G,
    the (G, n) column maxima over each block of m/G rows."""
    x = lib.dev_f32(x, 'x')
    m, ldx = x.shape
    if colmax_groups is not None:
        out = torch.zeros(colmax_groups, n, dtype=torch.float32, device=x.device)
        _call('dclr_linear', 'linear+colmax[%dx%dx%d]' % (m, n, kp), m, n, kp, x.data_ptr(), ldx, w_packed.data_ptr(), lib.ptr(bias), 1, None, 0,
                                         out.data_ptr(), m // colmax_groups, lib.stream_ptr())
        return out
    ldy = n if ldy is None else ldy
    alloc = torch.zeros if ldy > n else torch.empty     # padding columns feed the next layer's zero weights
    y = alloc(m, ldy, dtype=torch.float32, device=x.device)
    _call('dclr_linear', 'linear[%dx%dx%d]' % (m, n, kp), m, n, kp, x.data_ptr(), ldx, w_packed.data_ptr(), lib.ptr(bias), int(relu),
                                     y.data_ptr(), ldy, None, 0, lib.stream_ptr())
    return y


def head_conv_fused(x: torch.Tensor, layers, groups: int) -> torch.Tensor:
    """x rows (m, ldx); layers = [(w_packed, bias, n, kp), ...] -> (groups, n_last) column maxima of the
    ReLU'd last layer over each block of m / groups rows (the conv chain of the pose head in one launch)."""
    x = lib.dev_f32(x, 'x')
    m, ldx = x.shape
    nl = len(layers)
    k_h = (ctypes.c_int * nl)(*[int(l[3]) for l in layers])
    n_h = (ctypes.c_int * nl)(*[int(l[2]) for l in layers])
    w_h = (ctypes.c_void_p * nl)(*[l[0].data_ptr() for l in layers])
    b_h = (ctypes.c_void_p * nl)(*[l[1].data_ptr() for l in layers])
    out = torch.zeros(groups, layers[-1][2], dtype=torch.float32, device=x.device)
    _call('dclr_head_conv_fused', 'head_conv_fused[%dx%d]' % (groups, m // groups), m, nl, ctypes.cast(k_h, ctypes.c_void_p), ctypes.cast(n_h, ctypes.c_void_p),
          ctypes.cast(w_h, ctypes.c_void_p), ctypes.cast(b_h, ctypes.c_void_p), x.data_ptr(), ldx, out.data_ptr(),
          m // groups, lib.stream_ptr())
    return out


def pack_weight_f16(w: torch.Tensor, kp: int, width: int, kmap: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row-major (n_out, k_in) -> split-fp16 fragments (hi plane | lo plane) for `width`-column MFMA tiles."""
    w = lib.dev_f32(w.detach().reshape(w.shape[0], -1).contiguous(), 'w')
    check_f16_range(w, 'pack_weight_f16')
    n_out, k_in = w.shape
    np_ = (n_out + width - 1) // width * width
    packed = torch.empty(np_ * kp, dtype=torch.float32, device=w.device)          # 2 planes of np*kp halves
    if kmap is not None:
        assert kmap.dtype == torch.int32 and kmap.numel() == kp and kmap.is_cuda
    _call('dclr_pack_weight_f16', 'pack_weight_f16', n_out, k_in, w.data_ptr(), lib.ptr(kmap), kp, width,
          packed.data_ptr(), lib.stream_ptr())
    return packed


def head_conv_fused_f16(x: torch.Tensor, k_in: int, layers, groups: int) -> torch.Tensor:
    """head_conv_fused on the split-fp16 matrix path; layers = [(w_packed_f16, bias, n, kp), ...], kp % 16 == 0."""
    x = lib.dev_f32(x, 'x')
    m, ldx = x.shape
    nl = len(layers)
    k_h = (ctypes.c_int * nl)(*[int(l[3]) for l in layers])
    n_h = (ctypes.c_int * nl)(*[int(l[2]) for l in layers])
    w_h = (ctypes.c_void_p * nl)(*[l[0].data_ptr() for l in layers])
    b_h = (ctypes.c_void_p * nl)(*[l[1].data_ptr() for l in layers])
    out = torch.zeros(groups, layers[-1][2], dtype=torch.float32, device=x.device)
    _call('dclr_head_conv_fused_f16', 'head_conv_fused[%dx%d]' % (groups, m // groups), m, nl, int(k_in), ctypes.cast(k_h, ctypes.c_void_p),
          ctypes.cast(n_h, ctypes.c_void_p), ctypes.cast(w_h, ctypes.c_void_p), ctypes.cast(b_h, ctypes.c_void_p),
          x.data_ptr(), ldx, out.data_ptr(), m // groups, lib.stream_ptr())
    return out


def flow_f16_tile(k: int) -> int:
    """Tile width the library's split-f16 flow kernel wants its layer-2 / layer-3 weights packed with when it runs k
    neighbours per point (32 from k = 29 up, 16 below)."""
    return int(lib.load().dclr_flow_f16_tile(int(k)))


def flow_embedding_fused_f16(f_rows: torch.Tensor, knn_idx: torch.Tensor, pt: torch.Tensor, ps: torch.Tensor,
                             w1a: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor,
                             w3p: torch.Tensor, b3: torch.Tensor, radius: float) -> torch.Tensor:
    pairs, npoint, k = knn_idx.shape
    e = torch.empty(pairs * npoint, E_STRIDE, dtype=torch.float32, device=f_rows.device)
    _call('dclr_flow_embedding_fused_f16', 'flow_embedding[%dx%dx%d]' % (pairs, npoint, k), pairs, npoint, k, float(radius), f_rows.data_ptr(),
          knn_idx.data_ptr(), pt.data_ptr(), ps.data_ptr(), w1a.data_ptr(), b1.data_ptr(), w2p.data_ptr(),
          b2.data_ptr(), w3p.data_ptr(), b3.data_ptr(), e.data_ptr(), lib.stream_ptr())
    return e


def knn_rows(f_rows: torch.Tensor, pairs: int, npoint: int, k: int) -> torch.Tensor:
    f_rows = lib.dev_f32(f_rows, 'f_rows')
    idx = torch.empty(pairs, npoint, k, dtype=torch.int32, device=f_rows.device)
    _call('dclr_knn_rows', 'knn_rows[%dx%dx%d]' % (pairs, npoint, k), pairs, npoint, k, f_rows.data_ptr(), idx.data_ptr(), lib.stream_ptr())
    return idx


def flow_embedding_fused(f_rows: torch.Tensor, knn_idx: torch.Tensor, pt: torch.Tensor, ps: torch.Tensor,
                         w1a: torch.Tensor, b1: torch.Tensor, w2p: torch.Tensor, b2: torch.Tensor,
                         w3p: torch.Tensor, b3: torch.Tensor, radius: float) -> torch.Tensor:
    pairs, npoint, k = knn_idx.shape
    e = torch.empty(pairs * npoint, E_STRIDE, dtype=torch.float32, device=f_rows.device)
    _call('dclr_flow_embedding_fused', 'flow_embedding[%dx%dx%d]' % (pairs, npoint, k), pairs, npoint, k, float(radius), f_rows.data_ptr(),
                                                   knn_idx.data_ptr(), pt.data_ptr(), ps.data_ptr(), w1a.data_ptr(),
                                                   b1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), w3p.data_ptr(),
                                                   b3.data_ptr(), e.data_ptr(), lib.stream_ptr())
    return e


def fc(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act: int) -> torch.Tensor:
    """act(x @ w.T + bias): x (m, k), w (n, k), bias (n,) or None; act 0 none, 1 relu, 2 dual quaternion (sigmoid on
    column 0, tanh on 1..3), 3 quaternion (sigmoid on column 3, tanh on 4..)."""
    x, w = lib.dev_f32(x, 'x'), lib.dev_f32(w, 'w')
    if x.dim() != 2 or w.dim() != 2 or w.shape[1] != x.shape[1]:
        raise RuntimeError("fc: x (m, k) and w (n, k) expected, got {} and {}".format(tuple(x.shape), tuple(w.shape)))
    m, k = x.shape
    n = w.shape[0]
    if bias is not None and tuple(lib.dev_f32(bias, 'bias').shape) != (n,):
        raise RuntimeError("fc: bias of shape ({},) expected, got {}".format(n, tuple(bias.shape)))
    y = torch.empty(m, n, dtype=torch.float32, device=x.device)
    _call('dclr_fc', 'fc[%d]' % m, m, n, k, x.data_ptr(), w.data_ptr(), lib.ptr(bias), act, y.data_ptr(),
                                 lib.stream_ptr())
    return y


# ------------------------------------------------------------------------------------------------
# training: the fused set abstraction's forward with argmax and its weight backward (libdeepclr_amd_train.so)
# ------------------------------------------------------------------------------------------------
SA_TRAIN_MLP_FLOATS = 896           # per scale: W1 (16 x 4) b1 W2 (16 x 16) b2 W3 (32 x 16) b3 (include/deepclr_amd_train.h)


def _call_train(name: str, what: str, *args) -> None:
    lib.check(getattr(lib.load_train(), name)(*args), what)


def pack_sa_train_mlp(params: Sequence[torch.Tensor], in_feat: int) -> torch.Tensor:
    """Conv weights / biases of the scales, in order [W1 b1 W2 b2 W3 b3] per scale (W (out, in, 1, 1)) -> the flat
    (scales * 896) buffer of dclr_sa_msg_train_*; W1's feature column is zero when in_feat = 0. Built from the tensors as
    they are at the call (an optimizer step updates them in place), without gradient (SAMsgTrainFunction has the backward)."""
    parts = []
    for j in range(0, len(params), 6):
        w1, b1, w2, b2, w3, b3 = (t.detach() for t in params[j:j + 6])
        w1 = w1.reshape(16, 3 + in_feat)
        if in_feat == 0:
            w1 = torch.cat((w1, w1.new_zeros(16, 1)), dim=1)
        parts += [w1.reshape(-1), b1.reshape(-1), w2.reshape(-1), b2.reshape(-1), w3.reshape(-1), b3.reshape(-1)]
    return torch.cat(parts).to(torch.float32).contiguous()


def sa_msg_train_forward(xyz: torch.Tensor, feats: Optional[torch.Tensor], new_xyz: torch.Tensor,
                         idx: Sequence[torch.Tensor], weights: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """xyz (B, N, 3), feats (B, f, N) (f <= 1) or None, new_xyz (B, npoint, 3), idx: per scale the ball query
    (B, npoint, nsample) int32, weights (scales * 896) -> features (B, 32 * scales, npoint) and arg (same shape, int32):
    the point index of the first slot reaching each maximum."""
    xyz, new_xyz, weights = lib.dev_f32(xyz, 'xyz'), lib.dev_f32(new_xyz, 'new_xyz'), lib.dev_f32(weights, 'weights')
    b, n, _ = xyz.shape
    npoint = new_xyz.shape[1]
    f = 0 if feats is None else lib.dev_f32(feats, 'feats').shape[1]
    scales = len(idx)
    for t in idx:
        if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.shape[:2] == (b, npoint)):
            raise RuntimeError("idx: (B, npoint, nsample) int32 contiguous GPU tensors from ball_query")
    if weights.numel() != scales * SA_TRAIN_MLP_FLOATS:
        raise RuntimeError("weights: {} floats for {} scales".format(scales * SA_TRAIN_MLP_FLOATS, scales))
    features = torch.empty(b, 32 * scales, npoint, dtype=torch.float32, device=xyz.device)
    arg = torch.empty(b, 32 * scales, npoint, dtype=torch.int32, device=xyz.device)
    ns = (ctypes.c_int * scales)(*[t.shape[2] for t in idx])
    ptrs = (ctypes.c_void_p * scales)(*[t.data_ptr() for t in idx])
    _call_train('dclr_sa_msg_train_forward', 'sa_msg_train_forward', b, n, f, npoint, scales, ns, xyz.data_ptr(),
                lib.ptr(feats), new_xyz.data_ptr(), ptrs, weights.data_ptr(), features.data_ptr(), arg.data_ptr(),
                lib.stream_ptr())
    return features, arg


def sa_msg_train_workspace_bytes(b: int, npoint: int, scales: int) -> int:
    nbytes = lib.load_train().dclr_sa_msg_train_workspace_bytes(b, npoint, scales)
    lib.check(nbytes if nbytes < 0 else 0, 'sa_msg_train_workspace_bytes')
    return nbytes


def sa_msg_train_backward(grad_out: torch.Tensor, arg: torch.Tensor, xyz: torch.Tensor, feats: Optional[torch.Tensor],
                          new_xyz: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """grad_out (B, 32 * scales, npoint) and arg from sa_msg_train_forward on the same inputs -> the gradient of
    `weights` (scales * 896), bit-identical from run to run."""
    grad_out = lib.dev_f32(grad_out, 'grad_out')
    xyz, new_xyz, weights = lib.dev_f32(xyz, 'xyz'), lib.dev_f32(new_xyz, 'new_xyz'), lib.dev_f32(weights, 'weights')
    b, n, _ = xyz.shape
    npoint = new_xyz.shape[1]
    f = 0 if feats is None else lib.dev_f32(feats, 'feats').shape[1]
    scales = weights.numel() // SA_TRAIN_MLP_FLOATS
    if not (arg.is_cuda and arg.dtype == torch.int32 and arg.is_contiguous() and arg.shape == grad_out.shape
            and tuple(grad_out.shape) == (b, 32 * scales, npoint)):
        raise RuntimeError("grad_out / arg: (B, 32 * scales, npoint), arg int32 from sa_msg_train_forward")
    nbytes = sa_msg_train_workspace_bytes(b, npoint, scales)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=xyz.device)
    grad = torch.empty(scales * SA_TRAIN_MLP_FLOATS, dtype=torch.float32, device=xyz.device)
    _call_train('dclr_sa_msg_train_backward', 'sa_msg_train_backward', b, n, f, npoint, scales, xyz.data_ptr(),
                lib.ptr(feats), new_xyz.data_ptr(), weights.data_ptr(), grad_out.data_ptr(), arg.data_ptr(),
                grad.data_ptr(), ws.data_ptr(), nbytes, lib.stream_ptr())
    return grad


# ------------------------------------------------------------------------------------------------
# training: the fused flow embedding's forward with argmax and its backward (libdeepclr_amd_flow_train.so)
# ------------------------------------------------------------------------------------------------
FLOW_TRAIN_GRAD_FLOATS = 66432      # W1 (128 x 131) b1 W2 (128 x 128) b2 W3 (256 x 128) b3 (include/deepclr_amd_flow_train.h)
FLOW_TRAIN_MLP_FLOATS = 101248      # ... then W2^T (128 x 128) and W1^T padded to (144 x 128)
FLOW_TRAIN_FEAT = 64


def _call_flow_train(name: str, what: str, *args) -> None:
    lib.check(getattr(lib.load_flow_train(), name)(*args), what)


def pack_flow_train_mlp(params: Sequence[torch.Tensor]) -> torch.Tensor:
    """Conv weights / biases [W1 b1 W2 b2 W3 b3] of the flow embedding's 131 -> 128 -> 128 -> 256 MLP (W (out, in, 1))
    -> the flat buffer of dclr_flow_train_*. Built from the tensors as they are at the call (an optimizer step updates
    them in place), without gradient (FlowTrainFunction has the backward)."""
    w1, b1, w2, b2, w3, b3 = (t.detach().to(torch.float32) for t in params)
    w1, w2, w3 = w1.reshape(128, 131), w2.reshape(128, 128), w3.reshape(256, 128)
    w1t = torch.cat((w1.t(), w1.new_zeros(144 - 131, 128)), dim=0)
    return torch.cat([t.reshape(-1) for t in (w1, b1, w2, b2, w3, b3, w2.t().contiguous(), w1t.contiguous())]).contiguous()


def _flow_clouds(cloud0: torch.Tensor, cloud1: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    for name, t in (('cloud0', cloud0), ('cloud1', cloud1)):
        lib.dev_f32(t, name)
        if t.dim() != 3 or t.shape[2] != 3 + FLOW_TRAIN_FEAT:
            raise RuntimeError("{}: (pairs, n, 67) point-major rows [xyz | 64 features] expected, got {}".format(
                name, tuple(t.shape)))
    if cloud0.shape[0] != cloud1.shape[0]:
        raise RuntimeError("cloud0 / cloud1: the same number of pairs")
    return cloud0, cloud1


def flow_train_forward(cloud0: torch.Tensor, cloud1: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor,
                       radius: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """cloud0 (B, P0, 67), cloud1 (B, P1, 67) point-major, idx (B, P0, k) int32 source points, weights from
    pack_flow_train_mlp -> pooled (B, 256, P0), arg (B, 256, P0) int32 (first slot reaching each maximum), pt (B, P0, 128)
    and ps (B, P1, 128) (the layer-1 feature products the backward reuses)."""
    cloud0, cloud1 = _flow_clouds(cloud0, cloud1)
    weights = lib.dev_f32(weights, 'weights')
    b, n0, _ = cloud0.shape
    n1 = cloud1.shape[1]
    if not (idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 3
            and tuple(idx.shape[:2]) == (b, n0)):
        raise RuntimeError("idx: (B, P0, k) int32 contiguous GPU tensor")
    if weights.numel() != FLOW_TRAIN_MLP_FLOATS:
        raise RuntimeError("weights: {} floats expected (pack_flow_train_mlp)".format(FLOW_TRAIN_MLP_FLOATS))
    k = idx.shape[2]
    dev = cloud0.device
    pt = torch.empty(b, n0, 128, dtype=torch.float32, device=dev)
    ps = torch.empty(b, n1, 128, dtype=torch.float32, device=dev)
    pooled = torch.empty(b, 256, n0, dtype=torch.float32, device=dev)
    arg = torch.empty(b, 256, n0, dtype=torch.int32, device=dev)
    _call_flow_train('dclr_flow_train_forward', 'flow_train_forward', b, n0, n1, k, FLOW_TRAIN_FEAT, float(radius),
                     cloud0.data_ptr(), cloud1.data_ptr(), idx.data_ptr(), weights.data_ptr(), pt.data_ptr(),
                     ps.data_ptr(), pooled.data_ptr(), arg.data_ptr(), lib.stream_ptr())
    return pooled, arg, pt, ps


def flow_train_workspace_bytes(pairs: int, n0: int, n1: int, k: int) -> int:
    nbytes = lib.load_flow_train().dclr_flow_train_workspace_bytes(pairs, n0, n1, k)
    lib.check(nbytes if nbytes < 0 else 0, 'flow_train_workspace_bytes')
    return nbytes


def flow_train_backward(grad_pooled: torch.Tensor, cloud0: torch.Tensor, cloud1: torch.Tensor, idx: torch.Tensor,
                        weights: torch.Tensor, pt: torch.Tensor, ps: torch.Tensor, pooled: torch.Tensor,
                        arg: torch.Tensor, input_grads: bool = True
                        ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """grad_pooled (B, 256, P0) and the outputs of flow_train_forward on the same inputs -> the gradient of the first
    FLOW_TRAIN_GRAD_FLOATS floats of `weights` and, with input_grads, of cloud0 / cloud1 (point-major, like them; cloud0's
    xyz columns without the gradient of the xyz rows the caller copies into its output). Bit-identical from run to run."""
    cloud0, cloud1 = _flow_clouds(cloud0, cloud1)
    grad_pooled = lib.dev_f32(grad_pooled, 'grad_pooled')
    b, n0, _ = cloud0.shape
    n1, k = cloud1.shape[1], idx.shape[2]
    for name, t in (('pooled', pooled), ('arg', arg), ('grad_pooled', grad_pooled)):
        if tuple(t.shape) != (b, 256, n0) or not t.is_contiguous():
            raise RuntimeError("{}: (B, 256, P0) contiguous expected".format(name))
    if tuple(pt.shape) != (b, n0, 128) or tuple(ps.shape) != (b, n1, 128) or arg.dtype != torch.int32:
        raise RuntimeError("pt / ps / arg: the outputs of flow_train_forward on the same clouds")
    dev = cloud0.device
    nbytes = flow_train_workspace_bytes(b, n0, n1, k)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    grad = torch.empty(FLOW_TRAIN_GRAD_FLOATS, dtype=torch.float32, device=dev)
    g0 = torch.empty(b, n0, 67, dtype=torch.float32, device=dev) if input_grads else None
    g1 = torch.empty(b, n1, 67, dtype=torch.float32, device=dev) if input_grads else None
    _call_flow_train('dclr_flow_train_backward', 'flow_train_backward', b, n0, n1, k, FLOW_TRAIN_FEAT,
                     cloud0.data_ptr(), cloud1.data_ptr(), idx.data_ptr(), weights.data_ptr(), pt.data_ptr(),
                     ps.data_ptr(), pooled.data_ptr(), arg.data_ptr(), grad_pooled.data_ptr(), grad.data_ptr(),
                     int(bool(input_grads)), lib.ptr(g0), lib.ptr(g1), ws.data_ptr(), nbytes, lib.stream_ptr())
    return grad, g0, g1
