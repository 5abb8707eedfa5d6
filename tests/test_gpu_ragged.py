"""GPU: clouds of different point counts in one launch per size class (ops.cloud_rows_ragged, the list forms of
DeepCLR.cloud_feature_rows / cloud_features and ModelInferenceHelper.predict_sequence / predict_batch).

A cloud in a ragged launch must get exactly what it gets alone: the same samples (the oracle's), the same neighbour counts
and bit-identical feature rows -- the per-centroid arithmetic is the same, only the cloud's base address and size come
from its record."""
import numpy as np
import pytest
import torch

import oracle
from deepclr_amd import ops, synthetic
from deepclr_amd.config import model_config_from_dict
from deepclr_amd.labels import LabelType
from deepclr_amd.models import build_model, ModelInferenceHelper
from helpers import small_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL, ATOL = 1e-5, 1e-6                       # as tests/test_gpu_entry_points.py
POSE_ATOL = 1e-4


def _cloud(i: int, n: int) -> torch.Tensor:
    """Even i: a LiDAR ring scan cut to n points (dense near field: ball queries reach their caps); odd i: Gaussian."""
    if i % 2 == 0:
        return torch.from_numpy(synthetic.ring_scan(np.random.default_rng(77 + i), (n + 31) // 32 * 32)[:n].astype(np.float32))
    return torch.from_numpy(synthetic.kitti_like_pair(i, n)[0])


def _model(cfg, seed=0):
    sd = synthetic.random_state_dict(cfg, seed=seed)
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval(), oracle.build_oracle_model(cfg, sd)


def _alone(sam, x1):
    """Samples, rows and counts of one cloud (1, N, C) through the tensor entry points."""
    fps, gpts, gbox, sbox = ops.fps_clouds_grouped(x1, sam.npoint)
    groups = None if gpts is None else (gpts, gbox) + (() if sbox is None else (sbox,))
    rows, counts = ops.sa_msg_fused(x1, fps, sam.radii, sam.nsamples, sam.packed_mlps(), want_counts=True, groups=groups)
    return fps[0], rows, counts[0]


def _check_against_alone(model, clouds_h, oracle_fps=True):
    sam = model._cloud_layers[0]._sa0
    clouds = [x.to(DEV) for x in clouds_h]
    rows, idx, counts = ops.cloud_rows_ragged(clouds, sam.npoint, sam.radii, sam.nsamples, sam.packed_mlps(), want_counts=True)
    with torch.no_grad():
        rows_model = model.cloud_feature_rows(clouds)
    assert torch.equal(rows_model[:, :67], rows[:, :67])
    rows = rows.view(len(clouds), sam.npoint, -1)
    for i, x in enumerate(clouds):
        what = (i, x.shape[0])
        fps1, rows1, counts1 = _alone(sam, x.unsqueeze(0))
        assert torch.equal(idx[i], fps1), what
        if oracle_fps:
            assert torch.equal(idx[i].cpu(), oracle.furthest_point_sample(clouds_h[i][None, :, :3].contiguous(), sam.npoint)[0]), what
        assert torch.equal(counts[i], counts1), what
        assert torch.equal(rows[i, :, :67], rows1[:, :67]), what              # (column 67: padding)
        with torch.no_grad():
            assert torch.equal(rows[i, :, :67], model.cloud_feature_rows(x.unsqueeze(0))[:, :67]), what


def test_every_size_class_gives_each_cloud_what_it_gets_alone():
    sizes = [1025, 2048, 2049, 3000, 5000, 8193, 16384, 16385, 30000, 32769, 50000, 65536]
    order = np.random.default_rng(3).permutation(len(sizes))
    clouds_h = [_cloud(i, sizes[j]) for i, j in enumerate(order)]
    model, _ = _model(synthetic.model_cfg('kitti'))
    _check_against_alone(model, clouds_h)


def test_clouds_outside_the_classes_take_the_per_cloud_calls():
    cfg = small_cfg()
    model, _ = _model(cfg)
    sizes = [96, 40, 1000, 3000, 20000]                                    # 40 < npoint = 64
    _check_against_alone(model, [_cloud(i, n) for i, n in enumerate(sizes)])
    big = [_cloud(0, 3000), _cloud(1, 70000), _cloud(2, 1000)]
    clouds = [x.to(DEV) for x in big]
    sam = model._cloud_layers[0]._sa0
    with pytest.raises(RuntimeError, match='composed'):
        ops.cloud_rows_ragged(clouds, sam.npoint, sam.radii, sam.nsamples, sam.packed_mlps())
    with torch.no_grad():
        rows = model.cloud_feature_rows(clouds).view(3, sam.npoint, -1)
        for i, x in enumerate(clouds):
            assert torch.equal(rows[i, :, :67], model.cloud_feature_rows(x.unsqueeze(0))[:, :67]), i


def _mats(y) -> np.ndarray:
    return np.stack([LabelType.POSE3D_DUAL_QUAT.to_matrix(v) for v in np.asarray(y, dtype=np.float64)])


def _close(got, want, what):
    got, want = got.detach().cpu(), torch.as_tensor(want, dtype=torch.float32)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    scale = max(1.0, float(want.abs().max()))
    assert torch.allclose(got, want, rtol=RTOL, atol=ATOL * scale), (what, float((got - want).abs().max()))
    assert float(np.abs(_mats(got.numpy()) - _mats(want.numpy())).max()) < POSE_ATOL, what


def _oracle_pair(orc, t, s):
    with torch.no_grad():
        feats = torch.cat((orc.cloud_features(t[None]), orc.cloud_features(s[None])))
        return orc(feats, is_feat=True)[0]


def test_predict_sequence_on_frames_of_varying_size():
    model, orc = _model(small_cfg(), seed=1)
    sizes = [3000, 1500, 5000, 4000, 4000, 1200, 9000]
    frames_h = [_cloud(i, n) for i, n in enumerate(sizes)]
    frames = [f.to(DEV) for f in frames_h]
    loop = ModelInferenceHelper(model, is_sequential=True)
    want = [loop.predict(f) for f in frames]
    loop.finish()
    assert want[0] is None
    want = torch.stack(want[1:])
    seq = ModelInferenceHelper(model, is_sequential=True)
    parts = [seq.predict_sequence(frames[0:3]),                            # fresh state: one pose fewer than frames
             seq.predict_sequence(torch.stack(frames[3:5])),               # a tensor chunk between two lists
             seq.predict_sequence(tuple(frames[5:7]))]
    assert [p.shape[0] for p in parts] == [2, 2, 2]
    got = torch.cat(parts)
    _close(got, want.cpu(), 'predict loop')
    for i in range(len(frames) - 1):
        _close(got[i:i + 1], _oracle_pair(orc, frames_h[i], frames_h[i + 1])[None], ('oracle', i))
    one = ModelInferenceHelper(model, is_sequential=True)
    assert one.predict_sequence([frames[0]]).shape[0] == 0 and one.has_state()      # the carry of a one-frame chunk
    _close(one.predict_sequence([frames[1]]), want[:1].cpu(), 'carry')


def test_predict_batch_on_pairs_of_unequal_sizes():
    model, orc = _model(small_cfg(), seed=2)
    t_h = [_cloud(i, n) for i, n in enumerate([3000, 1500, 9000, 2049])]
    s_h = [_cloud(10 + i, n) for i, n in enumerate([2500, 7000, 9000, 1000])]
    helper = ModelInferenceHelper(model)
    got = helper.predict_batch([s.to(DEV) for s in s_h], [t.to(DEV) for t in t_h])
    assert got.shape[0] == 4
    for i, (t, s) in enumerate(zip(t_h, s_h)):
        with torch.no_grad():
            feats = torch.cat((model.cloud_features([t.to(DEV)]), model.cloud_features([s.to(DEV)])))
            pair = model.forward(feats, is_feat=True)[0]
        _close(got[i:i + 1], pair.cpu(), ('pair', i))
        _close(got[i:i + 1], _oracle_pair(orc, t, s)[None], ('oracle', i))


def test_equal_sizes_as_a_list_match_the_tensor_path_bit_for_bit():
    model, _ = _model(synthetic.model_cfg('kitti'), seed=3)
    frames = torch.stack([_cloud(i, 4096) for i in range(5)]).to(DEV)
    a = ModelInferenceHelper(model, is_sequential=True).predict_sequence(frames)
    b = ModelInferenceHelper(model, is_sequential=True).predict_sequence(list(frames.unbind(0)))
    assert a.shape[0] == 4 and torch.equal(a, b)
    with torch.no_grad():
        fa = model.cloud_features(frames.clone())
        fb = model.cloud_features(list(frames.unbind(0)))
    assert torch.equal(fa, fb)


SA_SCALE, HOT = 15.0, 2.0e4      # tests/test_gpu_entry_points.py: set-abstraction layer 2 passes 65504 on hot clouds only


def test_a_hot_frame_in_a_ragged_chunk_never_yields_a_finite_pose():
    if ops.PRECISION != 'f16x2' or ops.CHECK_RANGE == 'never':
        pytest.skip('the range contract belongs to the split-f16 path with range checks')
    cfg = small_cfg()
    sd = synthetic.random_state_dict(cfg, seed=5)
    for s in range(2):
        sd['_cloud_layers.0._sa0.mlps.%d.layer1.conv.weight' % s] = sd['_cloud_layers.0._sa0.mlps.%d.layer1.conv.weight' % s] * SA_SCALE
        sd['_cloud_layers.0._sa0.mlps.%d.layer2.conv.weight' % s] = sd['_cloud_layers.0._sa0.mlps.%d.layer2.conv.weight' % s] / SA_SCALE
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    cold = [_cloud(2 * i + 1, n).to(DEV) for i, n in enumerate([3000, 2500, 5000])]
    hot = [c.clone() for c in cold]
    for h in hot:
        h[:, 3] *= HOT
    chunk = [cold[0], hot[1], cold[2]]

    def drain():
        try:
            model.check_range(synchronize=True)
        except RuntimeError:
            pass
        model.check_range(synchronize=True)                            # cleared once reported

    # the first call after loading: the range-checked forward refuses
    seq = ModelInferenceHelper(model, is_sequential=True)
    with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
        seq.predict_sequence(chunk)
    drain()
    # in range: finite poses (and the checks pass)
    ok = ModelInferenceHelper(model, is_sequential=True).predict_sequence(cold)
    assert ok.shape[0] == 2 and bool(torch.isfinite(ok).all())
    # a later call: the overflow word, then finish() -- no pose is handed out
    seq = ModelInferenceHelper(model, is_sequential=True)
    with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
        seq.predict_sequence(chunk)
    drain()
    again = ModelInferenceHelper(model, is_sequential=True).predict_sequence(cold)
    torch.testing.assert_close(again, ok, rtol=0, atol=0)
