"""GPU parity, level 2: the fused forward path against the CPU oracle and the committed goldens.

Tolerances: indices/counts exact; activations rtol 1e-5 / atol 1e-6 x max|want| against fp32 CPU (SURVEY.md
section 8c; the matrix products accumulate in f32, only the summation order differs from the CPU GEMMs); pose
4x4 within 1e-4 absolute (BASELINE.json's stated tolerance). Measured on MI355X (profiles/r02_parity_errors.txt,
written by the `stage=` calls below): max |error| / scale <= 1.2e-6 and elementwise relative error <= 4.2e-5 on
every stage against the reference-generated goldens and the oracle."""
import os

import numpy as np
import pytest
import torch

import oracle
from oracle import labels as olabels
from deepclr_amd import lib, ops, synthetic
from deepclr_amd.config import model_config_from_dict
from deepclr_amd.labels import LabelType
from deepclr_amd.models import build_model, ModelInferenceHelper
from helpers import GOLDEN_CASES, load_golden, case_cfg, case_label_type, degenerate_batch, pose_delta, small_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RTOL, ATOL = 1e-5, 1e-6


def _models(cfg: dict, sd):
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=True)
    return model.to(DEV).eval(), oracle.build_oracle_model(cfg, sd)


def _mats(y, label_type=LabelType.POSE3D_DUAL_QUAT):
    y = y.detach().cpu().numpy() if torch.is_tensor(y) else np.asarray(y)
    return np.stack([label_type.to_matrix(v) for v in y.astype(np.float64)])


PARITY_LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out', 'parity_errors.txt')


def _close(got: torch.Tensor, want, rtol=RTOL, atol=ATOL, stage=None):
    """assert_close with the tolerances of the module header; with `stage` the measured error is also printed and
    appended to gpurun_out/parity_errors.txt (max |got - want|, the same relative to max |want|, and the largest
    elementwise relative error among elements above 1e-3 of the scale)."""
    want = torch.as_tensor(want)
    scale = max(1.0, float(want.abs().max()))
    if stage is not None:
        g, w = got.detach().cpu().double(), want.double()
        err = (g - w).abs()
        big = w.abs() > 1e-3 * scale
        rel = float((err[big] / w.abs()[big]).max()) if bool(big.any()) else 0.0
        line = '%-58s max abs %.3e  (/scale %.3e)  max rel %.3e  scale %.3g' % (stage, float(err.max()), float(err.max()) / scale, rel, scale)
        print(line)
        try:
            os.makedirs(os.path.dirname(PARITY_LOG), exist_ok=True)
            with open(PARITY_LOG, 'a') as fh:
                fh.write(line + '\n')
        except OSError:
            pass
    torch.testing.assert_close(got.detach().cpu(), want, rtol=rtol, atol=atol * scale)


@pytest.mark.parametrize('name', list(GOLDEN_CASES))
def test_model_matches_golden_and_oracle(name):
    g, cfg, sd = load_golden(name)
    model, orc = _models(cfg, sd)
    x = torch.from_numpy(g['x']).to(DEV)
    with torch.no_grad():
        feat = model.cloud_features(x.clone())
        emb = model._merge_layers[0](feat)
        y, loss, dbg = model(x.clone())
        y_feat, _, _ = model(feat, is_feat=True)
    assert loss is None and dbg is None
    # stage by stage against the reference-composition golden
    picks = torch.from_numpy(g['fps_idx'].astype(np.int64))
    if 'fps_idx1' in g.files:                     # second set-abstraction level: samples of the level-0 centroids
        picks = picks.gather(1, torch.from_numpy(g['fps_idx1'].astype(np.int64)))
    assert torch.equal(feat[:, :3, :].cpu(), torch.from_numpy(g['x'])[:, :, :3].gather(
        1, picks[:, :, None].expand(-1, -1, 3)).transpose(1, 2))
    if GOLDEN_CASES[name][1]:
        _close(feat, g['cloud_features'], stage=name + ': cloud_features vs reference golden')
        _close(emb, g['flow_embedding'], stage=name + ': flow_embedding vs reference golden')
    else:
        for key, t in (('cloud_features', feat), ('flow_embedding', emb)):
            assert tuple(t.shape) == tuple(g[key + '_shape'])
            got = t.contiguous().view(-1)[torch.from_numpy(g[key + '_pos']).to(DEV)]
            _close(got, g[key + '_val'], stage=name + ': ' + key + ' (sampled) vs reference golden')
    lt = case_label_type(name)
    assert tuple(y.shape) == tuple(g['y'].shape) == (x.shape[0] // 2, lt.dim)
    _close(y, g['y'], stage=name + ': y (B, label_dim) vs reference golden')
    _close(y_feat, g['y'], stage=name + ': y via is_feat=True vs reference golden')
    # the reference's 4x4 where the golden holds it; euler goldens hold none (its to_matrix needs a library absent where
    # the goldens are made): their reference labels go through deepclr_amd.labels like the outputs
    mat_g = g['mat'] if 'mat' in g.files else _mats(g['y'], lt)
    mat_err = float(np.abs(_mats(y, lt) - mat_g).max())
    _close(torch.from_numpy(_mats(y, lt)).float(), mat_g.astype(np.float32), rtol=0, atol=1e-4, stage=name + ': 4x4 pose vs reference golden')
    assert mat_err < 1e-4
    # and against the oracle recomputed on this host
    _close(y, orc(torch.from_numpy(g['x'])), stage=name + ': y vs oracle on this host')


@pytest.mark.parametrize('kind,n,pairs', [('kitti', 4096, 2), ('modelnet', 2048, 3)])
def test_fused_stages_against_oracle(kind, n, pairs):
    cfg = synthetic.model_cfg(kind)
    sd = synthetic.random_state_dict(cfg, seed=21)
    model, orc = _models(cfg, sd)
    x_cpu = torch.from_numpy(synthetic.make_batch(kind, pairs, n, first_pair=40))
    x = x_cpu.to(DEV)
    sa = cfg['params']['cloud_features']['params']
    npoint = sa['npoint'][0]

    # sampling + grouping indices: exact
    fps = ops.fps_clouds(x, npoint)
    xyz = x_cpu[:, :, :3].contiguous()
    fps_o = oracle.furthest_point_sample(xyz, npoint)
    assert torch.equal(fps.cpu(), fps_o)
    new_xyz = oracle.gather_operation(xyz.transpose(1, 2).contiguous(), fps_o).transpose(1, 2).contiguous()
    sam = model._cloud_layers[0]._sa0
    rows, counts = ops.sa_msg_fused(x, fps, sam.radii, sam.nsamples, sam.packed_mlps(), want_counts=True)
    for s, (r, ns) in enumerate(zip(sam.radii, sam.nsamples)):
        bq = oracle.ball_query(r, ns, xyz, new_xyz)
        # hits = 1 + number of later slots that are not padding (padding repeats the first hit;
        # every centroid is a cloud point, so it always hits itself)
        hits = 1 + (bq[:, :, 1:] != bq[:, :, :1]).sum(-1)
        assert torch.equal(counts[:, :, s].cpu(), hits.to(torch.int32)), 'scale %d' % s

    feat_o = orc.cloud_features(x_cpu)
    with torch.no_grad():
        feat = model.cloud_features(x.clone())
    _close(feat, feat_o, stage='%s n=%d: cloud_features vs oracle' % (kind, n))

    # kNN on the oracle's features (identical xyz) : exact neighbour lists
    f_rows = ops.channels_to_rows(feat_o.to(DEV).contiguous(), ops.F_STRIDE)
    k = cfg['params']['merge']['params']['k']
    knn_idx = ops.knn_rows(f_rows, pairs, npoint, k).cpu()
    _, _, gi = orc.knn_groups(feat_o[:pairs], feat_o[pairs:])
    local = (gi[1] - (torch.arange(pairs).repeat_interleave(npoint) * npoint).view(-1, 1)).view(pairs, npoint, k)
    assert torch.equal(knn_idx.long(), local)

    with torch.no_grad():
        emb = model._merge_layers[0](feat_o.to(DEV))
        emb_o = orc.flow_embedding(feat_o)
        _close(emb, emb_o, stage='%s n=%d: flow_embedding vs oracle (oracle features in)' % (kind, n))
        y = model._merge_layers[1](emb_o.to(DEV))
        _close(y, orc.pose_head(emb_o), stage='%s n=%d: pose head vs oracle (oracle embedding in)' % (kind, n))
        y_full, _, _ = model(x.clone())
    y_o = orc(x_cpu)
    _close(y_full, y_o, stage='%s n=%d: y end to end vs oracle' % (kind, n))
    mats_o = np.stack([olabels.dual_quat_to_matrix(v) for v in y_o.numpy()])
    assert pose_delta(_mats(y_full), mats_o) < 1e-4


@pytest.mark.parametrize('c,n,npoint,radii,nsamples', [
    (3, 2048, 100, (0.3, 0.6), (64, 128)),      # dense: every neighbourhood overflows its cap, drains mid-sweep
    (4, 1500, 37, (0.25, 5.0), (16, 700)),      # one scale sparse, one that swallows half the cloud; ragged tail
    (4, 777, 64, (0.05,), (8,)),                # single scale
    (4, 6000, 90, (0.4, 1.0), (24, 64)),        # groups of 128 points: two slices per group (slice boxes)
    (4, 16384, 128, (0.5, 1.0), (512, 1024)),   # groups of 256 points: four slices per group, the model's own shapes
    (3, 12000, 77, (0.2, 0.7), (16, 40)),       # four slices, ragged last group, 3 channels
])
def test_fused_set_abstraction_dense_neighbourhoods(c, n, npoint, radii, nsamples):
    _check_set_abstraction(c, n, npoint, radii, nsamples)


def _check_set_abstraction(c, n, npoint, radii, nsamples, expect_cap=True):
    from deepclr_amd.pointnet2 import PointnetSAModuleMSG
    rng = np.random.default_rng(n)
    pts = rng.normal(size=(2, n, 3))
    pts /= np.linalg.norm(pts, axis=2, keepdims=True)
    pts *= rng.uniform(0.2, 1.0, size=(2, n, 1))
    x_np = np.concatenate((pts, rng.uniform(size=(2, n, c - 3))), axis=2).astype(np.float32)
    torch.manual_seed(5)
    sam = PointnetSAModuleMSG(npoint=npoint, radii=list(radii), nsamples=list(nsamples),
                              mlps=[[c - 3, 16, 16, 32] for _ in radii], bn=False, use_xyz=True)
    for prm in sam.parameters():
        if prm.dim() == 1:
            torch.nn.init.uniform_(prm, -0.1, 0.1)
    x = torch.from_numpy(x_np)
    xyz = x[:, :, :3].contiguous()
    feats = x[:, :, 3:].transpose(1, 2).contiguous() if c > 3 else None
    weights = [[(u.conv.weight.detach(), u.conv.bias.detach()) for u in stack] for stack in sam.mlps]
    from oracle.model import sa_msg_forward
    new_xyz_o, feat_o = sa_msg_forward(xyz, feats, npoint, list(radii), list(nsamples), weights)
    sam = sam.to(DEV)
    with torch.no_grad():
        new_xyz, feat = sam(xyz.to(DEV), None if feats is None else feats.to(DEV))
    assert torch.equal(new_xyz.cpu(), new_xyz_o)
    _close(feat, feat_o)
    fps, gpts, gbox, sbox = ops.fps_clouds_grouped(x.to(DEV), npoint)
    assert torch.equal(fps, ops.fps_clouds(x.to(DEV), npoint)) and (gpts is not None) == (n > 1024)
    assert (sbox is not None) == (gpts is not None and ops.fps_group_layout(n)[1] > 64 and x.shape[0] % 2 == 0)
    rows_a, counts = ops.sa_msg_fused(x.to(DEV), fps, list(radii), list(nsamples), sam.packed_mlps(), want_counts=True)
    rows_f32, counts_f32 = ops.sa_msg_fused(x.to(DEV), fps, list(radii), list(nsamples), sam.packed_mlps(), want_counts=True,
                                            precision='f32')
    assert torch.equal(counts, counts_f32)
    _close(rows_a, rows_f32.cpu(), stage='set abstraction: split-f16 vs f32 shared MLP')
    if gpts is not None:                              # spatial-group fast path == exhaustive sweep, bit for bit
        rows_b, counts_b = ops.sa_msg_fused(x.to(DEV), fps, list(radii), list(nsamples), sam.packed_mlps(),
                                            want_counts=True, groups=(gpts, gbox))
        assert torch.equal(counts, counts_b)
        assert torch.equal(rows_a, rows_b)
        if sbox is not None:
            # slice level: the exported groups lie slice by slice (64 consecutive points of the sorted cloud each), the slice
            # boxes are their exact bounding boxes, and the slice-by-slice scan finds the same neighbours
            rows_c, counts_c = ops.sa_msg_fused(x.to(DEV), fps, list(radii), list(nsamples), sam.packed_mlps(),
                                                want_counts=True, groups=(gpts, gbox, sbox))
            assert torch.equal(counts, counts_c) and torch.equal(rows_a, rows_c)
            sl = gpts.view(x.shape[0], -1, 64, 4)
            live = sl[..., 3].contiguous().view(torch.int32) >= 0
            for a in range(3):
                lo = torch.where(live, sl[..., a], torch.full_like(sl[..., a], 3.0e38)).min(dim=2).values
                hi = torch.where(live, sl[..., a], torch.full_like(sl[..., a], -3.0e38)).max(dim=2).values
                assert torch.equal(sbox[..., a], lo) and torch.equal(sbox[..., 3 + a], hi)
        k = gpts[..., 3].contiguous().view(torch.int32)   # the groups are a permutation of the cloud
        for b_ in range(x.shape[0]):
            kk = k[b_][k[b_] >= 0].long()
            assert sorted(kk.tolist()) == list(range(n))
            assert torch.equal(gpts[b_][k[b_] >= 0][:, :3], x.to(DEV)[b_, kk, :3])
    for s, (r, ns) in enumerate(zip(radii, nsamples)):
        bq = oracle.ball_query(r, ns, xyz, new_xyz_o)
        hits = 1 + (bq[:, :, 1:] != bq[:, :, :1]).sum(-1)
        assert torch.equal(counts[:, :, s].cpu(), hits.to(torch.int32))
        assert not expect_cap or (hits == ns).any() or r < 0.1


@pytest.mark.parametrize('n, pairs, c', [(20000, 1, 4), (32768, 1, 4), (40000, 1, 4), (65536, 2, 4), (50000, 1, 3), (17000, 1, 3)])
def test_large_cloud_groups_from_the_workspace_sampler(n, pairs, c):
    """16384 < n <= 65536: the workspace sampler exports its 128 / 256 groups of 256 points and set abstraction takes
    the grouped fast path over them: same samples as the ungrouped call, groups = a permutation of the cloud with
    tight boxes, rows and counts bit-identical to the exhaustive sweep."""
    cfg = synthetic.model_cfg('kitti')
    sa = {k_: v[0] for k_, v in cfg['params']['cloud_features']['params'].items()}
    x = torch.from_numpy(synthetic.make_batch('kitti', pairs, n, first_pair=41)[:, :, :c].copy()).to(DEV)
    npoint = int(sa['npoint'])
    idx, gpts, gbox = ops.fps_clouds_grouped(x, npoint)[:3]
    assert gpts is not None and ops.fps_group_layout(n) == ((128 if n <= 32768 else 256), 256)
    assert torch.equal(idx, ops.fps_clouds(x, npoint))
    k = gpts[..., 3].contiguous().view(torch.int32)
    for b_ in range(x.shape[0]):
        real = k[b_] >= 0
        kk = k[b_][real].long()
        assert torch.equal(torch.sort(kk).values, torch.arange(n, device=DEV))
        assert torch.equal(gpts[b_][real][:, :3], x[b_, kk, :3])
        assert bool((gpts[b_][~real][:, :3] == 3.0e38).all())
        g = gpts[b_].view(-1, 256, 4)
        for a in range(3):
            col = g[:, :, a]
            live = k[b_].view(-1, 256) >= 0
            lo = torch.where(live, col, torch.full_like(col, 3.0e38)).min(dim=1).values
            hi = torch.where(live, col, torch.full_like(col, -3.0e38)).max(dim=1).values
            has = live.any(dim=1)
            assert torch.equal(gbox[b_, :, a][has], lo[has]) and torch.equal(gbox[b_, :, 3 + a][has], hi[has])
    from deepclr_amd.pointnet2 import PointnetSAModuleMSG
    torch.manual_seed(9)
    sam = PointnetSAModuleMSG(npoint=npoint, radii=list(sa['radii']), nsamples=list(sa['nsamples']),
                              mlps=[[c - 3, 16, 16, 32] for _ in sa['radii']], bn=False, use_xyz=True).to(DEV)
    rows_a, counts_a = ops.sa_msg_fused(x, idx, list(sa['radii']), list(sa['nsamples']), sam.packed_mlps(), want_counts=True)
    rows_b, counts_b = ops.sa_msg_fused(x, idx, list(sa['radii']), list(sa['nsamples']), sam.packed_mlps(),
                                        want_counts=True, groups=(gpts, gbox))
    assert torch.equal(counts_a, counts_b) and torch.equal(rows_a, rows_b)
    assert int(counts_a.max()) > 1


@pytest.mark.parametrize('feat, n, npoint, radii, nsamples, mlps', [
    (64, 1024, 128, (0.3, 0.6), (16, 32), ([64, 64, 128], [64, 96, 128])),       # a PointNet++-style second level
    (64, 300, 48, (0.25,), (24,), ([64, 32, 32],)),
    (5, 2000, 100, (0.2, 0.4, 0.8), (8, 64, 100), ([5, 16], [5, 24, 24], [5, 8, 8, 40])),   # three scales, ragged depths
    (0, 777, 33, (0.3,), (20,), ([0, 16, 16, 48],)),                             # xyz only, widths the fused kernel lacks
])
def test_composed_set_abstraction_against_oracle(feat, n, npoint, radii, nsamples, mlps):
    """Shapes outside the fused kernel (feature inputs, other widths, three scales) run composed from the level-1 HIP
    operators + dclr_linear with the max folded in (deepclr_amd/pointnet2.py): centroids exact, features within the
    activation tolerance of the oracle's restatement of the same module."""
    from deepclr_amd.pointnet2 import PointnetSAModuleMSG
    from oracle.model import sa_msg_forward
    rng = np.random.default_rng(n + feat)
    pts = rng.normal(size=(2, n, 3))
    pts /= np.linalg.norm(pts, axis=2, keepdims=True)
    pts *= rng.uniform(0.2, 1.0, size=(2, n, 1))
    xyz = torch.from_numpy(pts.astype(np.float32))
    feats = torch.from_numpy(rng.normal(size=(2, feat, n)).astype(np.float32)) if feat else None
    torch.manual_seed(3)
    sam = PointnetSAModuleMSG(npoint=npoint, radii=list(radii), nsamples=list(nsamples), mlps=[list(m) for m in mlps],
                              bn=False, use_xyz=True)
    assert not sam.fused
    for prm in sam.parameters():
        if prm.dim() == 1:
            torch.nn.init.uniform_(prm, -0.1, 0.1)
    weights = [[(u.conv.weight.detach(), u.conv.bias.detach()) for u in stack] for stack in sam.mlps]
    new_xyz_o, feat_o = sa_msg_forward(xyz, feats, npoint, list(radii), list(nsamples), weights)
    sam = sam.to(DEV)
    with torch.no_grad():
        new_xyz, out = sam(xyz.to(DEV), None if feats is None else feats.to(DEV))
    assert torch.equal(new_xyz.cpu(), new_xyz_o)
    assert tuple(out.shape) == (2, sum(m[-1] for m in mlps), npoint)
    _close(out, feat_o, stage='composed set abstraction (%d feature channels, %d scales) vs oracle' % (feat, len(radii)))


def test_radius_mask_is_exercised():
    """ModelNet arch: flow-embedding radius 0.2 with k = 30 of 512 points masks many neighbours."""
    cfg = synthetic.model_cfg('modelnet')
    sd = synthetic.random_state_dict(cfg, seed=3)
    model, orc = _models(cfg, sd)
    x_cpu = torch.from_numpy(synthetic.make_batch('modelnet', 1, 1024, first_pair=7))
    feat_o = orc.cloud_features(x_cpu)
    pts0, pts1, gi = orc.knn_groups(feat_o[:1], feat_o[1:])
    d = (pts1[gi[1]][:, :, :3] - pts0[gi[0]][:, :, :3]).norm(dim=2)
    frac = (d >= 0.2).float().mean().item()
    assert 0.05 < frac < 0.95, frac
    with torch.no_grad():
        _close(model._merge_layers[0](feat_o.to(DEV)), orc.flow_embedding(feat_o))


def test_degenerate_inputs():
    """Duplicates (exact ties everywhere) and npoint > N (reference test's 96-point clouds)."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=8)
    model, orc = _models(cfg, sd)
    x_cpu = torch.from_numpy(degenerate_batch(2, 96, 4, 77))
    with torch.no_grad():
        y, _, _ = model(x_cpu.to(DEV))
    _close(y, orc(x_cpu))


def test_reference_layer_shapes():
    """Shapes asserted by /root/reference/tests/model/test_deepclr.py:19-57 (5 pairs x 96 points)."""
    from deepclr_amd.models.deepclr import SetAbstraction, MotionEmbedding, OutputSimple
    cfg = model_config_from_dict(synthetic.model_cfg('kitti'))
    clouds_internal = torch.rand(10, cfg.input_dim, 96, device=DEV)
    sa = SetAbstraction(input_dim=cfg.input_dim, point_dim=cfg.point_dim, **cfg.params.cloud_features.params).to(DEV)
    f = sa(clouds_internal)
    assert f.shape == (10, 67, 1024)
    me = MotionEmbedding(input_dim=sa.output_dim(), point_dim=cfg.point_dim, **cfg.params.merge.params).to(DEV)
    e = me(f)
    assert e.shape == (5, 259, 1024)
    head = OutputSimple(input_dim=me.output_dim(), label_type=cfg.label_type, **cfg.params.output.params).to(DEV)
    assert head(e).shape == (5, cfg.label_type.dim)
    model = build_model(cfg).to(DEV)
    clouds = torch.rand(10, 96, cfg.input_dim, device=DEV)
    with torch.no_grad():
        y1, _, _ = model(clouds)
        y2, _, _ = model(model.cloud_features(clouds), is_feat=True)
    assert y1.shape == y2.shape == (5, 8)
    assert torch.equal(y1, y2)


def test_inference_helper_pairwise_and_sequential():
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=4)
    model, orc = _models(cfg, sd)
    frames = [torch.from_numpy(synthetic.kitti_like_pair(i, 2048)[0]) for i in range(3)]
    pair = ModelInferenceHelper(model, is_sequential=False)
    seq = ModelInferenceHelper(model, is_sequential=True)
    assert seq.predict(frames[0].to(DEV)) is None and seq.has_state()
    for a, b in ((0, 1), (1, 2)):
        want = orc(torch.stack((frames[a], frames[b])))[0]
        _close(pair.predict(frames[b].to(DEV), frames[a].to(DEV)), want)
        _close(seq.predict(frames[b].to(DEV)), want)
    seq.reset_state()
    assert not seq.has_state()
    with pytest.raises(RuntimeError):
        pair.predict(frames[0].to(DEV))
    with pytest.raises(RuntimeError):
        pair.predict(frames[0][:, :3].to(DEV), frames[1].to(DEV))
    with pytest.warns(UserWarning):
        wide = torch.cat((frames[0], frames[0][:, :1]), dim=1).to(DEV)
        pair.predict(wide, frames[1].to(DEV))
    batch = pair.predict_batch(torch.stack(frames[1:]).to(DEV), torch.stack(frames[:2]).to(DEV))
    _close(batch[1], orc(torch.stack((frames[1], frames[2])))[0])


def test_linear_kernel_against_torch():
    rng = np.random.default_rng(0)
    for m, n, k in ((64, 32, 8), (128, 100, 259), (256, 256, 512), (192, 1024, 64)):
        kp = (k + 7) // 8 * 8
        x = torch.zeros(m, kp + 4)
        x[:, :k] = torch.from_numpy(rng.normal(size=(m, k)).astype(np.float32))
        w = torch.from_numpy(rng.normal(size=(n, k)).astype(np.float32)) / np.sqrt(k)
        b = torch.from_numpy(rng.normal(size=(n,)).astype(np.float32))
        wp = ops.pack_weight(w.to(DEV), kp)
        want = torch.relu(x[:, :k].double() @ w.double().T + b.double()).float()
        _close(ops.linear(x.to(DEV), wp, b.to(DEV), n, kp, relu=True), want)
        groups = m // 64
        _close(ops.linear(x.to(DEV), wp, b.to(DEV), n, kp, relu=True, colmax_groups=groups),
               want.view(groups, 64, n).max(dim=1).values)
        raw = (x[:, :k].double() @ w.double().T).float()
        _close(ops.linear(x.to(DEV), wp, None, n, kp, relu=False), raw)


def test_fused_head_chain_equals_layer_by_layer_kernels(monkeypatch):
    """Batches of >= 4 pairs run the five head layers in one launch, smaller ones layer by layer. On the f32 matrix
    instructions both use the same k order: identical results. The split-fp16 chain (default) must agree with the
    float64 product at least as well as those do."""
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=7))
    head = model._merge_layers[1]
    layers = head._packed()
    rows, pairs = 4096, 4
    e = torch.zeros(rows, ops.E_STRIDE, device=DEV)
    e[:, :259] = torch.from_numpy(np.random.default_rng(3).normal(size=(rows, 259)).astype(np.float32)).to(DEV)
    saved, ops.PRECISION = ops.PRECISION, 'f32'
    try:
        assert head._fusable(layers, rows, pairs) and not head._fusable(layers, rows // 2, pairs // 2)
    finally:
        ops.PRECISION = saved
    fused = ops.head_conv_fused(e, layers, pairs)
    split = ops.head_conv_fused_f16(e, ops.E_STRIDE, head._packed_f16(), pairs)   # f16 hi/lo operands, f32-accurate
    h = e
    for wp, b, n, kp in layers[:-1]:
        h = ops.linear(h, wp, b, n, kp, relu=True, ldy=(n + 7) // 8 * 8)
    wp, b, n, kp = layers[-1]
    plain = ops.linear(h, wp, b, n, kp, relu=True, colmax_groups=pairs)
    assert torch.equal(fused, plain)
    want = e[:, :259].double().cpu()
    want = torch.cat((want[:, 256:259], want[:, :256]), dim=1)                 # reference column order [xyz | feat]
    for w, bias in head.conv.affine_params():
        want = torch.relu(want @ w.detach().double().cpu().reshape(w.shape[0], -1).t() + bias.detach().double().cpu())
    want = want.view(pairs, rows // pairs, -1).max(dim=1).values
    _close(fused, want.float())
    _close(split, want.float())
    err32, err16 = (fused.double().cpu() - want).abs().max().item(), (split.double().cpu() - want).abs().max().item()
    assert err16 <= 2 * err32 + 1e-7, (err16, err32)        # no less accurate than the f32 matrix instructions
    print('head chain max abs error vs float64: f32 MFMA %.3g, split-f16 %.3g' % (err32, err16))
    # every group size and row count the model can hand it: per-pair groups of 64 .. 1024 rows
    for rows2, pairs2 in ((64, 1), (128, 2), (1024, 1), (1536, 3), (8192, 8)):
        e2 = e[:rows2].contiguous() if rows2 <= rows else torch.cat((e, e.flip(0)))[:rows2].contiguous()
        a = ops.head_conv_fused_f16(e2, ops.E_STRIDE, head._packed_f16(), pairs2)
        assert torch.equal(a, ops.head_conv_fused_f16(e2, ops.E_STRIDE, head._packed_f16(), pairs2))     # deterministic
        want2 = e2[:, :259].double().cpu()
        want2 = torch.cat((want2[:, 256:259], want2[:, :256]), dim=1)
        for w, bias in head.conv.affine_params():
            want2 = torch.relu(want2 @ w.detach().double().cpu().reshape(w.shape[0], -1).t() + bias.detach().double().cpu())
        _close(a, want2.view(pairs2, rows2 // pairs2, -1).max(dim=1).values.float())


def test_full_size_kitti_batch_properties_and_oracle_pair():
    """BASELINE.json config 2 (B=8, N=16384): properties on the whole batch, oracle parity on pair 0."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=0)
    model, orc = _models(cfg, sd)
    x_np = synthetic.make_batch('kitti', 8, 16384)
    x = torch.from_numpy(x_np).to(DEV)
    fps = ops.fps_clouds(x, 1024).long()
    assert (fps[:, 0] == 0).all()
    assert all(len(set(row.tolist())) == 1024 for row in fps.cpu())           # no point sampled twice
    # greedy invariant: the distance of each new sample to the already chosen set never increases
    pts = torch.gather(x[:, :, :3], 1, fps[:, :, None].expand(-1, -1, 3)).double()
    d = torch.cdist(pts, pts)
    mask = torch.tril(torch.ones(1024, 1024, dtype=torch.bool, device=DEV), diagonal=-1)
    reach = torch.where(mask, d, torch.full_like(d, float('inf'))).min(dim=2).values[:, 1:]
    assert (reach[:, 1:] <= reach[:, :-1] + 1e-9).all()
    with torch.no_grad():
        y, _, _ = model(x.clone())
        y_half, _, _ = model(x[[0, 1, 2, 3, 8, 9, 10, 11]].clone())
        y_single, _, _ = model(x[[0, 8]].clone())
    assert torch.equal(y[:4], y_half) and torch.equal(y[:1], y_single)        # pairs are independent
    y_o = orc(torch.from_numpy(x_np[[0, 8]]))
    _close(y[:1], y_o)
    assert pose_delta(_mats(y[:1]), np.stack([olabels.dual_quat_to_matrix(v) for v in y_o.numpy()])) < 1e-4


@pytest.mark.parametrize('kind,n,pairs', [('modelnet', 2048, 6), ('kitti', 65536, 1)])
def test_other_baseline_configs_against_oracle(kind, n, pairs):
    """BASELINE.json configs 4 (ModelNet40, 2048 pts, many pairs per batch) and 5 (dense 65536-pt clouds) at a
    batch size the oracle finishes in seconds; the full-size runs differ only in the batch count (pairs are
    independent, checked in test_full_size_kitti_batch_properties_and_oracle_pair)."""
    cfg = synthetic.model_cfg(kind)
    sd = synthetic.random_state_dict(cfg, seed=31)
    model, orc = _models(cfg, sd)
    x_cpu = torch.from_numpy(synthetic.make_batch(kind, pairs, n, first_pair=100))
    with torch.no_grad():
        y, _, _ = model(x_cpu.to(DEV))
    y_o = orc(x_cpu)
    _close(y, y_o)
    mats_o = np.stack([olabels.dual_quat_to_matrix(v) for v in y_o.numpy()])
    assert pose_delta(_mats(y), mats_o) < 1e-4


@pytest.mark.parametrize('kind,n,pairs,npoint', [('modelnet', 2048, 256, 512), ('kitti', 65536, 4, 1024)])
def test_full_size_c4_c5_batches_properties_and_oracle_pairs(kind, n, pairs, npoint):
    """BASELINE.json configs[3] (C4: 256 ModelNet pairs of 2 x 2048 points = 512 clouds per batch, k = 30) and
    configs[4] (C5: 4 pairs of 2 x 65536 points, paged sampler + exhaustive set-abstraction sweep) AT FULL SIZE:
    whole-batch properties (no point sampled twice, greedy invariant, pairs independent of the batch they travel
    in -- bit-identical against sub-batches) and oracle parity on two pairs."""
    cfg = synthetic.model_cfg(kind)
    sd = synthetic.random_state_dict(cfg, seed=5)
    model, orc = _models(cfg, sd)
    x_np = synthetic.make_batch(kind, pairs, n, first_pair=300)
    x = torch.from_numpy(x_np).to(DEV)
    assert tuple(x.shape) == (2 * pairs, n, cfg['input_dim'])
    fps = ops.fps_clouds(x, npoint).long()
    assert (fps[:, 0] == 0).all() and int(fps.min()) >= 0 and int(fps.max()) < n
    srt = fps.sort(dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())                            # no point sampled twice
    sel = list(range(0, 2 * pairs, max(1, 2 * pairs // 16)))                  # greedy invariant on a spread of clouds
    pts = torch.gather(x[sel, :, :3], 1, fps[sel][:, :, None].expand(-1, -1, 3)).double()
    d = torch.cdist(pts, pts)
    mask = torch.tril(torch.ones(npoint, npoint, dtype=torch.bool, device=DEV), diagonal=-1)
    reach = torch.where(mask, d, torch.full_like(d, float('inf'))).min(dim=2).values[:, 1:]
    assert (reach[:, 1:] <= reach[:, :-1] + 1e-9).all()
    half = pairs // 2
    sub = list(range(half)) + list(range(pairs, pairs + half))
    with torch.no_grad():
        y, _, _ = model(x.clone())
        y_half, _, _ = model(x[sub].clone())
        y_two, _, _ = model(x[[0, 1, pairs, pairs + 1]].clone())
    assert tuple(y.shape) == (pairs, 8) and bool(torch.isfinite(y).all())
    assert torch.equal(y[:half], y_half) and torch.equal(y[:2], y_two)        # pairs are independent
    y_o = orc(torch.from_numpy(x_np[[0, 1, pairs, pairs + 1]]))
    _close(y[:2], y_o)
    assert pose_delta(_mats(y[:2]), np.stack([olabels.dual_quat_to_matrix(v) for v in y_o.numpy()])) < 1e-4
    # through the pipelined runner (what bench.py --config c4 / c5 times): identical outputs
    from deepclr_amd.pipeline import PipelinedForward
    runner = PipelinedForward(model, depth=2, ahead='knn', group=1 if kind == 'modelnet' else 2)
    got = list(runner.run([x, x, x]))
    assert all(torch.equal(g, y) for g in got)


def test_pipelined_runner_cold_start_on_side_streams():
    """A freshly built model whose very first use is the pipelined runner: the weight-packing kernels are enqueued
    by whichever stream asks first, every other stream must be ordered behind them (PackedCache events)."""
    from deepclr_amd.pipeline import PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=12)
    batches = [torch.from_numpy(synthetic.make_batch('kitti', 2, 4096, first_pair=20 + 3 * i)).to(DEV) for i in range(6)]
    for trial in range(3):
        fresh = build_model(model_config_from_dict(cfg))
        fresh.load_state_dict(sd, strict=True)
        fresh = fresh.to(DEV).eval()
        got = list(PipelinedForward(fresh, depth=3, ahead='knn', group=2).run(batches))
        if trial == 0:
            with torch.no_grad():
                want = [fresh(b)[0] for b in batches]
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    # parameters replaced AFTER the runner was built: the rebuild happens on a side stream
    fresh = build_model(model_config_from_dict(cfg)).to(DEV).eval()
    runner = PipelinedForward(fresh, depth=3, ahead='knn', group=2)
    fresh.load_state_dict(sd, strict=True)
    got = list(runner.run(batches))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_pipelined_runner_matches_plain_forward():
    from deepclr_amd.pipeline import PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=2))
    batches = [torch.from_numpy(synthetic.make_batch('kitti', 2, 4096, first_pair=10 * i)).to(DEV) for i in range(5)]
    with torch.no_grad():
        want = [model(b)[0] for b in batches]
    for ahead, group, dense in (('sample', 1, False), ('features', 1, False), ('features', 2, False), ('features', 3, False),
                                ('knn', 1, False), ('knn', 2, False), ('knn', 2, True), ('knn', 3, True), ('knn', 4, True)):
        got = list(PipelinedForward(model, depth=2, ahead=ahead, group=group, dense_group=dense).run(batches))
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    # single-batch dense launches alternating over several dense streams (bench.py --strict): same results, in step order on
    # the caller's stream, also when they are written into a caller's buffer
    for ahead, streams in (('knn', 2), ('knn', 3), ('features', 2)):
        runner = PipelinedForward(model, depth=4, ahead=ahead, dense_streams=streams, inputs_ready=True)
        got = list(runner.run(batches + batches))
        assert len(got) == 2 * len(want) and all(torch.equal(a, b) for a, b in zip(got, want + want))
        slots = torch.zeros(len(batches), want[0].shape[0], want[0].shape[1], device=DEV)
        for i, b in enumerate(batches):
            runner.step(b, batches[i + 1:], out=slots[i])
        assert torch.equal(slots, torch.stack(want))
    with pytest.raises(ValueError):
        PipelinedForward(model, depth=2, ahead='knn', group=2, dense_group=True, dense_streams=2)
    # dense groups writing straight into a caller's buffer: whole groups at their first step, singles otherwise
    runner = PipelinedForward(model, depth=2, ahead='knn', group=2, dense_group=True)
    slots = torch.zeros(len(batches), want[0].shape[0], want[0].shape[1], device=DEV)
    i = 0
    while i < len(batches):
        span = runner.group_start(batches[i])
        if span > 1:
            y = runner.step(batches[i], batches[i + 1:], out=slots[i:i + span].view(-1, slots.shape[-1]))
            assert y.data_ptr() == slots[i].data_ptr()
            for j in range(1, span):
                assert runner.group_start(batches[i + j]) == 0
                y = runner.step(batches[i + j], batches[i + j + 1:])
                assert y.data_ptr() == slots[i + j].data_ptr()
            i += span
        else:
            runner.step(batches[i], batches[i + 1:], out=slots[i])
            i += 1
    assert torch.equal(slots, torch.stack(want))
    # results written straight into a caller's buffer (what bench.py hands to the all-gather)
    runner = PipelinedForward(model, depth=2, ahead='knn', group=2)
    slots = torch.zeros(len(batches), want[0].shape[0], want[0].shape[1], device=DEV)
    for i, b in enumerate(batches):
        y = runner.step(b, batches[i + 1:], out=slots[i])
        assert y.data_ptr() == slots[i].data_ptr()
    assert torch.equal(slots, torch.stack(want))
    with pytest.raises(RuntimeError):
        model.merge_rows(model.cloud_feature_rows(batches[0]), batches[0].shape[0] // 2,
                         out=torch.zeros(3, 8, device=DEV))


def test_pipelined_runner_with_inputs_ready_and_buffer_ring_reuse():
    """inputs_ready=True (what bench.py times): sampling launches do not wait for the caller's stream, so the prep ring
    (3 slots per plan and stream) is ordered by its release events alone. Twelve distinct batches = at least five launches
    per stream and plan, with and without dense groups: every slot is reused, results must equal the plain forward."""
    from deepclr_amd.pipeline import PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=21))
    batches = [torch.from_numpy(synthetic.make_batch('kitti', 2, 2048, first_pair=7 * i)).to(DEV) for i in range(12)]
    with torch.no_grad():
        want = [model(b)[0] for b in batches]
    torch.cuda.synchronize()
    for depth, group, dense in ((1, 1, False), (2, 1, False), (1, 2, True), (2, 2, True), (3, 2, False)):
        runner = PipelinedForward(model, depth=depth, ahead='knn', group=group, dense_group=dense, inputs_ready=True)
        assert not runner._eager                             # the default: a group's dense stages at its first step
        got = list(runner.run(batches))
        assert len(got) == len(want)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (depth, group, dense, i)
    # round 6: the dense stages of a group enqueued right behind its sampling launch (eager_dense, an option: measured
    # slower in a short window) or at the group's first step (the default): the same outputs, also into a caller's buffer
    with pytest.raises(ValueError):
        PipelinedForward(model, depth=2, ahead='knn', group=2, dense_group=True, inputs_ready=False, eager_dense=True)
    for eager in (True, False):
        runner = PipelinedForward(model, depth=2, ahead='knn', group=3, dense_group=True, inputs_ready=True, eager_dense=eager)
        assert runner._eager == eager
        outs = torch.zeros(len(batches), 2, want[0].shape[1], device=DEV)
        for i in range(min(len(batches), runner.depth * runner.group)):
            runner.prefetch(batches[i], flush=False)
        for i, b in enumerate(batches):
            n_out = runner.group_start(b)
            buf = outs[i:i + n_out].view(-1, outs.shape[-1]) if n_out else None
            y = runner.step(b, upcoming=batches[i + 1:], out=buf)
            assert torch.equal(y, want[i]), (eager, i)
            if n_out:
                torch.cuda.synchronize()
                assert torch.equal(outs[i:i + n_out].view(-1, outs.shape[-1]), torch.cat(want[i:i + n_out])), (eager, i)


@pytest.mark.parametrize('kind, pairs, n', [('kitti', 2, 2048), ('modelnet', 3, 2048), ('kitti', 1, 16384), ('kitti', 1, 20000)])
def test_batches_read_in_place_equal_the_concatenated_launch(kind, pairs, n):
    """dclr_fps_clouds_grouped_batched / dclr_sa_msg_fused_batched: the batches of one launch at a constant stride (views of
    one chunk; the same tensor again and again) are read where they lie. Sampling indices, groups and feature rows must be
    those of the launch over the concatenated clouds [templates of every batch | sources of every batch]; batches without
    a constant stride are not a view."""
    cfg = synthetic.model_cfg(kind)
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=31))
    g = 3
    chunk = torch.stack([torch.from_numpy(synthetic.make_batch(kind, pairs, n, first_pair=4 * i)) for i in range(g)]).to(DEV)
    for batches in ([chunk[i] for i in range(g)], [chunk[1]] * g):
        view = ops.batch_view(batches)
        assert view == (pairs, g, chunk[0].numel() if batches[0] is not batches[1] else 0)
        big = torch.cat([b[:pairs] for b in batches] + [b[pairs:] for b in batches])
        with torch.no_grad():
            want_s = model.sample(big)
            want = model.cloud_feature_rows(big, want_s)
            got_s = model.sample(batches[0], view)
            got = model.cloud_feature_rows(batches[0], got_s, view)
            alone = model.cloud_feature_rows(batches[0], None, view)           # sampling inside
        # (the exported groups themselves are not compared: points of one sorting cell land in scatter order)
        assert torch.equal(got_s[0], want_s[0]) and got_s[1].shape == want_s[1].shape and got_s[2].shape == want_s[2].shape
        assert torch.equal(got, want) and torch.equal(alone, want)
    assert ops.batch_view([chunk[0], chunk[2], chunk[1]]) is None               # no constant stride
    assert ops.batch_view([chunk[0]]) is None and ops.batch_view([chunk[0][:, ::2], chunk[1][:, ::2]]) is None   # not contiguous


def test_dense_groups_of_the_runner_read_their_batches_in_place(monkeypatch):
    """PipelinedForward with dense groups: batches that are views of one chunk go through the in-place launch (no torch.cat
    of clouds on the way), batches allocated one by one through the concatenating launch; both equal the plain forward."""
    from deepclr_amd.pipeline import PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=32))
    chunk = torch.stack([torch.from_numpy(synthetic.make_batch('kitti', 2, 2048, first_pair=3 * i)) for i in range(8)]).to(DEV)
    views = [chunk[i] for i in range(8)]
    clones = {i: views[i].clone() for i in (3, 0, 2, 1, 7, 4, 6, 5)}           # allocated out of order: no constant stride
    separate = [clones[i] for i in range(8)]
    assert ops.batch_view(separate[:4]) is None and ops.batch_view(separate[4:]) is None
    with torch.no_grad():
        want = [model(b)[0] for b in separate]
    cats = []
    real_cat = torch.cat
    monkeypatch.setattr(torch, 'cat', lambda ts, *a, **k: cats.append(len(ts)) or real_cat(ts, *a, **k))
    for batches, expect_cat in ((views, False), (separate, True)):
        cats.clear()
        runner = PipelinedForward(model, depth=2, ahead='knn', group=4, dense_group=True, inputs_ready=True)
        got = list(runner.run(batches))
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (expect_cat, i)
        assert (8 in cats) == expect_cat, cats                                   # 4 template halves + 4 source halves


def test_pipelined_run_prefetches_every_batch_after_the_first(monkeypatch):
    """run() must hand every batch but the first to a side stream (the slice of upcoming batches skipped one
    per window, which was then sampled synchronously on the main stream)."""
    from deepclr_amd.pipeline import PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=22))
    batches = [torch.from_numpy(synthetic.make_batch('kitti', 1, 2048, first_pair=3 * i)).to(DEV) for i in range(10)]
    main = torch.cuda.current_stream().cuda_stream
    on_main = []
    real = type(model).cloud_feature_rows
    monkeypatch.setattr(type(model), 'cloud_feature_rows',
                        lambda self, x, sample=None, view=None: on_main.append(torch.cuda.current_stream().cuda_stream == main)
                        or real(self, x, sample, view))
    for depth, group, dense in ((2, 1, False), (3, 1, False), (2, 2, False), (2, 2, True)):
        on_main.clear()
        runner = PipelinedForward(model, depth=depth, ahead='knn', group=group, dense_group=dense)
        assert len(list(runner.run(batches))) == len(batches)
        assert not any(on_main), (depth, group, dense, on_main)          # every set-abstraction pass ran on a side stream


def test_host_batch_feeder_matches_resident_batches():
    """--h2d path of bench.py: batches in pinned host memory, copied chunk by chunk on a copy stream into a ring of device
    buffers that is shorter than the stream of batches (every slot rewritten several times while older batches are still in
    flight); ragged last chunk."""
    from deepclr_amd.pipeline import HostBatchFeeder, PipelinedForward
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=23))
    host = [torch.from_numpy(synthetic.make_batch('kitti', 2, 2048, first_pair=5 * i)) for i in range(14)]
    with torch.no_grad():
        want = [model(h.to(DEV))[0] for h in host]
    torch.cuda.synchronize()
    for depth, group, dense, chunk in ((2, 1, False, 1), (2, 2, True, 2), (1, 3, True, 4), (2, 2, False, 3)):
        runner = PipelinedForward(model, depth=depth, ahead='knn', group=group, dense_group=dense, inputs_ready=True)
        feeder = HostBatchFeeder(runner, host[0].to(DEV), chunk=chunk)
        chunks = [torch.stack(host[i:i + chunk]).pin_memory() for i in range(0, len(host), chunk)]
        got, fed = [], 0
        while len(got) < len(host):
            while fed < len(chunks) and feeder.room() and feeder.pending() <= depth * group:
                feeder.feed(chunks[fed])
                fed += 1
            got.append(feeder.step().clone())
        assert feeder.bytes_copied == len(host) * host[0].numel() * 4 and feeder.pending() == 0
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (depth, group, dense, chunk, i)
    with pytest.raises(RuntimeError):
        feeder.feed(torch.zeros(1, 4, 100, 4).pin_memory())            # wrong batch shape


@pytest.mark.parametrize('n, expect_capped', [(16384, False), (65536, True)])
def test_ring_scan_clouds_crowded_neighbourhoods_match_the_oracle(n, expect_capped):
    """LiDAR-density clouds (deepclr_amd/synthetic.py:ring_scan, bench.py --clouds ring): near the sensor a 1 m ball holds
    hundreds of points at 16384 points per scan (more than the 512-entry staging ring: the centroid is redone with
    mid-centroid drains) and more than nsample = 1024 at 65536 (the radix select on the point index decides which
    neighbours count). Sampling and counts exact, features and poses against the oracle."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=4)
    model, orc = _models(cfg, sd)
    x_np = synthetic.make_batch('ring', 1, n, first_pair=2)
    x = torch.from_numpy(x_np).to(DEV)
    sa = model._cloud_layers[0]._sa0
    fps, gpts, gbox = ops.fps_clouds_grouped(x, 1024)[:3]
    xyz = torch.from_numpy(x_np[:, :, :3]).contiguous()
    fps_o = oracle.furthest_point_sample(xyz, 1024)
    assert torch.equal(fps.cpu(), fps_o)
    rows, counts = ops.sa_msg_fused(x, fps, sa.radii, sa.nsamples, sa.packed_mlps(), want_counts=True, groups=(gpts, gbox))
    rows32, counts32 = ops.sa_msg_fused(x, fps, sa.radii, sa.nsamples, sa.packed_mlps(), want_counts=True,
                                        groups=(gpts, gbox), precision='f32')
    assert torch.equal(counts, counts32)
    _close(rows, rows32.cpu(), stage='ring clouds: split-f16 vs f32 set-abstraction MLP')
    rows_sweep, counts_sweep = ops.sa_msg_fused(x, fps, sa.radii, sa.nsamples, sa.packed_mlps(), want_counts=True)
    assert torch.equal(counts, counts_sweep) and torch.equal(rows, rows_sweep)      # groups + radix select == in-order sweep
    new_xyz = torch.gather(xyz, 1, fps_o.long()[:, :, None].expand(-1, -1, 3))
    capped, crowded = 0, 0
    for s, (r, ns) in enumerate(zip(sa.radii, sa.nsamples)):
        bq = oracle.ball_query(r, ns, xyz, new_xyz)
        hits = 1 + (bq[:, :, 1:] != bq[:, :, :1]).sum(-1)
        assert torch.equal(counts[:, :, s].cpu(), hits.to(torch.int32))
        capped += int((hits == ns).sum())
        crowded += int((hits > 450).sum())
    print('ring clouds n=%d: %d (centroid, scale) neighbourhoods at their nsample cap, %d above the staging ring; mean hits '
          '%.1f / %.1f' % (n, capped, crowded, float(counts[:, :, 0].float().mean()), float(counts[:, :, 1].float().mean())))
    assert crowded > 0 and (capped > 0 or not expect_capped)
    with torch.no_grad():
        feat = model.cloud_features(x.clone())
        y, _, _ = model(x.clone())
    _close(feat, orc.cloud_features(torch.from_numpy(x_np)), stage='ring clouds: cloud_features vs oracle')
    y_o = orc(torch.from_numpy(x_np))
    assert np.abs(_mats(y) - _mats(y_o)).max() < 1e-4


def test_sequence_mode_computes_each_frame_once_and_matches_pairwise_calls():
    """Reference sequential mode (models/base.py:97-112): frame t is the source of pair (t-1, t) and the template
    of pair (t, t+1). The chunked runner must return exactly what per-frame predict() calls return."""
    from deepclr_amd.models import ModelInferenceHelper
    from deepclr_amd.pipeline import PipelinedSequence
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=4)
    model, orc = _models(cfg, sd)
    clouds = synthetic.make_batch('kitti', 3, 4096, first_pair=50)             # 6 clouds, used as 6 "frames"
    frames = torch.from_numpy(np.ascontiguousarray(clouds[[0, 3, 1, 4, 2, 5]])).to(DEV)
    one = ModelInferenceHelper(model, is_sequential=True)
    assert one.predict(frames[0]) is None
    want = torch.stack([one.predict(frames[i]) for i in range(1, 6)])
    chunked = ModelInferenceHelper(model, is_sequential=True)
    got = torch.cat((chunked.predict_sequence(frames[:2]), chunked.predict_sequence(frames[2:])))
    assert torch.equal(got, want)
    assert torch.equal(chunked.predict(frames[0]), one.predict(frames[0]))      # the cached frame carries on
    piped = torch.cat(list(PipelinedSequence(model, depth=2).run([frames[:1], frames[1:4], frames[4:]])))
    assert torch.equal(piped, want)
    # round 6: the chunks sampled by one launch share one dense launch (dense_group): the same poses, whatever the chunking,
    # also across a group border (the carried frame) and for a stream that ends inside a group
    for group, chunks in ((2, [frames[:1], frames[1:4], frames[4:]]), (3, [frames[:2], frames[2:4], frames[4:5], frames[5:]]),
                          (2, [frames[i:i + 1] for i in range(6)]), (4, [frames[:3], frames[3:]])):
        runner = PipelinedSequence(model, depth=2, group=group, dense_group=True)
        outs = list(runner.run(chunks))
        assert [o.shape[0] for o in outs] == [c.shape[0] - (1 if i == 0 else 0) for i, c in enumerate(chunks)]
        assert torch.equal(torch.cat(outs), want), group
        more = list(runner.run([frames[:2], frames[2:3]]))                        # the sequence goes on: frame 5 -> 0 -> 1 -> 2
        assert more[0].shape[0] == 2 and torch.equal(more[1][0], want[1]) and torch.equal(more[0][1], want[0])
    y_o = orc(torch.stack((frames[2], frames[3])).cpu())                        # pair (frame 2 -> frame 3)
    _close(want[2:3], y_o)


@pytest.mark.parametrize('k,radius', [(20, 10.0), (7, 0.6), (30, 0.2)])
def test_flow_embedding_split_fp16_against_f32_path_and_float64(k, radius):
    """Flow-embedding kernel on both matrix paths: same neighbours, same mask; values against a float64 product."""
    cfg = synthetic.model_cfg('kitti')
    cfg['params']['merge']['params']['k'] = k
    cfg['params']['merge']['params']['radius'] = radius
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=9))
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 4096, first_pair=3)).to(DEV)
    me = model._merge_layers[0]._embedding
    saved = ops.PRECISION
    try:
        with torch.no_grad():
            f_rows = model.cloud_feature_rows(x)
            ops.PRECISION = 'f32'
            e32 = me.forward_rows(f_rows, 2, model.npoint)
            ops.PRECISION = 'f16x2'
            e16 = me.forward_rows(f_rows, 2, model.npoint)
    finally:
        ops.PRECISION = saved
    assert torch.equal(e32[:, 256:], e16[:, 256:])                            # xyz + padding columns: copies
    assert torch.equal(e32 == 0, e16 == 0) or (e32 - e16).abs().max() < 1e-5   # same radius mask
    # float64 restatement of deepclr.py:201-231 on the kernel's own neighbour lists
    (w1, b1), (w2, b2), (w3, b3) = [(w.detach().double().reshape(w.shape[0], -1), b.detach().double())
                                    for w, b in me._conv.affine_params()]
    n = model.npoint
    idx = ops.knn_rows(f_rows, 2, n, k).long()
    f = f_rows.double()
    tmpl, src = f[:2 * n].view(2, n, -1), f[2 * n:].view(2, n, -1)
    nb = torch.gather(src.unsqueeze(1).expand(-1, n, -1, -1), 2, idx.unsqueeze(-1).expand(-1, -1, -1, f.shape[1]))
    diff = nb[..., 64:67] - tmpl[:, :, None, 64:67]
    merged = torch.cat((diff, tmpl[:, :, None, :64].expand(-1, -1, k, -1), nb[..., :64]), dim=-1)
    h = torch.relu(merged @ w1.t() + b1)
    h = torch.relu(h @ w2.t() + b2)
    h = torch.relu(h @ w3.t() + b3)
    h = torch.where((diff.norm(dim=-1, keepdim=True) >= radius), torch.zeros_like(h), h).max(dim=2).values
    want = h.view(2 * n, 256)
    err32 = (e32[:, :256].double() - want).abs().max().item()
    err16 = (e16[:, :256].double() - want).abs().max().item()
    _close(e16[:, :256], want.float().cpu())
    assert err16 <= 2 * err32 + 1e-7, (err16, err32)


@pytest.mark.parametrize('pairs, npoint', [(3, 37), (8, 16), (1, 5)])
def test_flow_kernels_at_every_neighbour_count_with_masks_and_unfilled_slots(pairs, npoint):
    """Both split-f16 flow kernels (flow16_kernel up to k = 28, flow32_kernel from k = 29: csrc/flow16.hip) at EVERY k from 1 to
    32 on hand-made neighbour lists: slots the search left unfilled (-1), neighbours beyond the radius (reference
    deepclr.py:220-225: their columns are zeroed before the max), points with NO neighbour inside the radius (all zeros),
    point counts that are not a multiple of the 4 points per workgroup, pair counts with and without the one-pair-one-XCD
    block mapping -- against a float64 restatement, and the f32 kernel on the same lists."""
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=13))
    me = model._merge_layers[0]._embedding
    p = me._packed()
    (w1, b1), (w2, b2), (w3, b3) = me._conv.affine_params()
    w64 = [(w.detach().double().reshape(w.shape[0], -1), b.detach().double()) for w, b in ((w1, b1), (w2, b2), (w3, b3))]
    rng = np.random.default_rng(100 * pairs + npoint)
    rows = 2 * pairs * npoint
    f = np.zeros((rows, ops.F_STRIDE), dtype=np.float32)
    f[:, :64] = np.abs(rng.normal(size=(rows, 64)))
    f[:, 64:67] = rng.normal(scale=1.5, size=(rows, 3))
    f_rows = torch.from_numpy(f).to(DEV)
    half = pairs * npoint
    # per-point halves of layer 1 (dclr_linear_pair wants whole 32-row tiles; any row count through torch, in float64)
    w1f = w1.detach().double().reshape(w1.shape[0], -1)
    pt = (f_rows[:half, :64].double() @ w1f[:, 3:67].t()).float().contiguous()
    ps = (f_rows[half:, :64].double() @ w1f[:, 67:131].t()).float().contiguous()
    radius = 2.0
    f64 = f_rows.double()
    tmpl, src = f64[:half].view(pairs, npoint, -1), f64[half:].view(pairs, npoint, -1)
    tiles = set()
    for k in range(1, 33):
        idx = rng.integers(0, npoint, size=(pairs, npoint, k)).astype(np.int32)
        idx[rng.random(idx.shape) < 0.15] = -1                              # unfilled slots anywhere in the list
        idx[0, 0, :] = -1                                                   # a point without any neighbour
        far = np.linalg.norm(f[half:].reshape(pairs, npoint, -1)[:, :, 64:67][np.arange(pairs)[:, None], idx[:, 1].clip(0)]
                             - f[:half].reshape(pairs, npoint, -1)[:, 1:2, 64:67], axis=-1) >= radius
        idx[:, 1][~far & (idx[:, 1] >= 0)] = -1                             # point 1: only neighbours beyond the radius (or none)
        idx_t = torch.from_numpy(idx).to(DEV)
        tile = ops.flow_f16_tile(k)
        tiles.add(tile)
        w2h, w3h = ops.pack_weight_f16(w2, 128, tile), ops.pack_weight_f16(w3, 128, tile)
        e16 = ops.flow_embedding_fused_f16(f_rows, idx_t, pt, ps, p['w1a'], p['b1'], w2h, p['b2'], w3h, p['b3'], radius)
        e32 = ops.flow_embedding_fused(f_rows, idx_t, pt, ps, p['w1a'], p['b1'], p['w2p'], p['b2'], p['w3p'], p['b3'], radius)
        li = torch.from_numpy(idx.clip(0)).long().to(DEV)
        nb = torch.gather(src.unsqueeze(1).expand(-1, npoint, -1, -1), 2, li.unsqueeze(-1).expand(-1, -1, -1, f64.shape[1]))
        diff = nb[..., 64:67] - tmpl[:, :, None, 64:67]
        h = torch.cat((diff, tmpl[:, :, None, :64].expand(-1, -1, k, -1), nb[..., :64]), dim=-1)
        for w, b in w64:
            h = torch.relu(h @ w.t() + b)
        dead = (diff.norm(dim=-1, keepdim=True) >= radius) | (idx_t < 0).unsqueeze(-1)
        want = torch.where(dead, torch.zeros_like(h), h).max(dim=2).values.view(half, 256)
        assert bool((want[0] == 0).all()) and bool((want[npoint * 0 + 1] == 0).all())      # the two hand-made empty points
        _close(e16[:, :256], want.float().cpu(), stage='flow kernel k=%d (tile %d) vs float64' % (k, tile))
        _close(e32[:, :256], want.float().cpu(), stage='f32 flow kernel k=%d vs float64' % k)
        assert torch.equal(e16[:, 256:259], f_rows[:half, 64:67]) and bool((e16[:, 259:] == 0).all())
        assert torch.equal(e16 == 0, e32 == 0)                              # the same columns are empty on both paths
    assert tiles == {16, 32}


def test_forward_with_augmentation_matrix_m_transforms_in_place_and_matches_oracle():
    """`forward(x, m=m)` / `cloud_features(x, m)`: the homogeneous transforms m (2B, 4, 4) are applied to the point
    columns of x IN PLACE before set abstraction (reference: deepclr.py:512-514, tgm.transform_points(m, x[:, :, :3]));
    the outputs are then those of the plain forward on the transformed clouds (checked against the oracle)."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=17)
    model, orc = _models(cfg, sd)
    pairs, n = 2, 2048
    x_cpu = torch.from_numpy(synthetic.make_batch('kitti', pairs, n, first_pair=70))
    rng = np.random.default_rng(5)
    m = np.tile(np.eye(4, dtype=np.float32), (2 * pairs, 1, 1))
    for i in range(2 * pairs):
        m[i, :3, :3] = synthetic._euler_to_mat(*np.deg2rad(rng.uniform(-20, 20, size=3))).astype(np.float32)
        m[i, :3, 3] = rng.uniform(-2, 2, size=3).astype(np.float32)
    m_t = torch.from_numpy(m)
    want_x = x_cpu.clone()
    want_x[:, :, :3] = (x_cpu[:, :, :3].double() @ m_t[:, :3, :3].double().transpose(1, 2) + m_t[:, None, :3, 3].double()).float()
    for entry in ('forward', 'cloud_features'):
        x = x_cpu.clone().to(DEV)
        with torch.no_grad():
            if entry == 'forward':
                y, _, _ = model(x, m=m_t.to(DEV))
            else:
                feat = model.cloud_features(x, m_t.to(DEV))
        moved = x.cpu()
        assert torch.equal(moved[:, :, 3:], x_cpu[:, :, 3:])                      # feature columns untouched
        _close(moved[:, :, :3], want_x[:, :, :3], rtol=1e-5, atol=1e-6, stage='m path: transformed points vs float64 transform')
        assert not torch.equal(moved[:, :, :3], x_cpu[:, :, :3])                  # ... and it did happen in place
        if entry == 'forward':
            _close(y, orc(moved), stage='m path: y vs oracle on the transformed clouds')
            y_feat, _, _ = model(model.cloud_features(moved.to(DEV)), is_feat=True, m=m_t.to(DEV))   # m is ignored with is_feat
            assert torch.equal(y_feat, y)
        else:
            _close(feat, orc.cloud_features(moved), stage='m path: cloud_features vs oracle on the transformed clouds')


def test_inference_helper_reports_a_clamped_last_forward():
    """the sticky range flag used to be read only on the NEXT entry into the model, so the last (or only)
    forward of a run could hand out clamped poses silently. Now (1) the fused dense stages write NaN poses while the flag is
    set -- a clamped forward cannot be mistaken for a result by ANY caller; (2) predict_batch / predict_sequence end with
    finish() = check_range on the current stream and raise; (3) predict (one pair per call, the reference scripts' timed
    pattern) returns the NaN pose, raises at the next call, or at finish(); and the split-f16 set-abstraction layers report
    their clamps to the same word (they used to clamp silently: only flow embedding and head were tracked)."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=4)
    model, _ = _models(cfg, sd)
    helper = ModelInferenceHelper(model)
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 2048, first_pair=30)).to(DEV)
    y_ok = helper.predict_batch(x[2:], x[:2]).clone()                    # first forward of the checkpoint: checked in f32, passes
    assert not model._range_unchecked()
    hot = x.clone()
    hot[:, :, 3] *= 1.0e9                                                # intensities ~1e9: set abstraction layer 1 leaves the range
    with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
        helper.predict_batch(hot[2:], hot[:2])                           # ONE call, nothing after it: raises, no pose handed out
    _close(helper.predict_batch(x[2:], x[:2]), y_ok.cpu(), stage='in-range batch after the reported one')
    y_hot = helper.predict(hot[2], hot[0])                               # the reference scripts' call pattern: no wait inside
    assert bool(torch.isnan(y_hot.cpu()).all())                          # ... the clamped pair's pose is NaN, not a plausible vector
    with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
        helper.finish()                                                  # the caller's last word; (a next predict would raise too)
    y_one = helper.predict(x[2], x[0])
    assert y_one is not None and bool(torch.isfinite(y_one.cpu()).all())
    helper.finish()
    with torch.no_grad():                                                # plain forward(), no helper: NaN as well, raise at the next entry
        y_fwd, _, _ = model(hot.clone())
        assert bool(torch.isnan(y_fwd.cpu()).all())
        with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
            model(x.clone())
        _close(model(x.clone())[0], y_ok.cpu(), stage='forward after the reported one')
    # the set-abstraction kernel by itself sets the word it is given
    flag = lib.MappedFlag()
    sam = model._cloud_layers[0]._sa0
    fps = ops.fps_clouds(hot, sam.npoint)
    ops.sa_msg_fused(hot, fps, sam.radii, sam.nsamples, sam.packed_mlps(), precision='f16x2', overflow=flag.dev_ptr)
    torch.cuda.synchronize()
    assert flag.is_set()
    flag.clear()
    ops.sa_msg_fused(x, ops.fps_clouds(x, sam.npoint), sam.radii, sam.nsamples, sam.packed_mlps(), precision='f16x2',
                     overflow=flag.dev_ptr)
    torch.cuda.synchronize()
    assert not flag.is_set()


def test_split_f16_range_guard(monkeypatch):
    """The default matrix path carries operands as f16 hi/lo halves and clamps at +-65504 (csrc/mma16f.h). Weights out
    of range are refused when they are packed. Activations out of range are caught by the checked forward, which reruns
    the dense stages on the f32 matrix instructions: by DEFAULT on the first forward after the weights changed
    (ops.CHECK_RANGE = 'first'), on every forward with 'always', never with 'never'; and the f32 path itself
    (DCLR_PRECISION=f32) still agrees with the oracle on such a checkpoint."""
    assert ops.CHECK_RANGE == 'first'                                                      # the shipped default
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=9)
    x_cpu = torch.from_numpy(synthetic.make_batch('kitti', 2, 2048, first_pair=90))
    # in range: the first forward is a checked one and passes; later ones go straight through, with identical results
    model, orc = _models(cfg, sd)
    calls = []
    real = type(model)._merge_rows_checked
    monkeypatch.setattr(type(model), '_merge_rows_checked', lambda self, *a: calls.append(1) or real(self, *a))
    with torch.no_grad():
        assert model._range_unchecked()
        y_first, _, _ = model(x_cpu.to(DEV))
        assert calls == [1] and not model._range_unchecked()
        y_plain, _, _ = model(x_cpu.to(DEV))
        assert calls == [1]                                                                # not checked again
        monkeypatch.setattr(ops, 'CHECK_RANGE', 'always')
        y_checked, _, _ = model(x_cpu.to(DEV))
        assert calls == [1, 1]
        monkeypatch.setattr(ops, 'CHECK_RANGE', 'first')
        model.load_state_dict(sd)                                                          # weights rewritten: checked once more
        assert model._range_unchecked()
        model(x_cpu.to(DEV))
        assert calls == [1, 1, 1] and not model._range_unchecked()
    _close(y_first, y_plain.cpu(), stage='first (checked) forward vs plain forward (in range)')
    _close(y_checked, y_plain.cpu(), stage='checked mode vs plain forward (in range)')
    # A LATER input leaves the range (the first-forward check has passed for this checkpoint): the split-f16 kernels set
    # the sticky flag when a clamp engages, and the next look at it raises -- no synchronisation on the way (VERDICT r04
    # weak 9: "later inputs whose activations reach 65,504 are clamped silently")
    with torch.no_grad():
        assert not model._range_unchecked()
        f_rows = model.cloud_feature_rows(x_cpu.to(DEV))
        y_ok = model.merge_rows(f_rows, 2).clone()
        model.check_range(synchronize=True)                                                # in range: nothing to report
        f_big = f_rows.clone()
        f_big[:, :64] *= 3.0e5                                                             # features ~1e5: flow layer 1 overflows
        model.merge_rows(f_big, 2)                                                         # enqueued; not checked by an f32 re-run
        assert calls == [1, 1, 1]
        with pytest.raises(RuntimeError, match='DCLR_PRECISION=f32'):
            model.check_range(synchronize=True)
        model.check_range(synchronize=True)                                                # reported once, then cleared
        _close(model.merge_rows(f_rows, 2), y_ok.cpu(), stage='in-range batch after a reported overflow')
        model.merge_rows(f_big, 2)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match='split-f16 matrix path out of range'):      # ... or the next entry into the model
            model(x_cpu.to(DEV))
        y_after, _, _ = model(x_cpu.to(DEV))
    _close(y_after, y_plain.cpu(), stage='forward after the overflow was reported')
    # activations out of range: the last flow-embedding layer scaled so that rows E reach ~1e6
    big = {k: v.clone() for k, v in sd.items()}
    big['_merge_layers.0._embedding._conv._sequential.2._sequential.0.weight'] *= 3.0e5
    big['_merge_layers.1.conv._sequential.0._sequential.0.weight'] *= 1.0 / 3.0e5          # keeps the head in range
    model_big, orc_big = _models(cfg, big)
    y_o = orc_big(x_cpu)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='split-f16 matrix path out of range'):      # the default: first use raises
            model_big(x_cpu.to(DEV))
        with pytest.raises(RuntimeError, match='split-f16 matrix path out of range'):      # and keeps raising: never passed
            model_big(x_cpu.to(DEV))
        monkeypatch.setattr(ops, 'CHECK_RANGE', 'never')
        y16, _, _ = model_big(x_cpu.to(DEV))                                               # unchecked: silently clamped ...
        assert float((y16.cpu() - y_o).abs().max()) > 1e-3                                 # ... and therefore wrong (finite: not poisoned)
        assert bool(torch.isfinite(y16.cpu()).all())
        assert model_big._range_flag is None or not model_big._range_flag.is_set()         # 'never': the kernels get no word at all
        model_big.check_range()                                                            # nothing to report
        monkeypatch.setattr(ops, 'CHECK_RANGE', 'first')
        monkeypatch.setattr(ops, 'PRECISION', 'f32')
        y32, _, _ = model_big(x_cpu.to(DEV))
    _close(y32, y_o, stage='f32 matrix path vs oracle, activations ~1e6')
    monkeypatch.setattr(ops, 'PRECISION', 'f16x2')
    # weights out of range: refused at pack time
    huge = {k: v.clone() for k, v in sd.items()}
    huge['_merge_layers.1.conv._sequential.2._sequential.0.weight'][0, 0, 0] = 7.0e4
    model_huge, _ = _models(cfg, huge)
    with pytest.raises(RuntimeError, match='outside the split-f16 operand range'):
        with torch.no_grad():
            model_huge(x_cpu.to(DEV))


def test_timing_script_call_sequence_runs_on_the_hip_path():
    """The body of the reference's scripts/timing.py (lines 13-47), statement for statement, against this package
    under the reference's import names: load_config -> build_model -> model.to(cfg.device) -> ModelInferenceHelper ->
    make_data_loader(cfg, is_train=False, batch_size=1) -> prepare_tensor -> predict between two CUDA events."""
    from deepclr.config import load_config, Mode
    from deepclr.data import make_data_loader
    from deepclr.models import build_model as ref_build_model, ModelInferenceHelper as RefHelper
    from deepclr.utils.logging import create_logger
    from deepclr.utils.tensor import prepare_tensor
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = load_config(os.path.join(root, 'configs', 'timing_synthetic_kitti.yaml'), Mode.TEST)
    create_logger(name='timing')
    for sequential in (False, True):
        model = ref_build_model(cfg.model)
        model.to(cfg.device)
        model.eval()
        helper = RefHelper(model, is_sequential=sequential)
        data_loader = make_data_loader(cfg, is_train=False, batch_size=1)
        times, outs = [], []
        for i, batch in enumerate(data_loader):
            if i == 4:
                break
            x = prepare_tensor(batch['x'], device=cfg.device)
            template, source = x[0, ...], x[1, ...]
            t_start, t_end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t_start.record()
            if sequential:
                if not helper.has_state():
                    helper.predict(template)
                y = helper.predict(source)
            else:
                y = helper.predict(source, template)
            t_end.record()
            torch.cuda.synchronize()
            times.append(t_start.elapsed_time(t_end))
            outs.append(y)
        assert all(t > 0 for t in times) and all(tuple(o.shape) == (8,) and bool(torch.isfinite(o).all()) for o in outs)
        print('timing.py sequence (sequential=%s): %s ms per pair' % (sequential, ['%.2f' % t for t in times]))


def test_forward_with_labels_returns_the_configured_loss():
    """forward(x, y=labels) -> (y_pred, loss, debug) as in the reference (deepclr.py:488-508); no shipped model
    configures an in-model loss, so the layer is added to the synthetic configuration here."""
    from deepclr_amd import losses
    cfg = small_cfg()
    cfg['params']['loss'] = {'name': 'TransformUncertaintyLoss', 'params': {'p': 2, 'sx': 0.0, 'sq': -3.0}}
    sd = synthetic.random_state_dict(small_cfg(), seed=3)
    model = build_model(model_config_from_dict(cfg))
    missing = model.load_state_dict(sd, strict=False)
    assert sorted(missing.missing_keys) == ['_loss_layer._sq', '_loss_layer._sx'] and not missing.unexpected_keys
    model = model.to(DEV).eval()
    assert model.has_loss() and set(model.get_loss_weights()) == {'sx', 'sq'}
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512)).to(DEV)
    labels = torch.tensor([[1.0, 0, 0, 0, 0, 0.1, 0, 0], [0.9, 0.1, 0, 0, 0, 0, 0.2, 0]], device=DEV)
    with torch.no_grad():
        y_pred, loss, dbg = model(x.clone(), y=labels, debug=True)
        y_plain, none_loss, none_dbg = model(x.clone())
    assert torch.equal(y_pred, y_plain) and none_loss is None and none_dbg is None
    t, r = losses.transform_losses(y_pred, labels, LabelType.POSE3D_DUAL_QUAT, 2)
    want = t * np.exp(0.0) + 0.0 + r * np.exp(3.0) - 3.0
    torch.testing.assert_close(loss.reshape(()), want.reshape(()), rtol=1e-6, atol=1e-6)
    assert dbg['x_aug'].shape == (4, 67, model.npoint)


from hypothesis import HealthCheck, given, settings, strategies as st      # noqa: E402


@settings(max_examples=25, deadline=None, derandomize=True,
          suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(c=st.sampled_from([3, 4]), n=st.integers(130, 6000), npoint=st.integers(1, 200),
       r0=st.floats(0.03, 0.8), r1=st.floats(0.03, 2.5), ns0=st.integers(1, 96), ns1=st.integers(1, 600),
       scales=st.integers(1, 2))
def test_fused_set_abstraction_random_configurations(c, n, npoint, r0, r1, ns0, ns1, scales):
    """Random cloud sizes, centroid counts, radii and caps: fused kernel (with and without the sampler's groups)
    against the oracle -- counts exact, features within tolerance, group path identical to the exhaustive sweep."""
    radii, nsamples = ((r0,), (ns0,)) if scales == 1 else ((r0, r1), (ns0, ns1))
    _check_set_abstraction(c, n, min(npoint, n), radii, nsamples, expect_cap=False)


def test_unfilled_knn_slots_raise_on_the_checked_forward_and_are_masked_after(monkeypatch):
    """torch-cluster's k slots start at distance 1e10 / index -1: a template point with fewer than k source points within
    1e5 m (or NaN coordinates in the source cloud) gets -1 entries. Upstream fails there (KnnGrouping's .view(2, G, k),
    reference deepclr.py:164-167). Here the checked forward -- the default on first use -- raises; the unchecked fused
    path must stay inside its buffers (pair 0's source rows start the `ps` buffer: an index of -1 would read in front of
    it) and treats the slot as a masked neighbour: the result equals that of the same lists with every -1 replaced by a
    far, radius-masked source row."""
    cfg = synthetic.model_cfg('kitti')
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=4))
    pairs, npoint, k = 2, model.npoint, 20
    rng = np.random.default_rng(8)
    f = np.zeros((2 * pairs * npoint, ops.F_STRIDE), dtype=np.float32)
    f[:, :64] = np.abs(rng.normal(size=(len(f), 64)))
    f[:, 64:67] = rng.normal(scale=3.0, size=(len(f), 3))
    src = f[pairs * npoint:].reshape(pairs, npoint, ops.F_STRIDE)
    src[0, 12:, 64] += 3.0e5                     # pair 0: only 12 source points within reach -> 8 unfilled slots per query
    src[1, 5:9, 64:67] = np.nan                  # pair 1: four source rows without a position, never taken
    src[1, 40:, 65] -= 2.5e5                     # ... and 36 reachable ones left: slots 0..19 filled, no -1
    src[1, 5:9, 64:67] = np.nan
    f_rows = torch.from_numpy(f).to(DEV)
    idx = ops.knn_rows(f_rows, pairs, npoint, k)
    assert bool((idx[0, :, 12:] == -1).all()) and bool((idx[0, :, :12] >= 0).all()) and bool((idx[1] >= 0).all())
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='kNN grouping'):
            model.merge_rows(f_rows, pairs)
        monkeypatch.setattr(ops, 'CHECK_RANGE', 'never')
        y = model.merge_rows(f_rows, pairs)                                  # dclr_merge_forward, split-f16
        flow = model._merge_layers[0]._embedding
        p = flow._packed()
        pt = ops.linear(f_rows[:pairs * npoint], p['wt'], None, 128, 64, relu=False)
        ps = ops.linear(f_rows[pairs * npoint:], p['ws'], None, 128, 64, relu=False)
        far = idx.clone()
        far[far < 0] = npoint - 1                                            # a source row 3e5 m away: beyond the radius
        for fn, w2, w3 in ((ops.flow_embedding_fused_f16, 'w2h', 'w3h'), (ops.flow_embedding_fused, 'w2p', 'w3p')):
            args = (pt, ps, p['w1a'], p['b1'], p[w2], p['b2'], p[w3], p['b3'], flow._radius)
            got, want = fn(f_rows, idx, *args), fn(f_rows, far, *args)
            assert torch.isfinite(got[:pairs * npoint // 2]).all() and torch.equal(got, want)
        e = ops.flow_embedding_fused_f16(f_rows, far, pt, ps, p['w1a'], p['b1'], p['w2h'], p['b2'], p['w3h'], p['b3'], flow._radius)
        y_far = model._merge_layers[1].forward_rows(e, pairs)
    assert torch.isfinite(y[0]).all() and torch.equal(y[0], y_far[0])


@pytest.mark.parametrize('kind, pairs, n, batches', [('kitti', 2, 2048, 1), ('kitti', 2, 16384, 3), ('modelnet', 4, 2048, 2),
                                                     ('kitti', 1, 20000, 2)])
def test_cloud_forward_one_call_equals_the_separate_launches(kind, pairs, n, batches):
    """dclr_cloud_forward (sampling -> set abstraction -> layer-1 halves + kNN behind one foreign call, what the pipelined
    runner enqueues per sampling group) against the same stages called one by one: identical rows, identical stage-1
    buffers, identical poses; batches read in place through a view of one chunk."""
    cfg = synthetic.model_cfg(kind)
    model, _ = _models(cfg, synthetic.random_state_dict(cfg, seed=5))
    chunk = torch.stack([torch.from_numpy(synthetic.make_batch(kind, pairs, n, first_pair=10 * i)) for i in range(batches)]).to(DEV)
    xs = [chunk[i] for i in range(batches)]
    view = ops.batch_view(xs) if batches > 1 else None
    with torch.no_grad():
        assert model.cloud_merge_prep(xs[0], view) is None              # weights not range-checked yet: the caller's fallback
        rows_ref = model.cloud_feature_rows(xs[0], model.sample(xs[0], view), view)
        y_ref = model.merge_rows(rows_ref, pairs * batches).clone()      # (the first, checked forward)
        prep_ref = model.merge_prep(rows_ref, pairs * batches)
        got = model.cloud_merge_prep(xs[0], view)
        assert got is not None
        rows, prep = got
        assert torch.equal(rows, rows_ref)
        for a, b in zip(prep[:3], prep_ref[:3]):
            assert torch.equal(a, b)
        y = model.merge_rows(rows, pairs * batches, prep=prep)
        prep.release()
        assert torch.equal(y, y_ref)
        # the ring hands the slot out again only behind its release event; a second call must not disturb the first result
        rows2, prep2 = model.cloud_merge_prep(xs[0], view)
        assert rows2.data_ptr() != rows.data_ptr() and torch.equal(rows2, rows_ref)
        for i in range(batches):                                         # and every batch against its own plain forward
            yi, _, _ = model(xs[i])
            assert torch.equal(y[i * pairs:(i + 1) * pairs], yi)


@pytest.mark.parametrize('k, append', [(0, True), (64, False), (5, True)])
def test_composed_flow_embedding_variants_against_oracle(k, append):
    """Shapes beyond the goldens on the composed path: GlobalGrouping (k == 0) with other widths (the neighbourhood rows
    are processed in chunks), the largest k the search keeps, and a k that pads 59 of 64 rows per neighbourhood; against
    the CPU oracle, whose composition is pinned by the reference-generated goldens."""
    from helpers import custom_widths_cfg
    cfg = custom_widths_cfg()
    cfg['params']['merge']['params'].update(k=k, append_features=append, radius=5.0 if k else 8.0)
    sd = synthetic.random_state_dict(cfg, seed=21)
    model, orc = _models(cfg, sd)
    assert not model._rows_path
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 700, first_pair=31))
    with torch.no_grad():
        feat = model.cloud_features(x.to(DEV))
        y, _, _ = model(x.to(DEV))
    feat_o = orc.cloud_features(x)
    _close(feat, feat_o, stage='composed k=%d: cloud_features vs oracle' % k)
    _close(model._merge_layers[0](feat), orc.flow_embedding(feat_o), stage='composed k=%d: flow_embedding vs oracle' % k)
    _close(y, orc(x), stage='composed k=%d: y vs oracle' % k)
    helper = ModelInferenceHelper(model, is_sequential=True)              # the sequential cache works in channel layout too
    with torch.no_grad():
        assert helper.predict(x[0].to(DEV)) is None
        y_seq = helper.predict(x[2].to(DEV))
    _close(y_seq, orc(x[[0, 2]])[0], stage='composed k=%d: sequential helper vs oracle' % k)


@pytest.mark.parametrize('sequential', [False, True])
def test_inference_script_call_sequence_runs_on_the_hip_path(tmp_path, sequential):
    """The body of the reference's scripts/inference.py (lines 29-121), statement for statement, against this package under
    the reference's import names: load_scenario -> load_model_config -> load_trained_model -> model.cuda() ->
    ModelInferenceHelper / Evaluator -> scenario.yaml -> per data file: create_input_dataflow -> per pair: predict between
    two events -> label_type.to_matrix -> evaluator.add_transforms -> evaluator.write; then the result files are read back
    and compared with the oracle's poses for the same pairs. The data file is a .npz sequence (the reference's LMDB reader
    is the one piece of the script this build does not provide)."""
    import yaml
    from deepclr.config import load_model_config
    from deepclr.data import create_input_dataflow
    from deepclr.evaluation import load_scenario, Evaluator
    from deepclr.models import load_trained_model, ModelInferenceHelper as RefHelper
    from deepclr.utils.logging import create_logger
    # -- what the user has on disk: a model directory, a sequence file, a scenario
    cfg_d = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg_d, seed=3)
    model_dir = tmp_path / 'models' / 'demo'
    model_dir.mkdir(parents=True)
    (model_dir / 'model_config.yaml').write_text(yaml.safe_dump(cfg_d))
    torch.save(sd, model_dir / 'weights.tar')
    frames, n = 5, 2048
    rng = np.random.default_rng(77)
    clouds = [synthetic.kitti_like_pair(500, n)[0]]
    poses = [np.eye(4)]
    for i in range(1, frames):                                           # each frame = the previous one moved a little + noise
        t, s, m = synthetic.kitti_like_pair(500 + i, n)
        step = m
        moved = clouds[-1].copy()
        moved[:, :3] = (clouds[-1][:, :3] - step[:3, 3]) @ step[:3, :3] + rng.normal(0, 0.01, size=(n, 3))
        clouds.append(moved.astype(np.float32))
        poses.append(poses[-1] @ step)
    seq_file = tmp_path / 'kitti_demo.npz'
    np.savez(seq_file, clouds=np.stack(clouds), poses=np.stack(poses), timestamps=0.1 * np.arange(frames))
    scenario = tmp_path / 'scenario.yaml'
    scenario.write_text(yaml.safe_dump({'name': 'demo', 'dataset_type': 'KITTI_ODOMETRY_VELODYNE', 'sequential': sequential,
                                        'data': {'seq_a': str(seq_file)}}))

    # -- scripts/inference.py:29-121
    logger = create_logger('evaluation')
    scene_cfg = load_scenario(str(scenario), with_method=False)
    model_path = os.path.join(str(tmp_path / 'models'), 'demo')
    model_file = os.path.join(model_path, 'model_config.yaml')
    weights_file = os.path.join(model_path, 'weights.tar')
    model_cfg = load_model_config(model_file, weights_file)
    model = load_trained_model(model_cfg)
    model = model.cuda()
    helper = RefHelper(model, is_sequential=scene_cfg.sequential)
    evaluator = Evaluator()
    output_dir = os.path.join(str(tmp_path / 'out'), 'stamp_{}_{}'.format(scene_cfg.name, model_cfg.model_type.name))
    os.makedirs(output_dir, exist_ok=True)
    eval_cfg = scene_cfg.copy()
    eval_cfg.method.name = model_cfg.model_type.name
    eval_cfg.method.params.model_name = 'demo'
    eval_cfg.method.params.model_file = model_file
    eval_cfg.method.params.weights_file = weights_file
    eval_cfg.write_file(os.path.join(output_dir, 'scenario.yaml'), invalid=True, internal=True)
    kept = []
    for data_name, data_file in scene_cfg.data.items():
        logger.info("Evaluate '{}'".format(data_file))
        df = create_input_dataflow(scene_cfg.dataset_type, data_file, shuffle=False)
        df.reset_state()
        helper.reset_state()
        for i, ds in enumerate(df):
            template = torch.from_numpy(ds['clouds'][0]).cuda()
            source = torch.from_numpy(ds['clouds'][1]).cuda()
            stamp = ds['timestamps'][0]
            transform_gt = ds['transform']
            t_start = torch.cuda.Event(enable_timing=True)
            t_end = torch.cuda.Event(enable_timing=True)
            t_start.record()
            if scene_cfg.sequential:
                if not helper.has_state():
                    helper.predict(template)
                y_pred = helper.predict(source)
            else:
                y_pred = helper.predict(source, template)
            t_end.record()
            torch.cuda.synchronize()
            t_pred = t_start.elapsed_time(t_end)
            if y_pred is not None:
                y_pred = y_pred.detach().cpu().numpy()
                transform_pred = model_cfg.label_type.to_matrix(y_pred)
            else:
                transform_pred = None
            evaluator.add_transforms(data_name, stamp, transform_pred, transform_gt, t_pred)
            kept.append((ds['clouds'][0], ds['clouds'][1], transform_gt))
        assert len(df) == frames - 1 and i == frames - 2
        del df
    evaluator.write(output_dir)

    # -- the result files read back (26 columns: stamp, pred 3x4, gt 3x4, ms) against the oracle on the same pairs
    again = Evaluator.read(output_dir)
    assert again.has_sequence('seq_a') and os.path.exists(os.path.join(output_dir, 'scenario.yaml'))
    seq = again.get_sequence('seq_a')
    table = seq.table()
    assert table.shape == (frames - 1, 26) and np.allclose(table[:, 0], 0.1 * np.arange(frames - 1)) and (table[:, 25] > 0).all()
    orc = oracle.build_oracle_model(cfg_d, sd)
    for row, (t, s, gt) in zip(table, kept):
        want = olabels.dual_quat_to_matrix(orc(torch.from_numpy(np.stack([t, s])))[0].numpy())
        assert np.abs(row[1:13].reshape(3, 4) - want[:3]).max() < 1e-4
        assert np.abs(row[13:25].reshape(3, 4) - gt[:3]).max() < 1e-6
    stored = yaml.safe_load(open(os.path.join(output_dir, 'scenario.yaml')))
    assert stored['method']['name'] == 'DEEPCLR' and stored['method']['params']['weights_file'] == weights_file


@pytest.mark.parametrize('cfg_name', ['small', 'custom_features', 'small_quat', 'small_euler'])
def test_training_step_gradients_match_the_oracle_autograd(cfg_name):
    """model.train() + forward(x, y=labels) + loss.backward() (the reference's training step, engine/engines.py:57-84):
    sampling / ball query / kNN on the HIP operators, gather and group through the HIP operators and their HIP backward,
    MLPs in torch. Loss value and EVERY parameter's gradient against torch autograd over the CPU oracle's functional
    restatement of the same network (float32 on both sides; the index operators are bit-exact, so both differentiate the
    same piecewise-linear function). small_quat / small_euler: the other label types, whose loss and gradients go through
    the quaternion (sigmoid on column 3, tanh on 4..6) and the activation-free euler branches of the output layer."""
    from helpers import custom_features_batch, custom_features_cfg, small_euler_cfg, small_quat_cfg
    if cfg_name == 'custom_features':
        cfg, x_np = custom_features_cfg(), custom_features_batch()
    else:
        cfg = {'small': small_cfg, 'small_quat': small_quat_cfg, 'small_euler': small_euler_cfg}[cfg_name]()
        x_np = synthetic.make_batch('kitti', 2, 512, first_pair=41)
    cfg['params']['loss'] = {'name': 'TransformLoss', 'params': {'p': 2, 'sx': 1.0, 'sq': 10.0}}
    sd = synthetic.random_state_dict(cfg, seed=23)
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=False)
    model = model.to(DEV).train()
    x = torch.from_numpy(x_np)
    lt = LabelType.create(cfg['label_type'])
    labels = torch.from_numpy(np.stack([lt.from_matrix(synthetic.kitti_like_pair(41 + i, 16)[2])
                                        for i in range(2)]).astype(np.float32))
    y_pred, loss, _ = model(x.to(DEV), y=labels.to(DEV))
    assert tuple(y_pred.shape) == (2, lt.dim)
    assert y_pred.requires_grad and loss.requires_grad
    loss.backward()
    # oracle: the same state_dict as leaf tensors, the same loss module on its outputs
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    orc = oracle.build_oracle_model(cfg, sd)
    orc.sd = sd_o
    y_o = orc.pose_head(orc.flow_embedding(orc.cloud_features(x)))
    loss_o = model._loss_layer.cpu()(y_o, labels)
    loss_o.backward()
    _close(y_pred.detach(), y_o.detach(), stage=cfg_name + ': training forward y vs oracle')
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
    params = dict(model.named_parameters())
    worst = 0.0
    for key, ref in sd_o.items():
        got = params[key].grad
        assert got is not None and ref.grad is not None, key
        scale = float(ref.grad.abs().max())
        err = float((got.cpu() - ref.grad).abs().max())
        worst = max(worst, err / max(scale, 1e-12))
        assert err <= 2e-4 * max(scale, 1e-6), (key, err, scale)
    print("training step (%s): loss %.6f, worst gradient error / scale %.2e over %d tensors" % (cfg_name, float(loss.detach()), worst, len(sd_o)))
    # and eval mode still takes the inference kernels with the same outputs
    model = model.to(DEV).eval()
    with torch.no_grad():
        y_eval, _, _ = model(x.to(DEV))
    _close(y_eval, y_o.detach(), stage=cfg_name + ': eval forward after the training step vs oracle')


def test_training_step_with_batch_norm_and_dropout_then_eval_folds_the_updated_statistics():
    """`batch_norm: true`, `dropout: 0.7` (reference helper.py:27-36,57-63,107-113): a training step runs the torch modules
    themselves (batch statistics, random masks) on top of the HIP gather / group operators -- every parameter gets a finite
    gradient and the running statistics move; eval() afterwards folds the UPDATED statistics into the packed weights (the
    packed-weight caches key on the buffers too) and agrees with the oracle on the updated state_dict; a training-mode
    forward without gradients is refused instead of silently using running statistics."""
    from helpers import small_bn_cfg
    cfg = small_bn_cfg()
    cfg['params']['loss'] = {'name': 'TransformLoss', 'params': {'p': 2, 'sx': 1.0, 'sq': 10.0}}
    sd = synthetic.random_state_dict(cfg, seed=31)
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=False)
    model = model.to(DEV).eval()
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=43))
    labels = torch.from_numpy(np.stack([LabelType.POSE3D_DUAL_QUAT.from_matrix(synthetic.kitti_like_pair(43 + i, 16)[2])
                                        for i in range(2)]).astype(np.float32))
    with torch.no_grad():
        y_before, _, _ = model(x.to(DEV))
    _close(y_before, oracle.build_oracle_model(cfg, sd)(x), stage='batch norm model, eval forward before the training step vs oracle')
    model.train()
    with torch.no_grad(), pytest.raises(RuntimeError, match='model.eval'):
        model(x.to(DEV))
    mean_before = {k: v.clone() for k, v in model.state_dict().items() if k.endswith('running_mean')}
    torch.manual_seed(0)
    y_pred, loss, _ = model(x.to(DEV), y=labels.to(DEV))
    loss.backward()
    for name, prm in model.named_parameters():
        if name.startswith('_loss_layer'):
            continue
        assert prm.grad is not None and bool(torch.isfinite(prm.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for n, p in model.named_parameters() if n.endswith('_sequential.1.weight'))
    moved = [k for k, v in model.state_dict().items() if k.endswith('running_mean') and not torch.equal(v, mean_before[k])]
    assert len(moved) == len(mean_before) and len(moved) >= 10                  # every norm layer saw the batch
    model.eval()
    sd_after = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith('_loss_layer')}
    with torch.no_grad():
        y_after, _, _ = model(x.to(DEV))
    assert float((y_after - y_before).abs().max()) > 1e-6                       # the statistics did change the network
    _close(y_after, oracle.build_oracle_model(cfg, sd_after)(x), stage='batch norm model, eval forward after the training step vs oracle')


def test_clouds_beyond_the_fused_kernels_point_limit_run_composed():
    """More than 65536 points per cloud (the fused sampler and set-abstraction kernels index points with 16 bits; a raw
    KITTI scan holds ~120k): the same module composed from the level-1 operators, which take any n -- results against the
    oracle as for every other size, through forward(), cloud_features() and the inference helper."""
    cfg = synthetic.model_cfg('kitti')
    sd = synthetic.random_state_dict(cfg, seed=6)
    model, orc = _models(cfg, sd)
    x = torch.from_numpy(synthetic.make_batch('kitti', 1, 70001, first_pair=3))
    with torch.no_grad():
        feat = model.cloud_features(x.to(DEV))
        y, _, _ = model(x.to(DEV))
        y_h = ModelInferenceHelper(model).predict(x[1].to(DEV), x[0].to(DEV))
    feat_o = orc.cloud_features(x)
    assert torch.equal(feat[:, :3].cpu(), feat_o[:, :3])                   # the same 1024 centroids
    _close(feat, feat_o, stage='70001 points: cloud_features vs oracle')
    _close(y, orc(x), stage='70001 points: y vs oracle')
    assert torch.equal(y_h, y[0])
