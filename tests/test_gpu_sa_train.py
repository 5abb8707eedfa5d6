"""GPU: the fused training form of the set abstraction (csrc/sa_train.hip, libdeepclr_amd_train.so) against the composed
training path (PointnetSAModuleMSG._forward_composed(train=True): torch autograd over the grouped tensor) and the CPU
oracle's autograd; determinism, optimizer steps, memory."""
import numpy as np
import pytest
import torch

import oracle
from deepclr_amd import ops, synthetic
from deepclr_amd.config import model_config_from_dict
from deepclr_amd.labels import LabelType
from deepclr_amd.models import build_model
from helpers import small_cfg, small_transform_cfg, small_two_level_cfg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _full_f32():
    """The composed path's convolutions and GEMMs in plain f32 (no reduced-precision inner products) for the comparison."""
    saved = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = saved


def _model(cfg, seed=3, loss=False):
    if loss:
        cfg['params']['loss'] = {'name': 'TransformLoss', 'params': {'p': 2, 'sx': 1.0, 'sq': 10.0}}
    sd = synthetic.random_state_dict(cfg, seed=seed)
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=not loss)
    return model.to(DEV), sd


def _split(x):
    x = x.to(DEV)
    xyz = x[:, :, :3].contiguous()
    feats = x[:, :, 3:].transpose(1, 2).contiguous() if x.shape[2] > 3 else None
    return xyz, feats


def _dense_clouds(b, n, seed):
    """KITTI-sized clouds packed densely enough that every ball of the shipped radii (0.5 / 1.0) holds more than its
    nsample (512 / 1024) points: the saturated case."""
    rng = np.random.default_rng(seed)
    x = np.empty((b, n, 4), dtype=np.float32)
    x[:, :, :2] = rng.uniform(-1.5, 1.5, size=(b, n, 2))
    x[:, :, 2] = rng.uniform(-0.3, 0.3, size=(b, n))
    x[:, :, 3] = rng.uniform(0.0, 1.0, size=(b, n))
    return torch.from_numpy(x)


def _close(got, want, rtol=1e-5, atol=1e-6):
    want = want.detach().cpu()
    scale = max(1.0, float(want.abs().max()))
    torch.testing.assert_close(got.detach().cpu(), want, rtol=rtol, atol=atol * scale)


def _sa_params(sa):
    return [p for stack in sa.mlps for u in stack for p in (u.conv.weight, u.conv.bias)]


def _cpu_channel(sa, xyz, feats, new_xyz, b, ch, p, k):
    """Output channel `ch` of centroid p in cloud b for neighbour point k, in float64 on the CPU."""
    s, c = divmod(ch, 32)
    x = (xyz[b, k].double() - new_xyz[b, p].double())
    if feats is not None:
        x = torch.cat((x, feats[b, :, k].double()))
    for j, u in enumerate(sa.mlps[s]):
        w = u.conv.weight.detach().cpu().double().reshape(u.conv.weight.shape[0], -1)
        x = torch.relu(w @ x + u.conv.bias.detach().cpu().double())
    return float(x[c])


def _forward_case(sa, x, arg_checks=64):
    xyz, feats = _split(x)
    sa.fused_training = True
    assert sa.fused_training_applies(xyz, feats)
    with torch.no_grad():
        want_xyz, want = sa._forward_composed(xyz, feats, train=True)
        got_xyz, got = sa._forward_fused_train(xyz, feats)
    assert torch.equal(got_xyz, want_xyz)
    _close(got, want)
    # the argmax point of sampled (cloud, channel, centroid) entries reproduces the stored maximum
    out, arg = ops.sa_msg_train_forward(xyz, feats, got_xyz,
                                        [ops.ball_query(r, s, xyz, got_xyz) for r, s in zip(sa.radii, sa.nsamples)],
                                        ops.pack_sa_train_mlp(_sa_params(sa), sa._in_feat))
    assert torch.equal(out, got)
    rng = np.random.default_rng(0)
    xyz_c, new_c, arg_c, out_c = xyz.cpu(), got_xyz.cpu(), arg.cpu(), out.cpu()
    feats_c = None if feats is None else feats.cpu()
    for _ in range(arg_checks):
        b, ch, p = (int(rng.integers(0, d)) for d in out.shape)
        k = int(arg_c[b, ch, p])
        assert 0 <= k < xyz.shape[1]
        v = _cpu_channel(sa, xyz_c, feats_c, new_c, b, ch, p, k)
        assert abs(v - float(out_c[b, ch, p])) <= 1e-5 * max(1.0, abs(v)), (b, ch, p, k, v, float(out_c[b, ch, p]))


def test_forward_matches_the_composed_path_small_and_modelnet():
    model, _ = _model(small_cfg())
    _forward_case(model._cloud_layers[0]._sa0, torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=5)))
    model, _ = _model(synthetic.model_cfg('modelnet'))
    _forward_case(model._cloud_layers[0]._sa0, torch.from_numpy(synthetic.make_batch('modelnet', 1, 1024, first_pair=2)))


def test_forward_matches_the_composed_path_on_saturated_kitti_balls():
    model, _ = _model(synthetic.model_cfg('kitti'))
    sa = model._cloud_layers[0]._sa0
    assert sa.nsamples == [512, 1024]
    x = _dense_clouds(2, 16384, seed=7)
    xyz, _ = _split(x)
    with torch.no_grad():
        new_xyz = ops.gather_operation(xyz.transpose(1, 2).contiguous(), ops.furthest_point_sample(xyz, sa.npoint))
        bq = ops.ball_query(sa.radii[0], sa.nsamples[0], xyz, new_xyz.transpose(1, 2).contiguous())
    # saturated: the last slot differs from the first (not padding) for almost every centroid
    assert float((bq[:, :, -1] != bq[:, :, 0]).float().mean()) > 0.9
    _forward_case(sa, x)


def _grads(sa, xyz, feats, g, fused):
    for p in sa.parameters():
        p.grad = None
    out = sa._forward_fused_train(xyz, feats)[1] if fused else sa._forward_composed(xyz, feats, train=True)[1]
    (out * g).sum().backward()
    return out.detach(), [p.grad.clone() for p in _sa_params(sa)]


def _check_grads(got, want, names):
    for name, a, b in zip(names, got, want):
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        assert err <= 2e-4 * max(scale, 1e-6), (name, err, scale)


@pytest.mark.parametrize('case', ['small', 'empty_and_dead', 'modelnet'])
def test_weight_gradients_match_torch_autograd_over_the_composed_path(case):
    if case == 'modelnet':
        model, _ = _model(synthetic.model_cfg('modelnet'), seed=4)
        x = torch.from_numpy(synthetic.make_batch('modelnet', 1, 1024, first_pair=8))
    else:
        model, _ = _model(small_cfg(), seed=4)
        x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=9))
    sa = model._cloud_layers[0]._sa0
    if case == 'empty_and_dead':
        # radius 0: every ball is empty (all slots read point 0); 0.5: partly filled balls padded with the first hit;
        # channels 3 and 37 pushed below zero everywhere: their maximum is 0 and they pass no gradient
        sa.radii = [0.0, 0.5]
        with torch.no_grad():
            sa.mlps[0].layer2.conv.bias[3] = -1e3
            sa.mlps[1].layer2.conv.bias[5] = -1e3
    xyz, feats = _split(x)
    g = torch.randn(xyz.shape[0], sa.out_features(), sa.npoint, generator=torch.Generator().manual_seed(1)).to(DEV)
    sa.fused_training = True
    out_f, got = _grads(sa, xyz, feats, g, True)
    out_c, want = _grads(sa, xyz, feats, g, False)
    _close(out_f, out_c)
    names = [n for n, _ in sa.named_parameters()]
    _check_grads(got, want, names)
    if case == 'empty_and_dead':
        assert float(out_f[:, 3].abs().max()) == 0.0 and float(out_f[:, 37].abs().max()) == 0.0
        assert float(got[5][3].abs().max()) == 0.0 and float(got[11][5].abs().max()) == 0.0
        assert all(bool(torch.isfinite(t).all()) for t in got)


def test_two_backward_passes_give_bit_identical_gradients():
    model, _ = _model(synthetic.model_cfg('kitti'), seed=5)
    sa = model._cloud_layers[0]._sa0
    sa.fused_training = True
    xyz, feats = _split(torch.from_numpy(synthetic.make_batch('kitti', 2, 4096, first_pair=3)))
    g = torch.randn(xyz.shape[0], 64, sa.npoint, generator=torch.Generator().manual_seed(2)).to(DEV)
    _, first = _grads(sa, xyz, feats, g, True)
    _, second = _grads(sa, xyz, feats, g, True)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert any(float(a.abs().max()) > 0 for a in first)


def _labels(first, pairs):
    return torch.from_numpy(np.stack([LabelType.POSE3D_DUAL_QUAT.from_matrix(synthetic.kitti_like_pair(first + i, 16)[2])
                                      for i in range(pairs)]).astype(np.float32))


def _augmentation(n_clouds, seed):
    rng = np.random.default_rng(seed)
    m = np.tile(np.eye(4, dtype=np.float32), (n_clouds, 1, 1))
    for i in range(n_clouds):
        a = rng.uniform(-0.1, 0.1)
        m[i, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        m[i, :3, 3] = rng.uniform(-0.5, 0.5, size=3)
    return torch.from_numpy(m)


def test_full_training_step_matches_the_oracle_autograd():
    cfg = small_cfg()
    model, sd = _model(cfg, seed=23, loss=True)
    assert model.set_fused_training() == ['_cloud_layers.0._sa0']
    model.train()
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=41))
    m = _augmentation(4, seed=3)
    labels = _labels(41, 2)
    x_aug = x.to(DEV)
    type(model)._augment(x_aug, m.to(DEV))                         # what forward(x, m=m) does in place, on the device
    x_aug = x_aug.cpu()
    y_pred, loss, _ = model(x.to(DEV), m=m.to(DEV), y=labels.to(DEV))
    loss.backward()
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    orc = oracle.build_oracle_model(cfg, sd)
    orc.sd = sd_o
    y_o = orc.pose_head(orc.flow_embedding(orc.cloud_features(x_aug)))
    loss_o = model._loss_layer.cpu()(y_o, labels)
    loss_o.backward()
    _close(y_pred, y_o)
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
    params = dict(model.named_parameters())
    for key, ref in sd_o.items():
        got = params[key].grad
        assert got is not None and ref.grad is not None, key
        scale = float(ref.grad.abs().max())
        assert float((got.cpu() - ref.grad).abs().max()) <= 2e-4 * max(scale, 1e-6), key


@pytest.mark.parametrize('cfg_fn', [small_two_level_cfg, small_transform_cfg])
def test_training_step_with_a_fused_first_level_equals_the_composed_step(cfg_fn):
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=11))
    m = _augmentation(4, seed=5)
    labels = _labels(11, 2).to(DEV)
    runs = []
    for fused in (False, True):
        model, _ = _model(cfg_fn(), seed=29, loss=True)
        assert model.set_fused_training(fused) == (['_cloud_layers.0._sa0'] if fused else [])
        model.train()
        y, loss, _ = model(x.clone().to(DEV), m=m.to(DEV), y=labels)
        loss.backward()
        runs.append((y.detach(), float(loss), {n: p.grad.detach().clone() for n, p in model.named_parameters()
                                               if p.grad is not None}))
    (y_c, loss_c, g_c), (y_f, loss_f, g_f) = runs
    _close(y_f, y_c)
    assert abs(loss_f - loss_c) <= 1e-5 * max(1.0, abs(loss_c))
    assert set(g_f) == set(g_c)
    for name in g_c:
        scale = float(g_c[name].abs().max())
        assert float((g_f[name] - g_c[name]).abs().max()) <= 2e-4 * max(scale, 1e-6), name


def test_sgd_steps_fused_and_composed_agree_and_eval_sees_the_updated_weights():
    cfg = small_cfg()
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=13))
    labels = _labels(13, 2).to(DEV)
    losses, models = [], []
    for fused in (False, True):
        model, _ = _model(small_cfg(), seed=31, loss=True)
        model.set_fused_training(fused)
        model.train()
        opt = torch.optim.SGD([p for n, p in model.named_parameters() if not n.startswith('_loss_layer')], lr=1e-4)
        run = []
        for _ in range(10):
            opt.zero_grad()
            _, loss, _ = model(x.clone().to(DEV), y=labels)
            loss.backward()
            opt.step()
            run.append(float(loss))
        losses.append(run)
        models.append(model)
    for a, b in zip(*losses):
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-6), losses
    assert losses[1][-1] != losses[1][0]                           # the steps did move the weights
    model = models[1].eval()
    sd_after = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith('_loss_layer')}
    with torch.no_grad():
        y, _, _ = model(x.to(DEV))
    _close(y, oracle.build_oracle_model(cfg, sd_after)(x))


def test_fused_sa_training_memory_is_a_small_fraction_of_the_composed_path():
    model, _ = _model(synthetic.model_cfg('kitti'), seed=7)
    sa = model._cloud_layers[0]._sa0
    sa.fused_training = True
    xyz, feats = _split(_dense_clouds(4, 16384, seed=9))
    g = torch.randn(4, 64, sa.npoint, generator=torch.Generator().manual_seed(3)).to(DEV)

    def peak(fused):
        for p in sa.parameters():
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = sa._forward_fused_train(xyz, feats)[1] if fused else sa._forward_composed(xyz, feats, train=True)[1]
        out.backward(g)
        del out
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak(True)                                                     # parameter .grad tensors now exist in both runs
    fused = peak(True)
    composed = peak(False)
    bq = 4 * 1024 * (512 + 1024) * 4
    assert fused <= bq + (16 << 20), fused
    assert composed >= 20 * fused, (composed, fused)
    print("SA forward + backward, 4 clouds x 16384 points: peak above baseline fused %.1f MB, composed %.1f MB"
          % (fused / 2 ** 20, composed / 2 ** 20))
