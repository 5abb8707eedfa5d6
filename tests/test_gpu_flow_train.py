"""GPU: the fused training form of the flow embedding (csrc/flow_train.hip, libdeepclr_amd_flow_train.so) against the
composed training path (MotionEmbeddingBase.forward_train: torch autograd over the grouped tensor), a tie-free torch
reference at the fused argmax, and the CPU oracle's autograd; determinism, optimizer steps, memory."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

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
    return model.to(DEV).train(), sd


def _embedding(cfg, seed=3, k=None, radius=None):
    model, _ = _model(cfg, seed)
    emb = model._merge_layers[0]._embedding
    if k is not None:
        emb._k = k
        emb._fused_shape = 1 <= k <= 32
    if radius is not None:
        emb._radius = float(radius)
    return emb


def _clouds(pairs, n, seed, spread=4.0, dup=1):
    """(B, 67, n) template and source feature clouds as the set abstraction hands them on: xyz in a box, non-negative
    features. dup > 1: every source point repeated dup times over a smaller set (many templates share neighbours)."""
    g = torch.Generator().manual_seed(seed)
    c0 = torch.rand(pairs, 67, n, generator=g)
    c0[:, :3] = (c0[:, :3] - 0.5) * spread
    m = n // dup
    c1 = torch.rand(pairs, 67, m, generator=g)
    c1[:, :3] = (c1[:, :3] - 0.5) * spread
    c1 = c1.repeat(1, 1, dup)[:, :, :n] + 0.0
    c1[:, :3] += 1e-3 * torch.arange(n).float().view(1, 1, n) / n          # distinct coordinates: no exact ties
    return c0.to(DEV), c1.to(DEV)


def _close(got, want, rtol=1e-5, atol=1e-6):
    want = want.detach().cpu()
    scale = max(1.0, float(want.abs().max()))
    torch.testing.assert_close(got.detach().cpu(), want, rtol=rtol, atol=atol * scale)


def _grad_close(a, b, name):
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= 2e-4 * max(scale, 1e-6), (name, err, scale)


def _activations(emb, c0, c1, idx):
    """The composed activations h (B, 256, P0, k) after the radius mask, differentiable in the clouds and weights."""
    b, _, p0 = c0.shape
    k = idx.shape[2]
    gi = idx.long().view(b, 1, p0 * k).expand(-1, c1.shape[1], -1)
    grouped = torch.gather(c1, 2, gi).view(b, c1.shape[1], p0, k)
    pos_diff = grouped[:, :3] - c0[:, :3, :].unsqueeze(-1)
    h = torch.cat((pos_diff, c0[:, 3:, :].unsqueeze(-1).expand(-1, -1, -1, k), grouped[:, 3:]), dim=1)
    h = h.reshape(b, h.shape[1], p0 * k)
    for layer in emb._conv.layers():
        conv = layer._sequential[0]
        h = F.relu(F.conv1d(h, conv.weight, conv.bias))
    h = h.view(b, -1, p0, k)
    if emb._radius > 0.0:
        h = h.masked_fill((torch.norm(pos_diff, dim=1) >= emb._radius).unsqueeze(1), 0.0)
    return h


def _fused_forward(emb, c0, c1):
    idx = emb._knn_slots(c0, c1)
    weights = ops.pack_flow_train_mlp(list(emb._conv.parameters()))
    pooled, arg, _, _ = ops.flow_train_forward(c0.transpose(1, 2).contiguous(), c1.transpose(1, 2).contiguous(), idx,
                                               weights, emb._radius)
    return idx, pooled, arg


@pytest.mark.parametrize('case', ['small', 'kitti', 'modelnet', 'k32', 'k1'])
def test_forward_matches_the_composed_path_and_the_argmax_holds_the_maximum(case):
    cfg = {'small': small_cfg, 'kitti': lambda: synthetic.model_cfg('kitti'), 'k32': small_cfg, 'k1': small_cfg,
           'modelnet': lambda: synthetic.model_cfg('modelnet')}[case]()
    emb = _embedding(cfg, k={'k32': 32, 'k1': 1}.get(case))
    assert emb._k == {'small': 8, 'kitti': 20, 'modelnet': 30, 'k32': 32, 'k1': 1}[case]
    c0, c1 = _clouds(2, 1024 if case in ('kitti', 'modelnet') else 256, seed=5)
    emb.fused_training = True
    assert emb.fused_training_applies(c0, c1)
    got = emb.forward_train(c0, c1).detach()                          # gradients on: the fused path
    with torch.no_grad():
        emb.fused_training = False
        want = emb.forward_train(c0, c1)
        idx, pooled, arg = _fused_forward(emb, c0, c1)
        h = _activations(emb, c0, c1, idx)
    assert got.shape == want.shape == (2, 259, c0.shape[2])
    _close(got, want)
    assert torch.equal(got[:, 3:], pooled)
    assert int(arg.min()) >= 0 and int(arg.max()) < emb._k
    at_arg = h.gather(3, arg.long().unsqueeze(-1)).squeeze(-1)
    _close(at_arg, h.max(dim=3)[0])
    assert float((pooled > 0).float().mean()) > 0.05                  # a real test: many channels are live


def _tie_free_grads(emb, c0, c1, idx, arg, g):
    a0, a1 = c0.detach().clone().requires_grad_(True), c1.detach().clone().requires_grad_(True)
    params = list(emb._conv.parameters())
    for p in params:
        p.grad = None
    h = _activations(emb, a0, a1, idx)
    out = torch.cat((a0[:, :3, :], h.gather(3, arg.long().unsqueeze(-1)).squeeze(-1)), dim=1)
    (out * g).sum().backward()
    return out.detach(), [p.grad.clone() for p in params], a0.grad, a1.grad


def _fused_grads(emb, c0, c1, g):
    a0, a1 = c0.detach().clone().requires_grad_(True), c1.detach().clone().requires_grad_(True)
    params = list(emb._conv.parameters())
    for p in params:
        p.grad = None
    emb.fused_training = True
    out = emb.forward_train(a0, a1)
    (out * g).sum().backward()
    return out.detach(), [p.grad.clone() for p in params], a0.grad, a1.grad


@pytest.mark.parametrize('case', ['radius0', 'all_masked', 'dead_channel', 'shared_neighbours', 'kitti'])
def test_gradients_match_a_tie_free_torch_reference_at_the_fused_argmax(case):
    cfg = synthetic.model_cfg('kitti') if case == 'kitti' else small_cfg()
    emb = _embedding(cfg, seed=4, radius={'radius0': 0.0, 'all_masked': 1e-6}.get(case))
    if case == 'dead_channel':
        with torch.no_grad():
            list(emb._conv.layers())[-1]._sequential[0].bias[7] = -1e3
    n = 1024 if case == 'kitti' else 256
    c0, c1 = _clouds(2, n, seed=9, spread=1.0 if case == 'shared_neighbours' else 4.0,
                     dup=4 if case == 'shared_neighbours' else 1)
    g = torch.randn(2, 259, n, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        idx, pooled, arg = _fused_forward(emb, c0, c1)
    out_f, gw_f, g0_f, g1_f = _fused_grads(emb, c0, c1, g)
    out_r, gw_r, g0_r, g1_r = _tie_free_grads(emb, c0, c1, idx, arg, g)
    _close(out_f, out_r)
    names = [nm for nm, _ in emb._conv.named_parameters()]
    for name, a, b in zip(names, gw_f, gw_r):
        _grad_close(a, b, name)
    _grad_close(g0_f, g0_r, 'clouds0')
    _grad_close(g1_f, g1_r, 'clouds1')
    _grad_close(g0_f[:, :3], g0_r[:, :3], 'clouds0 xyz')
    _grad_close(g1_f[:, :3], g1_r[:, :3], 'clouds1 xyz')
    assert all(bool(torch.isfinite(t).all()) for t in gw_f + [g0_f, g1_f])
    if case == 'all_masked':
        assert float(out_f[:, 3:].abs().max()) == 0.0
        assert all(float(t.abs().max()) == 0.0 for t in gw_f)
        assert float(g1_f.abs().max()) == 0.0
        assert torch.equal(g0_f[:, :3], g[:, :3]) and float(g0_f[:, 3:].abs().max()) == 0.0
    if case == 'dead_channel':
        assert float(out_f[:, 3 + 7].abs().max()) == 0.0 and float(gw_f[5][7].abs().max()) == 0.0
    if case == 'shared_neighbours':
        counts = torch.bincount(idx.long().flatten() + 0, minlength=n)
        assert int(counts.max()) >= 8                                   # the scatter sums many (p, j) per source point


@pytest.mark.parametrize('cfg_fn', [small_cfg, lambda: synthetic.model_cfg('kitti'),
                                    lambda: synthetic.model_cfg('modelnet')])
def test_weight_gradients_match_the_plain_composed_backward(cfg_fn):
    emb = _embedding(cfg_fn(), seed=6)
    c0, c1 = _clouds(2, 512, seed=12)
    g = torch.randn(2, 259, 512, generator=torch.Generator().manual_seed(3)).to(DEV)
    _, got, _, _ = _fused_grads(emb, c0, c1, g)
    for p in emb._conv.parameters():
        p.grad = None
    emb.fused_training = False
    (emb.forward_train(c0, c1) * g).sum().backward()
    for (name, p), a in zip(emb._conv.named_parameters(), got):
        _grad_close(a, p.grad, name)


def _labels(first, pairs):
    return torch.from_numpy(np.stack([LabelType.POSE3D_DUAL_QUAT.from_matrix(synthetic.kitti_like_pair(first + i, 16)[2])
                                      for i in range(pairs)]).astype(np.float32))


def test_full_training_step_matches_the_oracle_autograd():
    cfg = small_cfg()
    model, sd = _model(cfg, seed=23, loss=True)
    assert model.set_fused_training(True, merge=True) == ['_cloud_layers.0._sa0', '_merge_layers.0']
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=41))
    labels = _labels(41, 2)
    y_pred, loss, _ = model(x.to(DEV), y=labels.to(DEV))
    loss.backward()
    sd_o = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    orc = oracle.build_oracle_model(cfg, sd)
    orc.sd = sd_o
    y_o = orc.pose_head(orc.flow_embedding(orc.cloud_features(x)))
    loss_o = model._loss_layer.cpu()(y_o, labels)
    loss_o.backward()
    _close(y_pred, y_o)
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
    params = dict(model.named_parameters())
    for key, ref in sd_o.items():
        got = params[key].grad
        assert got is not None and ref.grad is not None, key
        _grad_close(got.cpu(), ref.grad, key)


@pytest.mark.parametrize('cfg_fn', [small_cfg, small_two_level_cfg, small_transform_cfg])
def test_is_feat_input_gradient_matches_the_composed_step(cfg_fn):
    cfg = cfg_fn()
    x_cpu = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=17))
    labels = _labels(17, 2).to(DEV)
    runs = []
    for merge in (False, True):
        model, _ = _model(cfg_fn(), seed=37, loss=True)
        model.set_fused_training(merge, merge=merge)
        with torch.no_grad():
            feat = model.cloud_features(x_cpu.to(DEV))
        feat = feat.detach().clone().requires_grad_(True)
        y, loss, _ = model(feat, is_feat=True, y=labels)
        loss.backward()
        runs.append((y.detach(), feat.grad.detach().clone(),
                     {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (y_c, x_c, g_c), (y_f, x_f, g_f) = runs
    _close(y_f, y_c)
    _grad_close(x_f, x_c, 'x.grad')
    assert float(x_c.abs().max()) > 0
    for name in g_c:
        _grad_close(g_f[name], g_c[name], name)
    del cfg


def test_two_backward_passes_give_bit_identical_gradients():
    emb = _embedding(synthetic.model_cfg('kitti'), seed=5)
    c0, c1 = _clouds(3, 1024, seed=21, spread=1.5, dup=2)
    g = torch.randn(3, 259, 1024, generator=torch.Generator().manual_seed(2)).to(DEV)
    first = _fused_grads(emb, c0, c1, g)
    second = _fused_grads(emb, c0, c1, g)
    for a, b in zip(first[1] + [first[2], first[3]], second[1] + [second[2], second[3]]):
        assert torch.equal(a, b)
    assert all(float(a.abs().max()) > 0 for a in first[1][:2] + [first[3]])


def test_sgd_steps_fused_and_composed_agree_and_eval_sees_the_updated_weights():
    cfg = small_cfg()
    x = torch.from_numpy(synthetic.make_batch('kitti', 2, 512, first_pair=13))
    labels = _labels(13, 2).to(DEV)
    losses, models = [], []
    for fused in (False, True):
        model, _ = _model(small_cfg(), seed=31, loss=True)
        model.set_fused_training(fused, merge=fused)
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
    assert losses[1][-1] != losses[1][0]
    model = models[1].eval()
    sd_after = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith('_loss_layer')}
    with torch.no_grad():
        y, _, _ = model(x.to(DEV))
    _close(y, oracle.build_oracle_model(cfg, sd_after)(x))


def test_fused_flow_training_memory_is_a_fraction_of_the_composed_path():
    emb = _embedding(synthetic.model_cfg('kitti'), seed=7)
    assert emb._k == 20
    c0, c1 = _clouds(4, 1024, seed=19)
    a0, a1 = c0.clone().requires_grad_(True), c1.clone().requires_grad_(True)
    g = torch.randn(4, 259, 1024, generator=torch.Generator().manual_seed(3)).to(DEV)

    def peak(fused):
        emb.fused_training = fused
        for p in list(emb._conv.parameters()) + [a0, a1]:
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = emb.forward_train(a0, a1)
        out.backward(g)
        del out
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    peak(True)                                                         # .grad tensors now exist in every run
    fused = peak(True)
    composed = peak(False)
    print("flow embedding forward + backward, 4 pairs x 1024 points, k = 20: peak above baseline fused %.1f MB, "
          "composed %.1f MB (%.1fx)" % (fused / 2 ** 20, composed / 2 ** 20, composed / fused))
    assert fused <= 128 << 20, fused
    assert composed >= 2 * fused, (composed, fused)
