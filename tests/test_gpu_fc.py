"""GPU: the small-row fully connected kernel (dclr_fc) against a float64 act(x @ w.T + b), at the shapes where it changes
course -- one row block or several per workgroup (gridDim.y stops at 64 blocks of 8 rows: m > 512 loops), partial row
blocks, column groups of 4 waves with dead waves, k below / at / above one 64-lane step and one 1024-column chunk (wider
rows run in chunks), the 16-byte staging and the scalar staging of an unaligned x or k % 4 != 0 -- and every output
activation (0 none, 1 relu, 2 dual quaternion, 3 quaternion) with pre-activations of up to +-100, so that sigmoid and tanh
saturate."""
import numpy as np
import pytest
import torch

from deepclr_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

MS = (1, 7, 8, 9, 64, 511, 512, 513, 1100)
NS = (1, 3, 4, 6, 7, 8, 9, 65)
KS = (1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2048, 2051, 3072)


def _ref(x: np.ndarray, w: np.ndarray, b, act: int):
    """float64 pre-activation, its bound sum |w_i x_i| + |b|, and the activation (the columns of act 2 / 3 as
    OutputSimple._act and the reference's _output_activation take them)."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    pre = x64 @ w64.T
    mag = np.abs(x64) @ np.abs(w64).T
    if b is not None:
        pre = pre + b.astype(np.float64)
        mag = mag + np.abs(b.astype(np.float64))
    y = pre.copy()
    col = np.arange(pre.shape[1])
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))                       # noqa: E731
    if act == 1:
        y = np.maximum(pre, 0.0)
    elif act == 2:
        y[:, col == 0] = sig(pre[:, col == 0])
        y[:, (col >= 1) & (col < 4)] = np.tanh(pre[:, (col >= 1) & (col < 4)])
    elif act == 3:
        y[:, col == 3] = sig(pre[:, col == 3])
        y[:, col > 3] = np.tanh(pre[:, col > 3])
    return y, mag


def _check(got: torch.Tensor, x, w, b, act, what):
    got = got.cpu().numpy().astype(np.float64)
    want, mag = _ref(x, w, b, act)
    assert got.shape == want.shape, what
    assert np.isfinite(got).all(), what + ': non-finite outputs'
    # float32 accumulation: <= 2e-6 of the magnitude sum; the transcendental activations add two ulps of their output
    tol = 2e-6 * mag + 1e-7 + (2.4e-7 * np.abs(want) if act in (2, 3) else 0.0)
    err = np.abs(got - want)
    bad = np.argwhere(err > tol)
    assert not len(bad), '{}: {} outputs off, first at {} ({} vs {}, tol {:.3g})'.format(
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], tol[tuple(bad[0])])
    col = np.arange(got.shape[1])
    if act == 2:
        assert (got[:, col == 0] >= 0).all() and (got[:, col == 0] <= 1).all(), what
        assert (np.abs(got[:, (col >= 1) & (col < 4)]) <= 1).all(), what
    elif act == 3:
        assert (got[:, col == 3] >= 0).all() and (got[:, col == 3] <= 1).all(), what
        assert (np.abs(got[:, col > 3]) <= 1).all(), what
    elif act == 1:
        assert (got >= 0).all(), what


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('m', MS)
def test_fc_matches_float64_reference(m, k):
    """Every (m, n, k) of the grid; per shape all four activations, with and without bias, x aligned (16-byte staging when
    k % 4 == 0) and x one float into its allocation (scalar staging)."""
    rng = np.random.default_rng(1000 * m + k)
    n_max = max(NS)
    x = rng.uniform(-1.0, 1.0, size=(m, k)).astype(np.float32)
    w_all = (rng.uniform(-1.0, 1.0, size=(n_max, k)) * (100.0 / np.sqrt(k))).astype(np.float32)   # |pre| up to ~100
    b_all = rng.uniform(-5.0, 5.0, size=n_max).astype(np.float32)
    x_dev = torch.from_numpy(x).to(DEV)
    buf = torch.empty(m * k + 1, dtype=torch.float32, device=DEV)
    x_off = buf[1:].view(m, k)
    x_off.copy_(x_dev)
    assert x_off.data_ptr() % 16 != 0 and x_off.is_contiguous()
    for n in NS:
        w, b = np.ascontiguousarray(w_all[:n]), b_all[:n].copy()
        w_dev, b_dev = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
        for act in range(4):
            for xi, xd in enumerate((x_dev, x_off)):
                with_bias = (act + xi + n) % 2 == 0
                got = ops.fc(xd, w_dev, b_dev if with_bias else None, act)
                _check(got, x, w, b if with_bias else None, act,
                       'm={} n={} k={} act={} {} {}'.format(m, n, k, act, 'offset x' if xi else 'aligned x',
                                                           'bias' if with_bias else 'no bias'))
    torch.cuda.synchronize()


def test_fc_wide_rows_at_k_1024_are_one_chunk():
    """The chunked loop over k keeps one lane's fmaf order: a row of 2048 columns whose second half is zero gives, bit for
    bit, what its first 1024 columns give alone (same weights, same accumulation order; the second chunk adds exact
    zeros)."""
    rng = np.random.default_rng(7)
    m, n = 19, 9
    x = torch.from_numpy(rng.uniform(-1, 1, size=(m, 1024)).astype(np.float32)).to(DEV)
    w = torch.from_numpy(rng.uniform(-1, 1, size=(n, 1024)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.uniform(-1, 1, size=n).astype(np.float32)).to(DEV)
    x2 = torch.cat((x, torch.zeros_like(x)), dim=1).contiguous()
    w2 = torch.cat((w, torch.from_numpy(rng.uniform(-1, 1, size=(n, 1024)).astype(np.float32)).to(DEV)), dim=1).contiguous()
    for act in range(4):
        assert torch.equal(ops.fc(x, w, b, act), ops.fc(x2, w2, b, act)), act


def test_fc_refuses_bad_arguments():
    x = torch.ones(4, 8, device=DEV)
    w = torch.ones(3, 8, device=DEV)
    for act in (4, -1):
        with pytest.raises(RuntimeError):
            ops.fc(x, w, None, act)
    with pytest.raises(RuntimeError):                                   # no rows
        ops.fc(torch.ones(0, 8, device=DEV), w, None, 0)
    with pytest.raises(RuntimeError):                                   # no columns
        ops.fc(torch.ones(4, 0, device=DEV), torch.ones(3, 0, device=DEV), None, 0)
    with pytest.raises(RuntimeError):                                   # no outputs
        ops.fc(x, torch.ones(0, 8, device=DEV), None, 0)
    with pytest.raises(RuntimeError):                                   # w of another width
        ops.fc(x, torch.ones(3, 9, device=DEV), None, 0)
    with pytest.raises(RuntimeError):                                   # bias of another length
        ops.fc(x, w, torch.ones(4, device=DEV), 0)
    torch.cuda.synchronize()


# ---- a head whose conv stack ends wider than one fc chunk ------------------------------------------------------------
def _wide_head_model():
    """small_cfg with 512 centroids and the head's conv stack ending at 2048 channels (linear [2048, 256]): the first fc
    layer reads 2048 columns. 8 pairs of 1024 points = 4096 head rows, so both matrix paths take the one-call route."""
    import oracle
    from deepclr_amd import synthetic
    from deepclr_amd.config import model_config_from_dict
    from deepclr_amd.models import build_model
    from helpers import small_cfg
    cfg = small_cfg()
    cfg['params']['cloud_features']['params']['npoint'] = [512]
    cfg['params']['output']['params'].update(mlp=[256, 512, 2048], linear=[2048, 256])
    sd = synthetic.random_state_dict(cfg, seed=31)
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(sd, strict=True)
    x = torch.from_numpy(synthetic.make_batch('kitti', 8, 1024, first_pair=51))
    return model.to(DEV).eval(), oracle.build_oracle_model(cfg, sd), x


def _close(got, want, what):
    got, want = got.detach().cpu(), torch.as_tensor(want)
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * scale), '{}: off by {:.3g}'.format(what, err)


@pytest.mark.parametrize('precision', ['f32', 'f16x2'])
def test_head_wider_than_1024_channels_against_the_oracle(precision):
    """forward() (first, range-checked call and the next one), the row API, the one-call cloud_merge_prep and the
    per-layer head (2 pairs: below the f32 fused head's 4096 rows) against the CPU oracle, on both matrix paths."""
    model, orc, x = _wide_head_model()
    want = orc(x)
    xd = x.to(DEV)
    saved, ops.PRECISION = ops.PRECISION, precision
    try:
        with torch.no_grad():
            outs = {'forward (first)': model(xd.clone())[0], 'forward': model(xd.clone())[0]}
            rows = model.cloud_feature_rows(xd)
            plan = model._merge_plan(rows, 8)
            assert plan is not None and plan.args.fc_k[0] == 2048, 'the one-call path must take this head'
            outs['merge_rows'] = model.merge_rows(rows, 8)
            got = model.cloud_merge_prep(xd)
            if got is None:                                     # the one-call sampling path does not apply: the two methods
                rows = model.cloud_feature_rows(xd)
                got = rows, model.merge_prep(rows, 8)
            outs['cloud_merge_prep'] = model.merge_rows(got[0], 8, prep=got[1])
            two = model(xd[[0, 1, 8, 9]].contiguous())[0]         # pairs 0 and 1 alone
        torch.cuda.synchronize()
    finally:
        ops.PRECISION = saved
    for what, y in outs.items():
        _close(y, want, precision + ': ' + what)
    _close(two, want[:2], precision + ': forward, 2 pairs')


def test_merge_forward_refuses_bad_fc_layers_before_any_launch():
    """The C ABI's promise (include/deepclr_amd.h): DCLR_E_* means nothing was enqueued. A one-call plan whose fc layers
    are made invalid (input width not the previous output width, an unknown activation, no outputs) must be refused with
    its workspace -- layer-1 halves, flow-embedding rows, column maxima -- and y untouched."""
    model, _, x = _wide_head_model()
    saved, ops.PRECISION = ops.PRECISION, 'f32'
    try:
        with torch.no_grad():
            xd = x.to(DEV)
            model(xd)
            rows = model.cloud_feature_rows(xd)
            plan = model._merge_plan(rows, 8)
            assert plan is not None
            a, ws = plan.args, plan._keep['ws']
            last = a.n_fc - 1
            for field, idx, bad in (('fc_k', 0, 2047), ('fc_k', 1, 255), ('fc_act', last, 4), ('fc_n', 0, 0)):
                arr = getattr(a, field)
                good = arr[idx]
                for t in (ws['pt'], ws['e'], ws['colmax']):
                    t.fill_(float('nan'))
                y = torch.full((8, 8), -7.0, device=DEV)
                arr[idx] = bad
                try:
                    with pytest.raises(RuntimeError):
                        plan.run(rows, out=y)
                finally:
                    arr[idx] = good
                torch.cuda.synchronize()
                what = '{}[{}] = {}'.format(field, idx, bad)
                assert bool((y == -7.0).all()), what + ': y written'
                for key in ('pt', 'e', 'colmax'):
                    assert bool(torch.isnan(ws[key]).all()), what + ': ' + key + ' written before the refusal'
            y = plan.run(rows)                                  # and the restored plan runs
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all())
    finally:
        ops.PRECISION = saved
