"""CPU: the ragged (different cloud sizes) entry points -- symbols, argument checks before any launch, the DclrCloudRef
record, the size classes, and the host-side validation of cloud lists."""
import ctypes
import os
import subprocess

import pytest
import torch

from deepclr_amd import build, lib, ops, synthetic
from deepclr_amd.config import model_config_from_dict
from deepclr_amd.models import build_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUP = -1, -2
RAGGED = ('dclr_fps_clouds_grouped_ragged', 'dclr_sa_msg_fused_ragged')


def test_ragged_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'deepclr_amd.h')).read()
    handle = ctypes.CDLL(build.LIB)
    for name in RAGGED:
        assert name + '(' in header and name in lib.SIGNATURES and hasattr(handle, name), name


def _fake(addr=0x100000):
    return ctypes.c_void_p(addr)                  # never dereferenced: every call below is rejected before a launch


def test_ragged_sampler_rejects_bad_arguments_without_a_gpu():
    f = lib.load().dclr_fps_clouds_grouped_ragged
    p = _fake()
    ok = dict(b=2, n_max=4096, c=4, m=64, refs=p, idx=p, gpts=p, gbox=p, sbox=None, ws=None, wsb=0)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['b'], a['n_max'], a['c'], a['m'], a['refs'], a['idx'], a['gpts'], a['gbox'], a['sbox'], a['ws'], a['wsb'],
                 None)
    for bad in ('refs', 'idx', 'gpts', 'gbox'):
        assert call(**{bad: None}) == INVAL, bad
    assert call(b=0) == INVAL and call(m=0) == INVAL and call(c=2) == INVAL
    assert call(refs=_fake(0x100004)) == INVAL                     # records are 8-byte aligned
    assert call(gpts=_fake(0x100008)) == INVAL                     # group points are float4
    assert call(n_max=1000) == UNSUP and call(n_max=1024) == UNSUP and call(n_max=70000) == UNSUP
    assert call(n_max=2048, sbox=p) == UNSUP                       # groups of one slice: no slice boxes
    assert call(m=20000) == UNSUP                                  # picked[] beyond LDS
    # 16384 < n_max: the workspace sampler -- a workspace of b * class * 10 bytes, no slice boxes, m <= 8192
    need = 2 * 65536 * 10
    assert call(n_max=50000) == INVAL                              # no workspace
    assert call(n_max=50000, ws=p, wsb=need - 1) == INVAL          # a short one
    assert call(n_max=50000, ws=_fake(0x100008), wsb=need) == INVAL   # misaligned
    assert call(n_max=50000, ws=p, wsb=need, sbox=p) == UNSUP
    assert call(n_max=50000, ws=p, wsb=need, m=9000) == UNSUP


def test_ragged_set_abstraction_rejects_bad_arguments_without_a_gpu():
    f = lib.load().dclr_sa_msg_fused_ragged
    p = _fake()
    radii = (ctypes.c_float * 2)(1.0, 2.0)
    ns = (ctypes.c_int * 2)(8, 16)
    mlp = (ctypes.c_void_p * 2)(0x100000, 0x100000)
    r, s, m = (ctypes.cast(a, ctypes.c_void_p) for a in (radii, ns, mlp))
    ok = dict(b=2, n_max=4096, c=4, npoint=64, refs=p, idx=p, scales=2, out=p, gpts=p, gbox=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(1, a['b'], a['n_max'], a['c'], a['npoint'], a['refs'], a['idx'], a['scales'], r, s, m, a['out'], None,
                 a['gpts'], a['gbox'], None, None, None)
    for bad in ('refs', 'idx', 'out', 'gpts', 'gbox'):
        assert call(**{bad: None}) == INVAL, bad
    assert call(b=0) == INVAL and call(b=70000) == INVAL and call(npoint=0) == INVAL
    assert call(refs=_fake(0x100004)) == INVAL
    assert call(n_max=1000) == UNSUP and call(n_max=70000) == UNSUP
    assert call(c=5) == UNSUP and call(scales=3) == UNSUP


def test_cloud_ref_matches_its_ctypes_mirror(tmp_path):
    src = tmp_path / 'ref.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "deepclr_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(DclrCloudRef), offsetof(DclrCloudRef, pts), '
                   'offsetof(DclrCloudRef, n), offsetof(DclrCloudRef, reserved)); return 0; }\n')
    exe = tmp_path / 'ref'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    r = lib.CloudRef
    assert got == [16, 0, 8, 12] == [ctypes.sizeof(r), r.pts.offset, r.n.offset, r.reserved.offset]


@pytest.mark.parametrize('edge', [1024, 2048, 4096, 8192, 16384, 32768, 65536])
def test_size_classes_follow_the_group_layout(edge):
    """Two clouds share a ragged launch exactly when the library gives them the same group layout (one kernel instance),
    and a class's buffers (its layout) hold every cloud of it."""
    for n in (edge, edge + 1):
        cls, layout = ops.ragged_class(n), ops.fps_group_layout(n)
        assert (cls is None) == (layout is None), n
        if cls is not None:
            assert cls // 2 < n <= cls and ops.fps_group_layout(cls) == layout and layout[0] * layout[1] == cls, n
            assert ops.ragged_class(n, npoint=1 << 14) == (None if n > 16384 else cls)   # picked[] in LDS bounds npoint
    assert ops.ragged_class(edge) != ops.ragged_class(edge + 1)
    assert ops.fps_group_layout(edge) != ops.fps_group_layout(edge + 1)


def _model():
    cfg = synthetic.model_cfg('kitti')
    model = build_model(model_config_from_dict(cfg))
    model.load_state_dict(synthetic.random_state_dict(cfg, seed=0))
    return model.eval()


@pytest.mark.parametrize('bad, err', [
    ([], ValueError),
    ((), ValueError),
    ([torch.zeros(3000, 4), torch.zeros(2000, 4)], RuntimeError),                # CPU tensors
    ([torch.zeros(2, 3000, 4)], ValueError),                                      # not (N, C)
    ([torch.zeros(3000)], ValueError),                                            # 1-D
])
def test_malformed_cloud_lists_raise_before_any_device_call(bad, err, monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(ops, '_call', no_device)
    model = _model()
    with pytest.raises(err):
        ops.check_cloud_list(bad)
    with pytest.raises(err):
        model.cloud_features(bad)
    with pytest.raises(err):
        ops.cloud_rows_ragged(bad, 64, [1.0], [8], [torch.zeros(1)])


def test_mixed_columns_dtype_and_empty_clouds_are_refused_on_the_host(monkeypatch):
    """The same checks for what only a GPU tensor could carry, on tensors that merely claim to be on one."""
    class Fake:
        def __init__(self, n, c, dtype=torch.float32, device='cuda:0', dim=2):
            self.shape, self.dtype, self.device, self.is_cuda = (n, c) if dim == 2 else (n,), dtype, torch.device(device), True
            self._dim = dim

        def dim(self):
            return self._dim
    orig = torch.is_tensor
    monkeypatch.setattr(torch, 'is_tensor', lambda x: isinstance(x, Fake) or orig(x))
    with pytest.raises(ValueError, match='columns'):
        ops.check_cloud_list([Fake(3000, 4), Fake(2000, 3)])
    with pytest.raises(ValueError, match='columns'):
        ops.check_cloud_list([Fake(3000, 2)])
    with pytest.raises(RuntimeError, match='float32'):
        ops.check_cloud_list([Fake(3000, 4), Fake(2000, 4, dtype=torch.float64)])
    with pytest.raises(ValueError, match='no points'):
        ops.check_cloud_list([Fake(3000, 4), Fake(0, 4)])
    with pytest.raises(ValueError, match='cuda:1'):
        ops.check_cloud_list([Fake(3000, 4), Fake(2000, 4, device='cuda:1')])
    assert ops.check_cloud_list([Fake(3000, 4), Fake(70000, 4), Fake(5, 4)]) == (torch.device('cuda:0'), 4)


def test_helper_checks_cloud_lists_on_the_host():
    from deepclr_amd.models import ModelInferenceHelper
    model = _model()
    seq = ModelInferenceHelper(model, is_sequential=True)
    with pytest.raises(RuntimeError, match='Wrong point dimension'):
        seq.predict_sequence([torch.zeros(3000, 4), torch.zeros(2000, 3)])
    with pytest.raises(ValueError):
        seq.predict_sequence([])
    pairs = ModelInferenceHelper(model)
    with pytest.raises(RuntimeError, match='as many templates'):
        pairs.predict_batch([torch.zeros(3000, 4)], [torch.zeros(3000, 4), torch.zeros(2000, 4)])
    with pytest.raises(ValueError):
        pairs.predict_batch([torch.zeros(3000, 4)], torch.zeros(1, 3000, 4))
