"""CPU: the training library (include/deepclr_amd_train.h) -- symbols, argument checks before any launch, the workspace
formula, the compiled kernel set, and which set-abstraction levels DeepCLR.set_fused_training puts on it."""
import ctypes
import os
import re

import pytest

from deepclr_amd import build, lib, synthetic
from deepclr_amd.config import model_config_from_dict
from deepclr_amd.models import build_model
from helpers import (custom_features_cfg, custom_widths_cfg, small_bn_cfg, small_cfg, small_transform_cfg,
                     small_two_level_cfg)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVAL, UNSUP = -1, -2


def test_train_header_signatures_and_exports_agree():
    header = open(os.path.join(ROOT, 'include', 'deepclr_amd_train.h')).read()
    declared = set(re.findall(r'\b(dclr_[a-z0-9_]+)\s*\(', header)) - {'dclr_stream_t'}
    assert declared == set(lib.TRAIN_SIGNATURES), declared ^ set(lib.TRAIN_SIGNATURES)
    assert not declared & set(lib.SIGNATURES)
    assert os.path.exists(lib.TRAIN_LIB_PATH), 'run python -m deepclr_amd.build'
    handle = ctypes.CDLL(lib.TRAIN_LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    assert lib.load_train().dclr_train_version() >= 1
    # the inference library is untouched: none of the training entry points, ABI 0.2
    inference = ctypes.CDLL(lib.LIB_PATH)
    assert not any(hasattr(inference, name) for name in declared)
    assert lib.load().dclr_version() == 2


def _fake(addr=0x100000):
    return ctypes.c_void_p(addr)                  # never dereferenced: every call below is rejected before a launch


def test_train_forward_rejects_bad_arguments_without_a_gpu():
    f = lib.load_train().dclr_sa_msg_train_forward
    p = _fake()
    ns = (ctypes.c_int * 2)(8, 16)
    ns_bad = (ctypes.c_int * 2)(8, 0)
    idx = (ctypes.c_void_p * 2)(0x100000, 0x100000)
    idx_null = (ctypes.c_void_p * 2)(0x100000, None)
    ok = dict(b=2, n=512, f=1, npoint=64, scales=2, ns=ns, xyz=p, feats=p, new_xyz=p, idx=idx, w=p, out=p, arg=p)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['b'], a['n'], a['f'], a['npoint'], a['scales'], a['ns'], a['xyz'], a['feats'], a['new_xyz'], a['idx'],
                 a['w'], a['out'], a['arg'], None)
    for bad in ('ns', 'idx', 'xyz', 'new_xyz', 'w', 'out', 'arg'):
        assert call(**{bad: None}) == INVAL, bad
    assert call(feats=None) == INVAL                               # f = 1 needs the feature channel
    assert call(b=0) == INVAL and call(n=0) == INVAL and call(npoint=0) == INVAL and call(npoint=-5) == INVAL
    assert call(scales=0) == INVAL and call(f=-1) == INVAL
    assert call(scales=3) == UNSUP and call(f=2) == UNSUP
    assert call(ns=ns_bad) == INVAL and call(idx=idx_null) == INVAL


def test_train_backward_rejects_bad_arguments_without_a_gpu():
    lt = lib.load_train()
    f = lt.dclr_sa_msg_train_backward
    p = _fake()
    need = lt.dclr_sa_msg_train_workspace_bytes(2, 64, 2)
    ok = dict(b=2, n=512, f=0, npoint=64, scales=2, xyz=p, feats=None, new_xyz=p, w=p, g=p, arg=p, out=p, ws=p, wsb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['b'], a['n'], a['f'], a['npoint'], a['scales'], a['xyz'], a['feats'], a['new_xyz'], a['w'], a['g'],
                 a['arg'], a['out'], a['ws'], a['wsb'], None)
    for bad in ('xyz', 'new_xyz', 'w', 'g', 'arg', 'out', 'ws'):
        assert call(**{bad: None}) == INVAL, bad
    assert call(f=1) == INVAL                                      # f = 1 without features
    assert call(b=0) == INVAL and call(n=-1) == INVAL and call(npoint=0) == INVAL and call(scales=0) == INVAL
    assert call(scales=3) == UNSUP and call(f=2, feats=p) == UNSUP
    assert call(wsb=need - 1) == INVAL                             # a short workspace
    assert call(wsb=0) == INVAL
    assert call(ws=_fake(0x100004)) == INVAL                       # misaligned
    assert call(ws=_fake(0x100008)) == INVAL


def test_train_workspace_formula_is_monotone_and_aligned():
    ws = lib.load_train().dclr_sa_msg_train_workspace_bytes
    assert ws(0, 64, 1) == INVAL and ws(1, 0, 1) == INVAL and ws(1, 64, 0) == INVAL and ws(1, 64, 3) == UNSUP
    prev = {}
    for scales in (1, 2):
        for b in (1, 2, 5, 10, 64):
            for npoint in (1, 31, 32, 33, 64, 96, 1000, 1024, 4096):
                v = ws(b, npoint, scales)
                assert v > 0 and v % 256 == 0, (b, npoint, scales, v)
                # enough for one 896-float partial per (cloud, scale, block of 32 centroids)
                assert v >= b * scales * -(-npoint // 32) * 896 * 4
                for key in ((b - 1, npoint, scales), (b, npoint - 1, scales), (b, npoint, scales - 1)):
                    if key in prev:
                        assert v >= prev[key], (key, prev[key], v)
                prev[(b, npoint, scales)] = v
                assert ws(b, npoint, 2) >= ws(b, npoint, 1)
    # the shipped KITTI shape: 10 clouds x 1024 centroids x 2 scales stays around a megabyte
    assert ws(10, 1024, 2) <= 4 << 20


def _kernel_name(mangled: str) -> str:
    m = re.search(r'\d+(sa_train_[a-z]+_kernel)', mangled)
    return m.group(1) if m else mangled


def test_train_library_holds_exactly_its_kernels_without_spills():
    usage = build.train_kernel_usage()
    assert usage, 'run python -m deepclr_amd.build'
    names = sorted(_kernel_name(k) for k in usage)
    assert names == ['sa_train_bwd_kernel', 'sa_train_fwd_kernel', 'sa_train_reduce_kernel']
    for k, u in usage.items():
        assert u['scratch'] == 0, (k, u)
        assert u['lds'] <= 64 * 1024, (k, u)


def test_inference_library_kernel_set_is_unchanged():
    usage = build.kernel_usage()
    assert not any('sa_train' in k for k in usage)
    assert 'sa_train.hip' not in build.SOURCES and build.TRAIN_SOURCES == ['sa_train.hip']
    sources = {os.path.basename(p) for p in os.listdir(build.CSRC) if p.endswith('.usage.txt')}
    assert {s.replace('.hip', '.usage.txt') for s in build.SOURCES} <= sources


@pytest.mark.parametrize('name, cfg, want', [
    ('small', small_cfg, ['_cloud_layers.0._sa0']),
    ('modelnet', lambda: synthetic.model_cfg('modelnet'), ['_cloud_layers.0._sa0']),
    ('kitti', lambda: synthetic.model_cfg('kitti'), ['_cloud_layers.0._sa0']),
    # level 1 reads level 0's features, which carry a gradient (and has widths the fused kernel does not take)
    ('two_level', small_two_level_cfg, ['_cloud_layers.0._sa0']),
    # the transform fuses; the feature module behind it reads the transform's features
    ('transform', small_transform_cfg, ['_cloud_layers.0._sa0']),
    ('custom_widths', custom_widths_cfg, []),
    ('custom_features', custom_features_cfg, []),
    ('batch_norm', small_bn_cfg, []),
])
def test_set_fused_training_reports_the_levels_that_take_the_fused_path(name, cfg, want):
    model = build_model(model_config_from_dict(cfg()))
    levels = [m for m in model.modules() if type(m).__name__ == 'PointnetSAModuleMSG']
    assert all(m.fused_training is False for m in levels)          # default off
    keys = set(model.state_dict())
    assert model.set_fused_training() == want
    assert all(m.fused_training is True for m in levels)
    assert set(model.state_dict()) == keys                         # a plain attribute: the state_dict is unchanged
    assert model.set_fused_training(False) == []
    assert all(m.fused_training is False for m in levels)
