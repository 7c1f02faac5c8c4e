"""CPU-side checks of K19's synchronised form (torch.nn.SyncBatchNorm on the HIP kernels): the opt-in switch and the predicates that
read it, the new entry points (declared, exported, bound), argument validation without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from far_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('far_bn_sync_moments_f32', 'far_bn_sync_stats_f32', 'far_bn_sync_apply_f32', 'far_bn_sync_bwd_sums_f32', 'far_bn_sync_bwd_dx_f32')


class _Cuda:                      # the predicate only looks at is_cuda / dtype
    is_cuda, dtype = True, torch.float32


@pytest.fixture
def switch():
    """Hands out a setter for ops.USE_HIP_SYNC_BATCHNORM and restores the default afterwards."""
    assert ops.USE_HIP_SYNC_BATCHNORM is False
    yield lambda on: setattr(ops, 'USE_HIP_SYNC_BATCHNORM', on)
    ops.USE_HIP_SYNC_BATCHNORM = False


def test_the_switch_is_off_by_default_and_the_predicate_follows_it(switch):
    from far_amd.loftr import backbone as bb
    from far_amd.ops import conv
    plain, sync = torch.nn.BatchNorm2d(4).train(), torch.nn.SyncBatchNorm(4).train()
    assert conv.USE_HIP_SYNC_BATCHNORM is False
    assert bb._bn_hip(plain, _Cuda) and not bb._bn_hip(sync, _Cuda)
    switch(True)
    assert conv.USE_HIP_SYNC_BATCHNORM is True                # the flat namespace forwards to the submodule that reads it
    assert bb._bn_hip(sync, _Cuda) and bb._bn_hip(plain, _Cuda)
    assert not bb._bn_hip(sync.eval(), _Cuda)                 # eval-mode modules: running statistics, folded elsewhere
    assert not bb._bn_hip(torch.nn.SyncBatchNorm(4).train(), torch.zeros(1, 4, 2, 2))     # CPU tensor
    with torch.no_grad():
        assert not bb._bn_hip(torch.nn.SyncBatchNorm(4).train(), _Cuda)
    switch(False)
    assert not bb._bn_hip(torch.nn.SyncBatchNorm(4).train(), _Cuda)


def test_loftr_method_sets_the_switch(switch):
    from far_amd.config import far_train_config
    from far_amd.loftr import LoFTR
    m = LoFTR(far_train_config()['loftr'])
    keys = list(m.state_dict())
    assert m.set_sync_batchnorm_training() is m and ops.USE_HIP_SYNC_BATCHNORM is True
    assert m.set_sync_batchnorm_training(False) is m and ops.USE_HIP_SYNC_BATCHNORM is False
    assert list(m.state_dict()) == keys


def test_cpu_tensors_raise_with_the_switch_on(switch):
    switch(True)
    bn = torch.nn.SyncBatchNorm(4).train()
    with pytest.raises(_lib.FarHipError):
        ops.bn_act_train(torch.zeros(1, 4, 2, 2), bn, 'relu')
    for fn, args in ((ops.sync_bn_moments, (torch.zeros(1, 4, 2, 2),)),
                     (ops.sync_bn_apply, (torch.zeros(1, 4, 2, 2), torch.zeros(20))),
                     (ops.sync_bn_stats, (torch.zeros(1, 3, 4, dtype=torch.float64),))):
        with pytest.raises(_lib.FarHipError):
            fn(*args)


def test_new_symbols_declared_exported_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'far_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for n in NEW:
        assert re.search(r'\b' + n + r'\s*\(', hdr), f'{n} is not declared in far_hip.h'
        assert hasattr(lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES
    assert lib.far_abi_version() == _lib.EXPECTED_ABI == 8              # pure additions
    # K19's existing entry points keep their signatures
    c_p, c_i, c_l, c_f = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
    assert _lib.SIGNATURES['far_bn_train_bwd_f32'] == (c_i, [c_p] * 6 + [c_l, c_i, c_i, c_f] + [c_p] * 5 + [c_l, c_p])
    assert _lib.SIGNATURES['far_bn_act_train_fwd_f32'] == (c_i, [c_p, c_p, c_l, c_i, c_p, c_p, c_f, c_f, c_p, c_p, c_i, c_f, c_p, c_p, c_p, c_l, c_p])
    for name in ('sync_bn_moments', 'sync_bn_stats', 'sync_bn_apply', 'sync_bn_bwd_sums', 'sync_bn_bwd_dx'):
        assert callable(getattr(ops, name))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                   # never dereferenced: every call below fails validation first
    big = 1 << 40
    # the existing entry points do the same
    assert lib.far_bn_train_stats_f32(None, 8, 4, None, None, 1e-5, 0.1, None, None, one, one, one, one, one, big, None) == -22
    assert lib.far_bn_sync_moments_f32(None, 8, 4, one, one, big, None) == -22
    assert lib.far_bn_sync_moments_f32(one, 8, 4, None, one, big, None) == -22
    assert lib.far_bn_sync_moments_f32(one, 0, 4, one, one, big, None) == -22              # an empty shard
    assert lib.far_bn_sync_moments_f32(one, 8, 6, one, one, big, None) == -22              # C % 4
    assert lib.far_bn_sync_moments_f32(one, 8, 1028, one, one, big, None) == -22           # C > 1024
    assert lib.far_bn_sync_moments_f32(one, 8, 4, one, one, 0, None) == -22                # workspace too small
    assert lib.far_bn_sync_stats_f32(None, 1, 4, None, None, 1e-5, 0.1, None, None, one, None) == -22
    assert lib.far_bn_sync_stats_f32(one, 0, 4, None, None, 1e-5, 0.1, None, None, one, None) == -22
    assert lib.far_bn_sync_stats_f32(one, 2, 4, None, None, 1e-5, 0.1, None, None, None, None) == -22
    assert lib.far_bn_sync_stats_f32(one, 2, 1028, None, None, 1e-5, 0.1, None, None, one, None) == -22
    assert lib.far_bn_sync_apply_f32(one, None, 8, 4, None, 1, 0.0, one, None) == -22
    assert lib.far_bn_sync_apply_f32(one, None, 8, 4, one, 3, 0.0, one, None) == -22      # activation code
    assert lib.far_bn_sync_apply_f32(one, None, 8, 5, one, 1, 0.0, one, None) == -22
    assert lib.far_bn_sync_bwd_sums_f32(one, one, None, one, 8, 4, 1, 0.0, one, one, one, one, big, None) == -22    # act without y
    assert lib.far_bn_sync_bwd_sums_f32(one, one, one, one, 8, 4, 1, 0.0, None, one, one, one, big, None) == -22
    assert lib.far_bn_sync_bwd_sums_f32(one, one, one, one, 8, 4, 1, 0.0, one, one, one, one, 0, None) == -22
    assert lib.far_bn_sync_bwd_dx_f32(one, one, one, one, None, None, 2, 8, 4, 1, 0.0, one, None, one, None) == -22
    assert lib.far_bn_sync_bwd_dx_f32(one, one, one, one, None, one, 0, 8, 4, 1, 0.0, one, None, one, None) == -22
    assert lib.far_bn_sync_bwd_dx_f32(one, one, one, one, None, one, 2, 8, 4, 1, 0.0, one, None, None, None) == -22
    assert lib.far_bn_sync_bwd_dx_f32(one, one, one, one, None, one, 2, -1, 4, 1, 0.0, one, None, one, None) == -22
