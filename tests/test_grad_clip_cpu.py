"""CPU-side checks of the clipping / Adam additions to K20 (far_amd/optim.py, far_amd/csrc/adamw_f32.hip): symbols, the workspace
query, constructor validation, build_optimizer's mapping, and that CPU parameters raise instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

from far_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('far_grad_norm_workspace_bytes', 'far_grad_norm_f32', 'far_grad_clip_scale_f32', 'far_adam_step_f32')


def _params():
    return [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3, 2))]


def test_new_symbols_declared_exported_bound():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'far_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for n in NEW:
        assert re.search(r'\b' + n + r'\s*\(', hdr), f'{n} is not declared in far_hip.h'
        assert hasattr(lib, n), f'{n} is not exported'
        assert n in _lib.SIGNATURES
    assert lib.far_abi_version() == 8
    assert _lib.EXPECTED_ABI == 8
    # far_adamw_step_f32 keeps its signature
    assert _lib.SIGNATURES['far_adamw_step_f32'] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_long] + [ctypes.c_double] * 7
                                                     + [ctypes.c_void_p])


def test_workspace_query_needs_no_gpu_and_grows():
    lib = _lib.load()
    sizes = [int(lib.far_grad_norm_workspace_bytes(n)) for n in (1, 2, 1024, 12500)]
    assert sizes[0] >= 16 + 8                                   # the result block and one float64 partial
    assert all(b > a for a, b in zip(sizes, sizes[1:]))
    assert sizes[3] - sizes[2] == (12500 - 1024) * 8            # one float64 per workgroup
    assert int(lib.far_grad_norm_workspace_bytes(0)) == 0 and int(lib.far_grad_norm_workspace_bytes(-3)) == 0


def test_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                   # never dereferenced: every call below fails validation first
    assert lib.far_grad_norm_f32(None, 1, 1, 0, 1, 2.0, 0.5, 0, one, None) == -22
    assert lib.far_grad_norm_f32(one, 1, 1, 0, 1, 2.0, 0.5, 0, None, None) == -22
    assert lib.far_grad_norm_f32(one, 1, -1, 0, 1, 2.0, 0.5, 0, one, None) == -22
    assert lib.far_grad_norm_f32(one, 0, 1, 0, 1, 2.0, 0.5, 0, one, None) == -22
    assert lib.far_grad_norm_f32(one, 1, 1, 0, 1, 2.0, 0.0, 0, one, None) == -22          # max_norm <= 0
    assert lib.far_grad_norm_f32(one, 1, 1, 0, 1, 2.0, -1.0, 0, one, None) == -22
    assert lib.far_grad_norm_f32(one, 1, 1, 0, 1, 2.0, float('nan'), 0, one, None) == -22
    assert lib.far_grad_norm_f32(one, 1, 1, 0, 1, 3.0, 0.5, 0, one, None) == -22          # norm_type
    assert lib.far_grad_norm_f32(one, 1, 4, 2, 5, 2.0, 0.5, 0, one, None) == -22          # total < first + nblocks
    assert lib.far_grad_norm_f32(one, 1, 1, -1, 0, 2.0, 0.5, 0, one, None) == -22
    assert lib.far_grad_clip_scale_f32(None, 1, 1, one, None) == -22
    assert lib.far_grad_clip_scale_f32(one, 1, 1, None, None) == -22
    assert lib.far_grad_clip_scale_f32(one, 1, 0, one, None) == -22
    args = (1e-3, 0.9, 0.999, 1e-8, 0.1, 0.1, 0.03)
    assert lib.far_adam_step_f32(None, 1, 1, *args, 1, None, 0, None) == -22
    assert lib.far_adam_step_f32(one, 1, -2, *args, 1, None, 0, None) == -22
    assert lib.far_adam_step_f32(one, 1, 1, *args, 0, None, 1, None) == -22               # skip_nonfinite needs the workspace


@pytest.mark.parametrize('cls', [optim.AdamW, optim.Adam])
def test_constructor_validation(cls):
    for bad in (0, 0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='max_grad_norm'):
            cls(_params(), max_grad_norm=bad)
    for bad in (1, 1.0, 3.0, 0.5, -float('inf')):
        with pytest.raises(ValueError, match='norm_type'):
            cls(_params(), max_grad_norm=0.5, norm_type=bad)
    with pytest.raises(ValueError, match='amsgrad'):
        cls(_params(), amsgrad=True)
    with pytest.raises(ValueError, match='maximize'):
        cls(_params(), maximize=True)
    o = cls(_params(), max_grad_norm=0.5, norm_type='inf', skip_nonfinite=True)
    assert o.max_grad_norm == 0.5 and o.norm_type == float('inf') and o.skip_nonfinite is True
    assert o.grad_norm is None and o.skipped_steps is None
    o = cls(_params())
    assert o.max_grad_norm is None and o.norm_type == 2.0 and o.skip_nonfinite is False
    # the constructor of the torch class: same positional order, same defaults
    t = getattr(torch.optim, cls.__name__)(_params())
    for k in ('lr', 'betas', 'eps', 'weight_decay'):
        assert o.defaults[k] == t.defaults[k]
    assert set(o.state_dict()['param_groups'][0]) == {'lr', 'betas', 'eps', 'weight_decay', 'params'}


def test_build_optimizer_maps_names():
    o = optim.build_optimizer(_params(), 'adamw', 8e-3)
    assert type(o) is optim.AdamW and o.defaults['lr'] == 8e-3 and o.defaults['weight_decay'] == 0.1 and o.max_grad_norm is None
    o = optim.build_optimizer(_params(), 'adam', 1e-3, adam_decay=0.25, adamw_decay=0.5, gradient_clip_val=0.5)
    assert type(o) is optim.Adam and o.defaults['weight_decay'] == 0.25 and o.max_grad_norm == 0.5 and o._coupled
    o = optim.build_optimizer(_params(), 'adamw', 1e-3, adam_decay=0.25, adamw_decay=0.5, gradient_clip_val=0.5)
    assert type(o) is optim.AdamW and o.defaults['weight_decay'] == 0.5 and o.max_grad_norm == 0.5 and not o._coupled
    assert optim.build_optimizer(_params(), 'adam', 1e-3).defaults['weight_decay'] == 0.0
    with pytest.raises(ValueError) as e:
        optim.build_optimizer(_params(), 'sgd', 1e-3)
    assert str(e.value) == 'TRAINER.OPTIMIZER = sgd is not a valid optimizer!'


@pytest.mark.parametrize('cls', [optim.AdamW, optim.Adam])
def test_cpu_parameters_raise(cls):
    ps = _params()
    for p in ps:
        p.grad = torch.ones_like(p)
    for kw in ({}, {'max_grad_norm': 0.5}, {'skip_nonfinite': True}):
        with pytest.raises(_lib.FarHipError):
            cls(ps, **kw).step()
    assert all(float(p.detach().abs().max()) == 0.0 for p in ps)


def test_clip_grad_norm_cpu_and_arguments():
    ps = _params()
    assert float(optim.clip_grad_norm_(ps, 0.5)) == 0.0          # no gradients: torch returns tensor(0.)
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(_lib.FarHipError):
        optim.clip_grad_norm_(ps, 0.5)
    with pytest.raises(ValueError, match='norm_type'):
        optim.clip_grad_norm_(ps, 0.5, norm_type=1.0)
    with pytest.raises(ValueError, match='max_norm'):
        optim.clip_grad_norm_(ps, 0.0)
    assert all(bool((p.grad == 1).all()) for p in ps)
