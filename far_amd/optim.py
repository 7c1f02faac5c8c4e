"""AdamW for a whole model in one launch (K20, far_amd/csrc/adamw_f32.hip): the optimizer of the reference's training step
(mp3d_loftr/src/optimizers/__init__.py:5-16 -> torch.optim.AdamW) with the same constructor and the same arithmetic, for fp32
parameters on one GPU.  Everything else (other dtypes, CPU parameters, amsgrad, maximize) is torch.optim.AdamW's business.

The rest of the reference's optimizer step lives here too: Adam (the other branch of build_optimizer), gradient clipping by the
global norm (train.py:339 hands gradient_clip_val = TRAINER.GRADIENT_CLIPPING = 0.5 to the trainer) fused into the update --
norm, finalize, update: three launches, no host synchronisation, no pass that rescales the gradients -- a stand-alone
clip_grad_norm_ for callers who keep another optimizer, and a device-side form of PL_LoFTR.optimizer_step's "skip the update when
a gradient is not finite" (lightning_loftr.py:114-123)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib

_CHUNK = 4096


def _norm_type(norm_type):
    nt = float(norm_type)
    if nt != 2.0 and nt != math.inf:
        raise ValueError(f'far_amd.optim: norm_type {norm_type!r} is not implemented (2 or inf; use torch.nn.utils.clip_grad_norm_)')
    return nt


def _upload_table(rows, numels, dev):
    """The device table of K20's kernels for rows {p, g, m, v, n} (int64 [n][5]): pinned host image + device copy.  -> dict"""
    n = len(numels)
    blocks = np.asarray([(i, c) for i, ne in enumerate(numels) for c in range((ne + _CHUNK - 1) // _CHUNK)], dtype=np.int32).reshape(-1, 2)
    nbytes = int(_lib.load().far_adamw_table_bytes(n, len(blocks)))
    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    hv[:n * 40] = rows.view(np.uint8).reshape(-1)
    hv[n * 40:n * 40 + blocks.size * 4] = blocks.view(np.uint8).reshape(-1)
    t = dict(n=n, nblocks=len(blocks), host=host, rows=hv[:n * 40].view(np.int64).reshape(n, 5),
             dev=torch.empty(nbytes, dtype=torch.uint8, device=dev))
    t['dev'].copy_(host, non_blocking=True)
    return t


def _upload_rows(t):
    """Refresh the rows of the device table from the pinned image (the caller has waited for t['uploaded'] before writing it)."""
    n = t['n']
    t['dev'][:n * 40].copy_(t['host'][:n * 40], non_blocking=True)
    if t.get('uploaded') is None:
        t['uploaded'] = torch.cuda.Event()
    t['uploaded'].record(torch.cuda.current_stream(t['dev'].device))


def _workspace(nblocks, dev):
    """A zeroed clipping workspace: the result block {norm f32, coef f32, nonfinite i32, skipped i32} at byte 0, float64 partials
    from byte 64 (far_grad_norm_workspace_bytes)."""
    buf = torch.zeros(int(_lib.load().far_grad_norm_workspace_bytes(nblocks)), dtype=torch.uint8, device=dev)
    return dict(buf=buf, nblocks=nblocks, norm=buf[0:4].view(torch.float32)[0], coef=buf[4:8].view(torch.float32)[0],
                nonfinite=buf[8:12].view(torch.int32)[0], skipped=buf[12:16].view(torch.int32)[0])


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's constructor, plus

    max_grad_norm: clip the gradients of ALL parameter groups by their global norm (torch.nn.utils.clip_grad_norm_(params,
        max_grad_norm, norm_type)) inside step(): a norm launch, a finalize launch and the update, which multiplies every
        gradient by the device-side coefficient on its way in.  p.grad is NOT modified -- torch's two-call form leaves the
        clipped gradients behind, the fused form does not; the parameters and moments are bit-identical to
        far_amd.optim.clip_grad_norm_ followed by a plain step().  norm_type: 2 or inf.
    skip_nonfinite: a step whose gradient norm is NaN or inf leaves every parameter and both moments untouched and counts in
        `skipped_steps`.  state['step'] still advances on such a step: the host cannot know without a synchronisation, so the
        bias corrections of later steps see one step more than was applied.

    grad_norm: 0-d device tensor, the norm of the last step() (a view of the workspace: the next step overwrites it);
    skipped_steps: 0-d int32 device tensor.  Both are None until a step has computed a norm; step() reads neither on the host.
    The defaults (None, False) are today's one-launch step, bit for bit."""
    _coupled = False          # torch.optim.Adam's L2 decay (added to the gradient) instead of the decoupled one

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, *,
                 max_grad_norm=None, norm_type=2.0, skip_nonfinite=False):
        name = type(self).__name__
        if amsgrad or maximize:
            raise ValueError(f'far_amd.optim.{name}: amsgrad / maximize are not implemented (use torch.optim.{name})')
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f'far_amd.optim.{name}: max_grad_norm must be positive (or None), got {max_grad_norm!r}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.norm_type = _norm_type(norm_type)
        self.skip_nonfinite = bool(skip_nonfinite)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tables = {}
        self._ws = None

    @property
    def grad_norm(self):
        return None if self._ws is None else self._ws['norm']

    @property
    def skipped_steps(self):
        return None if self._ws is None else self._ws['skipped']

    def _table(self, gi, group):
        ps = [p for p in group['params'] if p.requires_grad]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise _lib.FarHipError(f'far_amd.optim.{type(self).__name__} needs contiguous fp32 parameters on one GPU')
            st = self.state[p]
            if 'exp_avg' not in st:
                st['step'] = torch.tensor(0.0, dtype=torch.float32)      # a CPU float tensor, as torch.optim.AdamW keeps it
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            elif (st['exp_avg'].dtype != torch.float32 or not st['exp_avg'].is_contiguous() or st['exp_avg'].device != dev
                  or not st['exp_avg_sq'].is_contiguous()):
                raise _lib.FarHipError(f'far_amd.optim.{type(self).__name__}: loaded moment tensors must be contiguous fp32 on the parameters\' GPU')
        # the table holds raw pointers: rebuilt when a parameter or a moment tensor was replaced (load_state_dict, .to(), a new model)
        key = tuple((p.data_ptr(), p.numel(), self.state[p]['exp_avg'].data_ptr(), self.state[p]['exp_avg_sq'].data_ptr()) for p in ps)
        t = self._tables.get(gi)
        if t is not None and t['key'] == key:
            return t
        rows = np.zeros((len(ps), 5), dtype=np.int64)                        # {p, g, m, v, n}
        for i, p in enumerate(ps):
            st = self.state[p]
            rows[i] = (p.data_ptr(), 0, st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(), p.numel())
        t = _upload_table(rows, [p.numel() for p in ps], dev)
        t.update(key=key, params=ps)
        self._tables[gi] = t
        return t

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        name = type(self).__name__
        work = []
        for gi, group in enumerate(self.param_groups):
            t = self._table(gi, group)
            if t is None:
                continue
            # the gradient pointers change whenever autograd re-allocates them (zero_grad(set_to_none=True)): refresh that column --
            # after the previous step's upload has left the pinned buffer (nothing else orders the host against it)
            if t.get('uploaded') is not None:
                t['uploaded'].synchronize()
            # validate first, mutate after: a raise must leave the optimizer state as it was
            active = []
            for i, p in enumerate(t['params']):
                g = p.grad
                if g is not None:
                    if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                        raise _lib.FarHipError(f'far_amd.optim.{name} needs dense contiguous fp32 gradients')
                    active.append((i, p, g))
            steps = {int(self.state[p]['step']) for _, p, _ in active}
            if len(steps) > 1:
                raise _lib.FarHipError(f'far_amd.optim.{name}: parameters of one group have different step counts '
                                       f'(a parameter skipped earlier steps): use torch.optim.{name}')
            work.append((t, group, active, steps))
        clip = self.max_grad_norm is not None or self.skip_nonfinite
        if clip and len({t['dev'].device for t, _, _, steps in work if steps}) > 1:
            raise _lib.FarHipError(f'far_amd.optim.{name}: max_grad_norm / skip_nonfinite need all parameter groups on one GPU')
        launches = []
        for t, group, active, steps in work:
            t['rows'][:, 1] = 0
            if not steps:
                continue
            k = steps.pop() + 1
            for i, p, g in active:
                t['rows'][i, 1] = g.data_ptr()
                st = self.state[p]
                if torch.is_tensor(st['step']):           # the step stays a tensor (torch.optim can resume this state dict)
                    st['step'] += 1
                else:
                    st['step'] = k
            _upload_rows(t)
            launches.append((t, group, k))
        if not launches:
            return loss
        ws = None
        if clip:
            # one norm over all groups: every table writes its partials behind the previous one's, the last launch finalizes.
            # (skip_nonfinite alone: an infinite bound -- the coefficient is exactly 1 for every finite norm)
            dev = launches[0][0]['dev'].device
            total = sum(t['nblocks'] for t, _, _ in launches)
            ws = self._ws
            if ws is None or ws['nblocks'] < total or ws['buf'].device != dev:
                self._ws = _workspace(max(total, sum(t['nblocks'] for t in self._tables.values())), dev)
                if ws is not None and ws['buf'].device == dev:
                    self._ws['skipped'].copy_(ws['skipped'])          # the counter outlives its workspace
                ws = self._ws
            first = 0
            for j, (t, _, _) in enumerate(launches):
                rc = lib.far_grad_norm_f32(ctypes.c_void_p(t['dev'].data_ptr()), t['n'], t['nblocks'], first,
                                           total if j == len(launches) - 1 else 0, self.norm_type,
                                           math.inf if self.max_grad_norm is None else self.max_grad_norm, int(self.skip_nonfinite),
                                           ctypes.c_void_p(ws['buf'].data_ptr()), _stream(dev))
                _lib.check(rc, 'far_grad_norm_f32')
                first += t['nblocks']
        for t, group, k in launches:
            b1, b2 = group['betas']
            args = (ctypes.c_void_p(t['dev'].data_ptr()), t['n'], t['nblocks'], float(group['lr']), float(b1), float(b2),
                    float(group['eps']), float(group['weight_decay']), 1.0 - b1 ** k, math.sqrt(1.0 - b2 ** k))
            if ws is None and not self._coupled:
                _lib.check(lib.far_adamw_step_f32(*args, _stream(t['dev'].device)), 'far_adamw_step_f32')
            else:
                rc = lib.far_adam_step_f32(*args, int(self._coupled), ctypes.c_void_p(ws['buf'].data_ptr()) if ws is not None else None,
                                           int(self.skip_nonfinite), _stream(t['dev'].device))
                _lib.check(rc, 'far_adam_step_f32')
        return loss


class Adam(AdamW):
    """torch.optim.Adam (the reference's TRAINER.OPTIMIZER = 'adam'): the same step with the weight decay added to the gradient
    (g += weight_decay p, after clipping) instead of decoupled, in the order of torch's single-tensor path; its state dict is
    interchangeable with torch.optim.Adam's.  max_grad_norm / norm_type / skip_nonfinite as in AdamW."""
    _coupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False, *,
                 max_grad_norm=None, norm_type=2.0, skip_nonfinite=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         max_grad_norm=max_grad_norm, norm_type=norm_type, skip_nonfinite=skip_nonfinite)


_clip_tables = {}          # (device, numels) -> gradient-only table + workspace of clip_grad_norm_ (a few entries)


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ on K20's kernels, for callers who keep another optimizer: the gradients of `parameters` are
    multiplied in place by min(max_norm / (norm + 1e-6), 1) (norm, finalize and scale launches; the coefficient never leaves the
    device) and the norm comes back as a 0-d device tensor.  Only error_if_nonfinite=True synchronises."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    max_norm = float(max_norm)
    nt = _norm_type(norm_type)
    if not max_norm > 0.0:
        raise ValueError(f'far_amd.optim.clip_grad_norm_: max_norm must be positive, got {max_norm!r}')
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or g.is_sparse or not g.is_contiguous() or g.device != dev:
            raise _lib.FarHipError('far_amd.optim.clip_grad_norm_ needs dense contiguous fp32 gradients on one GPU')
    lib = _lib.load()
    numels = tuple(g.numel() for g in grads)
    ptrs = tuple(g.data_ptr() for g in grads)
    t = _clip_tables.get((dev, numels))
    if t is None:
        rows = np.zeros((len(grads), 5), dtype=np.int64)
        rows[:, 1] = ptrs
        rows[:, 4] = numels
        t = _upload_table(rows, numels, dev)
        t.update(key=ptrs, ws=_workspace(t['nblocks'], dev))
        while len(_clip_tables) >= 4:
            _clip_tables.pop(next(iter(_clip_tables)))
        _clip_tables[(dev, numels)] = t
    elif t['key'] != ptrs:                                 # the table holds raw pointers: autograd re-allocated the gradients
        if t.get('uploaded') is not None:
            t['uploaded'].synchronize()
        t['rows'][:, 1] = ptrs
        t['key'] = ptrs
        _upload_rows(t)
    ws = t['ws']
    tp, wp = ctypes.c_void_p(t['dev'].data_ptr()), ctypes.c_void_p(ws['buf'].data_ptr())
    _lib.check(lib.far_grad_norm_f32(tp, t['n'], t['nblocks'], 0, t['nblocks'], nt, max_norm, 0, wp, _stream(dev)), 'far_grad_norm_f32')
    if error_if_nonfinite and bool(ws['nonfinite']):
        raise RuntimeError(f'The total norm of order {nt} for gradients from `parameters` is non-finite, so it cannot be clipped. '
                           'To disable this error and scale the gradients by the non-finite norm anyway, set '
                           '`error_if_nonfinite=False`')
    _lib.check(lib.far_grad_clip_scale_f32(tp, t['n'], t['nblocks'], wp, _stream(dev)), 'far_grad_clip_scale_f32')
    return ws['norm'].clone()


def build_optimizer(params, name, lr, adam_decay=0., adamw_decay=0.1, gradient_clip_val=None):
    """The reference's build_optimizer (src/optimizers/__init__.py:5-14: TRAINER.OPTIMIZER, TRUE_LR, ADAM_DECAY, ADAMW_DECAY) with
    the trainer's gradient_clip_val (TRAINER.GRADIENT_CLIPPING, 0.5 in every configuration) folded into the step."""
    if name == 'adam':
        return Adam(params, lr=lr, weight_decay=adam_decay, max_grad_norm=gradient_clip_val)
    elif name == 'adamw':
        return AdamW(params, lr=lr, weight_decay=adamw_decay, max_grad_norm=gradient_clip_val)
    else:
        raise ValueError(f'TRAINER.OPTIMIZER = {name} is not a valid optimizer!')
