"""Times the optimizer step on the model's own parameter table (LoFTR(far_train_config()['loftr']): 189 tensors, 51 M elements):

  (a)  AdamW().step()                                  -- this tree, and the base revision's library + optim.py when prepared
  (b)  AdamW(max_grad_norm=0.5).step()                 -- norm, finalize, fused update
  (c)  far_amd.optim.clip_grad_norm_ + AdamW().step()  -- norm, finalize, scale, update
  (d)  torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step()

All legs run in ONE process, interleaved round by round, each round timed with device events around `--steps` steps after a warm-up
round; the spread of a leg is (max - min) / median over its rounds.  Bytes: the update moves 7 words per element (p, m, v read and
written, g read), the norm pass 1 more, the in-place scale 2 more.  The step() legs include the host side (the walk over 189
parameters that refreshes the gradient pointers); the "launches only" legs enqueue the same entry points on the tables those
optimizers built, with no host work in between, and so show the device time the byte counts speak about.

  python tools/optim_time.py --prepare-base [REV]     (where git is: builds far_amd/lib/libfar_hip_base.so through tools/ab_build.py
                                                       and writes REV's far_amd/optim.py next to it; default HEAD)
  python tools/optim_time.py [--rounds 7] [--steps 20] [--out FILE]      (on the GPU)"""
import argparse
import ctypes
import importlib.util
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BASE_LIB = os.path.join(ROOT, 'far_amd', 'lib', 'libfar_hip_base.so')
BASE_OPTIM = os.path.join(ROOT, 'far_amd', 'lib', 'optim_base.py')


def prepare_base(rev):
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'ab_build.py'), rev], cwd=ROOT)
    src = subprocess.check_output(['git', 'show', f'{rev}:far_amd/optim.py'], cwd=ROOT, text=True)
    with open(BASE_OPTIM, 'w') as f:
        f.write(src)
    print(BASE_LIB, BASE_OPTIM)


def load_base_adamw():
    """(the base revision's AdamW class on the base revision's library, that library), next to this tree's; (None, None) when
    not prepared."""
    if not (os.path.exists(BASE_LIB) and os.path.exists(BASE_OPTIM)):
        return None, None
    import torch  # noqa: F401  (its HIP runtime first: far_amd/_lib.py, load order)
    from far_amd import _lib
    cur = _lib.load()
    base = ctypes.CDLL(BASE_LIB)
    for name in ('far_adamw_table_bytes', 'far_adamw_step_f32', 'far_last_hip_error'):
        fn = getattr(base, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    assert base.far_adamw_step_f32 != cur.far_adamw_step_f32
    shim = types.SimpleNamespace(load=lambda: base, FarHipError=_lib.FarHipError, check=_lib.check)
    spec = importlib.util.spec_from_file_location('far_amd._optim_base', BASE_OPTIM)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod._lib = shim
    return mod.AdamW, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prepare-base', nargs='?', const='HEAD', default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.prepare_base:
        return prepare_base(a.prepare_base)
    import torch
    if not torch.cuda.is_available():
        sys.exit('tools/optim_time.py measures on the GPU: none found')
    from far_amd import optim
    from far_amd.config import far_train_config
    from far_amd.loftr import LoFTR
    shapes = [tuple(p.shape) for p in LoFTR(far_train_config()['loftr']).parameters()]
    nel = sum(torch.Size(s).numel() for s in shapes)
    torch.manual_seed(0)
    grads = [torch.randn(s, device='cuda') * 1e-3 for s in shapes]          # norm about 7: every step of (b), the first of (c), (d) clip

    def params():
        ps = [torch.nn.Parameter(torch.randn(s, device='cuda') * 0.05) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps

    kw = dict(lr=1e-5, weight_decay=0.1)
    legs = {}
    base_cls, base_lib = load_base_adamw()
    if base_cls is not None:
        o = base_cls(params(), **kw)
        legs['(a) AdamW().step(), base revision'] = o.step
    o_a = optim.AdamW(params(), **kw)
    legs['(a) AdamW().step(), this tree'] = o_a.step
    o_b = optim.AdamW(params(), max_grad_norm=0.5, **kw)
    legs['(b) AdamW(max_grad_norm=0.5).step(), fused'] = o_b.step
    p_c = params()
    o_c = optim.AdamW(p_c, **kw)
    legs['(c) far_amd clip_grad_norm_ + AdamW().step()'] = lambda: (optim.clip_grad_norm_(p_c, 0.5), o_c.step())
    p_d = params()
    o_d = torch.optim.AdamW(p_d, **kw)
    legs['(d) torch clip_grad_norm_ + torch.optim.AdamW.step()'] = lambda: (torch.nn.utils.clip_grad_norm_(p_d, 0.5), o_d.step())

    for fn in legs.values():                            # builds every table and workspace the launch-only legs below use
        fn()
    from far_amd import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    st = vp(torch.cuda.current_stream().cuda_stream)
    sc = (1e-5, 0.9, 0.999, 1e-8, 0.1, 1.0 - 0.9 ** 3, (1.0 - 0.999 ** 3) ** 0.5)

    def ok(*rcs):
        assert not any(rcs), rcs

    def tab(o):
        t = o._tables[0]
        return vp(t['dev'].data_ptr()), t['n'], t['nblocks']

    ta, tb, tc = tab(o_a), tab(o_b), tab(o_c)
    tg = next(iter(optim._clip_tables.values()))
    tgp, wg, wb = (vp(tg['dev'].data_ptr()), tg['n'], tg['nblocks']), vp(tg['ws']['buf'].data_ptr()), vp(o_b._ws['buf'].data_ptr())
    if base_cls is not None:
        # on this tree's table and buffers: where a leg's buffers lie moves the kernel by a few per cent, the library must not
        legs['launches only: (a) base revision'] = lambda: ok(base_lib.far_adamw_step_f32(*ta, *sc, st))
    legs['launches only: (a) update'] = lambda: ok(lib.far_adamw_step_f32(*ta, *sc, st))
    legs['launches only: (b) norm, finalize, fused update'] = lambda: ok(
        lib.far_grad_norm_f32(*tb, 0, tb[2], 2.0, 0.5, 0, wb, st), lib.far_adam_step_f32(*tb, *sc, 0, wb, 0, st))
    legs['launches only: (c) norm, finalize, scale, update'] = lambda: ok(
        lib.far_grad_norm_f32(*tgp, 0, tgp[2], 2.0, 0.5, 0, wg, st), lib.far_grad_clip_scale_f32(*tgp, wg, st),
        lib.far_adamw_step_f32(*tc, *sc, st))
    times = {k: [] for k in legs}
    for r in range(a.rounds + 1):                       # round 0 is the warm-up
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if r:
                times[k].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    lines = [f'optimizer step on the model table: {len(shapes)} tensors, {nel} elements ({nel * 4 / 1e6:.0f} MB per word), '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} interleaved rounds of {a.steps} steps per leg after one warm-up round, device events; microseconds per step']
    med = {}
    for k, t in times.items():
        med[k] = statistics.median(t)
        lines.append(f'{k:60s} median {med[k]:8.1f}  min {min(t):8.1f}  max {max(t):8.1f}  spread {(max(t) - min(t)) / med[k] * 100:5.1f} %')
    ka, kb, kc = '(a) AdamW().step(), this tree', '(b) AdamW(max_grad_norm=0.5).step(), fused', '(c) far_amd clip_grad_norm_ + AdamW().step()'
    lines.append(f'(b) / (a) = {med[kb] / med[ka]:.3f} (bytes: 8/7 = 1.143 plus two launch boundaries)   '
                 f'(c) / (a) = {med[kc] / med[ka]:.3f} (bytes: 10/7 = 1.429)   (b) / (c) = {med[kb] / med[kc]:.3f}')
    kbase = '(a) AdamW().step(), base revision'
    if kbase in med:
        lines.append(f'(a) this tree / base revision = {med[ka] / med[kbase]:.3f}')
    la, lb, lc = (med['launches only: ' + x] for x in ('(a) update', '(b) norm, finalize, fused update', '(c) norm, finalize, scale, update'))
    lines.append(f'launches only: (b) / (a) = {lb / la:.3f}   (c) / (a) = {lc / la:.3f}   (b) / (c) = {lb / lc:.3f}   '
                 f'update at 7 words per element: {7 * 4 * nel / la / 1e6:.2f} TB/s')
    if 'launches only: (a) base revision' in med:
        lines.append(f"launches only, same table and buffers: (a) this tree / base revision = {la / med['launches only: (a) base revision']:.3f}")
    print('\n'.join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
