"""Same-box A/B of output BITS: runs K22 (ops.full_attention_train) and K23 (ops.vit_attention_train, vit_attention_train_qkv) forward
and backward on seeded inputs with far_amd/lib/libfar_hip_base.so (tools/ab_build.py) and with the working tree's library, each in a
fresh child process, and compares the sha256 of every output (out, lse, dq, dk, dv).  The kernels are deterministic and built with
-ffp-contract=off: a refactor that keeps every expression gives equal digests; a difference names the case and the tensor.
Usage: python tools/ab_build.py [rev] && python tools/ab_outputs.py      (exit status 1 on any difference or a failed child)"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.join(ROOT, 'far_amd', 'lib', 'libfar_hip_base.so')

# K22 (N, L, S, H, D): forward split + dq split; dk/dv split; no split; the one-wave form; forward one-wave, backward tiled; masks
K22 = [(2, 300, 1200, 8, 32), (2, 1200, 300, 8, 32), (2, 200, 150, 8, 32), (3, 25, 25, 8, 16), (2, 40, 25, 8, 16), (2, 130, 70, 3, 16)]
K22_VALID = {(2, 130, 70, 3, 16): ((90, 130), (70, 33))}          # valid query / key prefix per image (tests: case t7)
# K23 (Z, L, S, H); the last one also as one packed (Z, N, 3 H 64) qkv projection
K23 = [(2, 130, 65, 3), (2, 33, 40, 3), (2, 576, 576, 3), (2, 130, 130, 3)]


def child():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from far_amd import ops

    def emit(case, names, tensors):
        torch.cuda.synchronize()
        for nm, t in zip(names, tensors):
            print(json.dumps({'case': case, 'tensor': nm, 'sha256': hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()}), flush=True)

    def randn(rng, *shape):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()

    names = ('out', 'lse', 'dq', 'dk', 'dv')
    for i, (N, L, S, H, D) in enumerate(K22):
        rng = np.random.default_rng(100 + i)
        q, k, v, g = randn(rng, N, L, H * D), randn(rng, N, S, H * D), randn(rng, N, S, H * D), randn(rng, N, L, H * D)
        qm = km = None
        if (N, L, S, H, D) in K22_VALID:
            qv, kv = K22_VALID[(N, L, S, H, D)]
            qm = (torch.arange(L)[None] < torch.tensor(qv)[:, None]).cuda()
            km = (torch.arange(S)[None] < torch.tensor(kv)[:, None]).cuda()
        q.requires_grad_(); k.requires_grad_(); v.requires_grad_()
        out = ops.full_attention_train(q, k, v, H, qm, km)
        lse = out.grad_fn.saved_tensors[4]
        emit(f'K22 {(N, L, S, H, D)}', names, (out.detach(), lse) + torch.autograd.grad(out, (q, k, v), g))
    for i, (Z, L, S, H) in enumerate(K23):
        rng = np.random.default_rng(200 + i)
        q, k, v, g = randn(rng, Z, L, H * 64), randn(rng, Z, S, H * 64), randn(rng, Z, S, H * 64), randn(rng, Z, L, H * 64)
        q.requires_grad_(); k.requires_grad_(); v.requires_grad_()
        out = ops.vit_attention_train(q, k, v, H)
        lse = out.grad_fn.saved_tensors[-1]
        emit(f'K23 {(Z, L, S, H)}', names, (out.detach(), lse) + torch.autograd.grad(out, (q, k, v), g))
    Z, N, _, H = K23[-1]
    rng = np.random.default_rng(300)
    qkv, g = randn(rng, Z, N, 3 * H * 64).requires_grad_(), randn(rng, Z, N, H * 64)
    out = ops.vit_attention_train_qkv(qkv, H)
    lse = out.grad_fn.saved_tensors[-1]
    dqkv, = torch.autograd.grad(out, (qkv,), g)
    emit(f'K23 packed {(Z, N, N, H)}', names, (out.detach(), lse) + tuple(dqkv[..., j * H * 64:(j + 1) * H * 64] for j in range(3)))
    if ops.activation_overflowed('cuda'):
        sys.exit('the overflow flag is set: the inputs left the split range')


def run(lib):
    env = dict(os.environ)
    env.pop('FAR_HIP_LIB', None)
    if lib:
        env['FAR_HIP_LIB'] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, stdout=subprocess.PIPE, text=True, timeout=300)
    if p.returncode != 0:
        sys.exit(f'the child on {lib or "the working tree library"} ended with status {p.returncode}')
    return [json.loads(l) for l in p.stdout.splitlines() if l.startswith('{')]


def main():
    if not os.path.exists(BASE):
        sys.exit(f'{BASE} is missing: python tools/ab_build.py [rev] builds it')
    base, new = run(BASE), run(None)
    diff = [(b, n) for b, n in zip(base, new) if b != n]
    for b, n in diff:
        print(f'DIFFERENT {b["case"]} {b["tensor"]}: base {b["sha256"][:16]} new {n["sha256"][:16]}')
    ok = len(base) == len(new) and not diff
    print(json.dumps({'tool': 'ab_outputs', 'outputs': len(new), 'different': len(diff), 'equal': ok}))
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    child() if '--child' in sys.argv else main()
