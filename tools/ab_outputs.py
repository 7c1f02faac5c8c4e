"""Same-box A/B of output BITS: runs K22 (ops.full_attention_train), K23 (ops.vit_attention_train, vit_attention_train_qkv), the
K1 training ops (ops.coarse_pos_conf, coarse_dense_focal_loss, sinkhorn_pos_conf, sinkhorn_dense_focal_loss) and K24 (ops.conv_valid,
conv_valid_dgrad, conv_valid_wgrad, conv_valid_train; with two calls of K16's ops.conv_wgrad, whose slab reduction K24 shares) forward
and backward on seeded inputs with far_amd/lib/libfar_hip_base.so (tools/ab_build.py) and with the working tree's library, each in a
fresh child process, and compares the sha256 of every output (out, lse, dq, dk, dv; values, loss, df0, df1, dbin; y, dx, dw).  The
kernels are deterministic and built with -ffp-contract=off: a refactor that keeps every expression gives equal digests; a difference
names the case and the tensor.
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

# K1 training (Z, L, S): one whole tile; the other two straddle the 32-column tile and the 128-row padding.  Each runs without and
# with padded masks (coarse_pos_conf takes none).  K1_T: skt_backward's dispatch -- T = 0 (no dense part), 2 T <= 6 (k_skt_bwd<6>),
# <= 12 (<12>, sparse only), beyond (<0>); the dense forms have <6, .> (also at T = 0) and <0, .>.
K1 = [(2, 48, 48), (1, 35, 72), (1, 130, 70)]
K1_T = {'sparse': (0, 2, 5, 8), 'dense': (0, 2, 8)}
K1_FOCAL = (0.25, 2.0, 0.3, 300.0)                 # alpha, gamma, pos_weight, neg_weight: the dense negative part carries the gradient


def k1_case(np, torch, Z, L, S, amp, seed):
    """f1 = noisy copies of f0's rows at permuted columns (confident matches next to entries far below the clamp); `one`: labels with
    pairwise distinct rows and columns per image (coarse_pos_conf adds u, v with float atomics: one addend per sum); `multi`: the same
    plus six positions on one row of image 0 (more than KFOLD); masks: valid prefixes that differ per image."""
    rng = np.random.default_rng(seed)
    f0 = (amp * rng.standard_normal((Z, L, 256))).astype(np.float32)
    f1 = (amp * rng.standard_normal((Z, S, 256))).astype(np.float32)
    K = min(L, S) - 3
    b, i, j = [], [], []
    for z in range(Z):
        rows, cols = rng.permutation(L)[:K], rng.permutation(S)[:K]
        f1[z, cols] = f0[z, rows] + 0.02 * rng.standard_normal((K, 256)).astype(np.float32)
        keep = rng.permutation(K)[:int(0.7 * K)]
        b += [z] * len(keep); i += rows[keep].tolist(); j += cols[keep].tolist()
    ids = lambda *a: tuple(torch.tensor(x, dtype=torch.int64).cuda() for x in a)
    one = ids(b, i, j)
    extra = rng.permutation(S)[:6].tolist()
    multi = ids(b + [0] * 6, i + [i[0]] * 6, j + extra)
    m0 = torch.arange(L)[None] < torch.tensor([L - 5 - 2 * z for z in range(Z)])[:, None]
    m1 = torch.arange(S)[None] < torch.tensor([S - 3 - z for z in range(Z)])[:, None]
    return torch.from_numpy(f0).cuda(), torch.from_numpy(f1).cuda(), one, multi, (m0.cuda(), m1.cuda())


def k1_training(np, torch, ops, emit):
    from far_amd.ops import coarse
    for n, (Z, L, S) in enumerate(K1):
        f0, f1, one, multi, masks = k1_case(np, torch, Z, L, S, 2.0, 400 + n)
        g0, g1, a0 = k1_case(np, torch, Z, L, S, 3.75, 500 + n)[:2] + (torch.tensor(1.0).cuda(),)         # the Sinkhorn operands
        rng = np.random.default_rng(600 + n)
        up = lambda *shape: torch.from_numpy(np.asarray(rng.standard_normal(shape), np.float32)).cuda()      # upstream gradients
        leaf = lambda *ts: tuple(t.detach().clone().requires_grad_() for t in ts)
        x0, x1 = leaf(f0, f1)
        p = ops.coarse_pos_conf(x0, x1, *one, 0.1)
        emit(f'K1 pos_conf {(Z, L, S)}', ('values', 'df0', 'df1'), (p.detach(),) + torch.autograd.grad(p, (x0, x1), up(p.numel())))
        for mm in ((None, None), masks):
            tag = f'{(Z, L, S)}{" masked" if mm[0] is not None else ""}'
            for split_g in (True, False):
                for no_gt in ((False, True) if n == 0 else (False,)):
                    coarse.DENSE_FOCAL_SPLIT_G = split_g
                    x0, x1 = leaf(f0, f1)
                    loss = ops.coarse_dense_focal_loss(x0, x1, *multi, 0.1, *K1_FOCAL, *mm, no_gt=no_gt)
                    emit(f'K1 dense_focal {tag} split_g={split_g} no_gt={no_gt}', ('loss', 'df0', 'df1'),
                         (loss.detach(),) + torch.autograd.grad(loss, (x0, x1), up()))
            coarse.DENSE_FOCAL_SPLIT_G = True
            for T in K1_T['sparse']:
                x0, x1, a = leaf(g0, g1, a0)
                out = ops.sinkhorn_pos_conf(x0, x1, a, T, *multi, *mm)
                grads = torch.autograd.grad(out, (x0, x1, a), tuple(up(*o.shape) for o in out))
                emit(f'K1 sinkhorn_pos_conf {tag} T={T}', ('values', 'bin0', 'bin1', 'df0', 'df1', 'dbin'), tuple(o.detach() for o in out) + grads)
            for T in K1_T['dense']:
                for no_gt in ((False, True) if n == 0 and T == 2 else (False,)):
                    x0, x1, a = leaf(g0, g1, a0)
                    loss = ops.sinkhorn_dense_focal_loss(x0, x1, a, T, *multi, *K1_FOCAL, *mm, no_gt=no_gt)
                    emit(f'K1 sinkhorn_dense_focal {tag} T={T} no_gt={no_gt}', ('loss', 'df0', 'df1', 'dbin'),
                         (loss.detach(),) + torch.autograd.grad(loss, (x0, x1, a), up()))


# K24 (Cin, Cout) x (N, H, W): 192 output channels are six full N-tiles, 32 and 160 are not; Cin = 128 takes the dgrad's two-tile form;
# 3 images take the forward's 8-row launch form, 64 its 24-row form; 9 x 11 has partial tiles in both directions, 5 x 5 one output pixel
K24_CH = [(32, 192), (128, 192), (192, 192), (32, 32), (64, 160)]
K24_NHW = [(3, 9, 11), (3, 5, 5), (3, 28, 28), (64, 28, 28)]
K16 = [(2, 20, 24, 64, 128, 3, 1), (2, 20, 24, 64, 128, 3, 2)]      # (N, H, W, Cin, Cout, ksize, stride): the shared slab reduction
K24_TRAIN = (2, 9, 11, 128, 192)


def k24(np, torch, ops, emit):
    for i, (cin, cout) in enumerate(K24_CH):
        for j, (N, H, W) in enumerate(K24_NHW):
            rng = np.random.default_rng(700 + 10 * i + j)
            t = lambda *shape, mul=1.0: torch.from_numpy((mul * rng.standard_normal(shape)).astype(np.float32)).cuda()
            x, w = t(N, H, W, cin, mul=3.0), t(cout, cin, 5, 5, mul=(2.0 / (25 * cin)) ** 0.5)
            scale, shift, res = 0.5 + t(cout).abs(), t(cout, mul=0.3), t(N, H - 4, W - 4, cout)
            dy = t(N, H - 4, W - 4, cout, mul=1e-3)
            tag = f'K24 {cin}->{cout} @ {(N, H, W)}'
            emit(tag + ' forward', ('y', 'y_fused'), (ops.conv_valid(x, ops.PackedConvValid(w)),
                                                      ops.conv_valid(x, ops.PackedConvValid(w, scale, shift), residual=res, act='relu')))
            pd = ops.PackedConvValid(w, dgrad=True, pack_scale=ops.PackedConvValid(w).pack_scale)
            sc = ops.grad_scale(dy)
            emit(tag + ' backward', ('dx', 'dw'), (ops.conv_valid_dgrad(dy, pd, dy_scale=sc), ops.conv_valid_wgrad(x, dy, dy_scale=sc)))
    for i, (N, H, W, cin, cout, ks, st) in enumerate(K16):
        rng = np.random.default_rng(800 + i)
        x = torch.from_numpy(rng.standard_normal((N, H, W, cin)).astype(np.float32)).cuda()
        dy = torch.from_numpy((1e-3 * rng.standard_normal((N, (H - 1) // st + 1, (W - 1) // st + 1, cout))).astype(np.float32)).cuda()
        emit(f'K16 {cin}->{cout} {ks}x{ks} stride {st} @ {(N, H, W)}', ('dw',), (ops.conv_wgrad(x, dy, ks, st),))
    N, H, W, cin, cout = K24_TRAIN
    rng = np.random.default_rng(900)
    x = torch.from_numpy((3.0 * rng.standard_normal((N, H, W, cin))).astype(np.float32)).cuda().requires_grad_()
    w = torch.from_numpy((0.03 * rng.standard_normal((cout, cin, 5, 5))).astype(np.float32)).cuda().requires_grad_()
    dy = torch.from_numpy((1e-3 * rng.standard_normal((N, H - 4, W - 4, cout))).astype(np.float32)).cuda()
    y = ops.conv_valid_train(x, w, ops.PackCache(), 'layer')
    emit(f'K24 train {cin}->{cout} @ {(N, H, W)}', ('y', 'dx', 'dw'), (y.detach(),) + torch.autograd.grad(y, (x, w), dy))


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
    k1_training(np, torch, ops, emit)
    k24(np, torch, ops, emit)
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
