"""Inputs of golden G21 (LoFTR's full softmax attention), shared by tools/make_goldens.py:g21 and the tests: everything comes from
seeded numpy generators, so the fixture stores seeds and expected outputs only.  Not a test module."""
import numpy as np

NHEAD = 8

# attention-core cases: q (N, L, H D), k, v (N, S, H D); amp scales q and k (scores = q . k / sqrt(D) have std amp^2)
#   a1 / a2  the coarse shape class at two score magnitudes (|score| up to ~7 and ~60)
#   b        L != S (short query side: the key axis is split across workgroups)
#   c        64 fine-level windows of 25 tokens, head dim 16
#   d        q_mask and kv_mask, different extents per image (the reference is defined on valid query rows only)
CASES = {
    'a1': dict(seed=2101, N=2, L=1200, S=1200, D=32, amp=1.04, stride=24),
    'a2': dict(seed=2102, N=2, L=1200, S=1200, D=32, amp=2.94, stride=24),
    'b': dict(seed=2103, N=2, L=300, S=1200, D=32, amp=1.5, stride=6),
    'c': dict(seed=2104, N=64, L=25, S=25, D=16, amp=1.2, stride=5),
    'd': dict(seed=2105, N=2, L=900, S=1200, D=32, amp=1.5, stride=18, q_valid=(700, 900), kv_valid=(1200, 830)),
}
LAYER = dict(seed=2106, N=2, L=600, S=700, C=256, stride=12)                 # (e) one LoFTREncoderLayer(256, 8, 'full'), x != source
STACK = dict(seed=2107, N=1, h=24, w=32, C=256, stride=8,                    # (f) LocalFeatureTransformer, ['self', 'cross'] * 2
             config={'d_model': 256, 'nhead': NHEAD, 'layer_names': ['self', 'cross'] * 2, 'attention': 'full'})


def core_inputs(name):
    """-> dict(q, k, v fp32 arrays, q_mask / kv_mask bool arrays or None, H, D) of attention-core case `name`."""
    c = CASES[name]
    rng = np.random.default_rng(c['seed'])
    C = NHEAD * c['D']
    q = (c['amp'] * rng.standard_normal((c['N'], c['L'], C))).astype(np.float32)
    k = (c['amp'] * rng.standard_normal((c['N'], c['S'], C))).astype(np.float32)
    v = rng.standard_normal((c['N'], c['S'], C)).astype(np.float32)
    qm = km = None
    if 'q_valid' in c:
        qm = np.zeros((c['N'], c['L']), bool)
        km = np.zeros((c['N'], c['S']), bool)
        for n in range(c['N']):
            qm[n, :c['q_valid'][n]] = True
            km[n, :c['kv_valid'][n]] = True
    return dict(q=q, k=k, v=v, q_mask=qm, kv_mask=km, H=NHEAD, D=c['D'])


def seeded_fill(module, seed):
    """Fills a module's parameters (visited in sorted-name order) from one seeded numpy generator: LayerNorm weights around 1,
    other vectors small, matrices with rows of norm ~1.5 (scores of a few units)."""
    import torch
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            x = rng.standard_normal(tuple(p.shape))
            if name.endswith('norm1.weight') or name.endswith('norm2.weight'):
                x = 1.0 + 0.1 * x
            elif p.dim() == 1:
                x = 0.1 * x
            else:
                x = x * (1.5 / p.shape[1] ** 0.5)
            p.copy_(torch.from_numpy(x).to(p.dtype))
    return module


def layer_inputs():
    c = LAYER
    rng = np.random.default_rng(c['seed'] + 1000)
    x = rng.standard_normal((c['N'], c['L'], c['C'])).astype(np.float32)
    src = rng.standard_normal((c['N'], c['S'], c['C'])).astype(np.float32)
    return x, src


def stack_inputs():
    c = STACK
    rng = np.random.default_rng(c['seed'] + 1000)
    L = c['h'] * c['w']
    f0 = rng.standard_normal((c['N'], L, c['C'])).astype(np.float32)
    f1 = (0.5 * f0[:, rng.permutation(L)] + rng.standard_normal((c['N'], L, c['C']))).astype(np.float32)
    return f0, f1


def strided_rows(a, stride):
    """Rows 0, stride, 2 stride, ... of an (N, L, C) array flattened to (N L, C): what the fixture stores of an output."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1])[::stride])
