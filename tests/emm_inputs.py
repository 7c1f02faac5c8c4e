"""Inputs, float64 / fp32 references and the per-block parity rule of the K2 tests (tests/test_emm_parity_cpu.py,
tests/test_emm_parity_gpu.py).  torch only, device-agnostic, seeded: the values are drawn on the CPU generator and moved, so a
case is the same numbers wherever it runs.

K2 is the bilinear dual-softmax attention of the EMM head (transformer.py:275-292):
    s = (q k^T) * scale,  P = softmax(s, keys) * softmax(s, queries),  v~ = [v | pos],  T = P v~ (Z, N, 70),  F = v~^T T (Z, 70, 70).

The rule is the project's parity rule (tests/test_full_attention_gpu.py: _bar, FLOOR = 2^-20, factor 3 on dev32) applied per output
block instead of per tensor, because the dual softmax spreads the rows of T over many decades and a whole-tensor tolerance hides
every block whose entries are small next to max|T|:

    max_b |got - r64|  <=  max(3 max_b |r32 - r64|,  2^-20 max_b S)

r64 / r32 are the float64 / fp32 torch compositions on the same device in the same run, and S the sum of magnitudes behind each
element from the float64 reference (S = P |v~| for T, |v~|^T P |v~| for F): rounding of a sum scales with the magnitudes summed, and
the split keeps 22 bits per operand and drops lo.lo -- about 2^-21 S for a product -- so the floor leaves a margin of two.
With the floor at 2^-20 S alone the rule cannot be met by an fp32-grade kernel, the exact-f32 one included (figures in the docstring
of tests/test_emm_parity_gpu.py: test_forward_per_block): it knows nothing of the score's magnitude, which enters P through the
exponent, and dev32_b is ~0 wherever the torch softmax cancels exactly.  The floor is therefore extended by terms derived from the
code and the number formats (score_floor_T, split_floor_T); nothing in the bar is taken from a kernel's error.
Blocks of T: 32 consecutive rows x the columns [0, 32), [32, 64), [64, 70) (the MFMA row tile and the three column tiles; the third is
the partly filled one that shares its tile with the column references).  Blocks of F: the 3 x 3 products of those column groups."""
import math

import torch

REGIMES = ('flat', 'peaked', 'shifted', 'negative')
KEY_COUNTS = (1, 33, 64, 65, 128, 129, 221, 320)
SCALE = 0.125
FLOOR = 2.0 ** -20
FACTOR = 3.0
ROWS = 32
COL_GROUPS = ((0, 32), (32, 64), (64, 70))
HIDDEN = 2e-4                     # a block is hidden when max_b |T| < HIDDEN max|T|: ten times the old atol of 2e-5 max|T|


def case_seed(N, regime):
    """The committed seed of the (N, regime) case."""
    return 100 * N + REGIMES.index(regime)


def emm_case(Z, N, regime, seed, device='cpu'):
    """q, k, v (Z, N, 64) and pos (N, 6) fp32.  pos is signed uniform in (-1, 1) (no constant column).
    flat: q, k = 2 randn.  peaked: q, k = 6 randn (|s| beyond 100).  shifted: u = randn(64), q = 2 randn + u, k = 2 randn, last key
    = 6 u: the maximum-score key of (nearly) every row is the last real key, so every row rescales in the last, possibly partial,
    tile.  negative: q = 2 randn + 3 u, k = 2 randn - 3 u: every real score is far below 0, the score of a zero-padded key or query."""
    if regime not in REGIMES:
        raise ValueError(regime)
    g = torch.Generator().manual_seed(int(seed))
    q = torch.randn(Z, N, 64, generator=g)
    k = torch.randn(Z, N, 64, generator=g)
    v = torch.randn(Z, N, 64, generator=g)
    pos = torch.rand(N, 6, generator=g) * 2 - 1
    u = torch.randn(64, generator=g)
    if regime == 'flat':
        q, k = 2 * q, 2 * k
    elif regime == 'peaked':
        q, k = 6 * q, 6 * k
    elif regime == 'shifted':
        q, k = 2 * q + u, 2 * k
        k[:, -1] = 6 * u
    else:
        q, k = 2 * q + 3 * u, 2 * k - 3 * u
    return tuple(t.contiguous().to(device) for t in (q, k, v, pos))


def vtilde(v, pos):
    return torch.cat([v, pos.unsqueeze(0).expand(v.shape[0], -1, -1)], dim=2)


def reference(q, k, v, pos, dtype, scale=SCALE, sums=False):
    """The torch composition of transformer.py:275-292 in `dtype` (as tests/vendor_ops.py: bilinear_attention): dict of s, P, vt,
    T = P v~ and F = (v~^T P) v~; with sums=True also ST = P |v~| and SF = |v~|^T P |v~|, the magnitudes behind T and F, and
    sig = scale sum_c |q_ic| |k_jc|, the magnitudes behind each score."""
    q, k, v, pos = (t.to(dtype) for t in (q, k, v, pos))
    s = (q @ k.transpose(-2, -1)) * scale
    P = s.softmax(dim=-1) * s.softmax(dim=-2)
    vt = vtilde(v, pos)
    out = {'s': s, 'P': P, 'vt': vt, 'T': P @ vt, 'F': (vt.transpose(-2, -1) @ P) @ vt}
    if sums:
        out['ST'] = P @ vt.abs()
        out['SF'] = vt.abs().transpose(-2, -1) @ out['ST']
        out['sig'] = (q.abs() @ k.abs().transpose(-2, -1)) * scale
    return out


def score_floor_T(s64, sig64, vt64):
    """Per-element floor of T = P v~ for every K2 forward kernel, the exact-f32 ones included, float64 (Z, N, 70):

        2^-20 S  +  ln2 2^-24 sum_j P_ij E_ij |v~_jb|,      E_ij = 2 sg_ij + sum_j' r_ij' sg_ij' + sum_i' c_i'j sg_i'j

    sg = sig log2(e) the sum of magnitudes behind a score in the kernels' log2 domain, r / c the softmax over keys / queries.
    A score is a 64-term sum held in an fp32 accumulator: whatever the operands, its accumulation error is taken as
    2^-24 sum_c |q_c k_c| scale: one rounding at the full magnitude of the terms (the split form's 12 and the exact form's 32
    dependent MFMA steps each round the running sum, so this is no worst case).  P = 2^(2 x_ij - lse_row_i - lse_col_j), and each of the two normalisers comes
    from ANOTHER pass over the scores (far_emm_pv_f16s: the row side takes acc through one fused multiply-add, the column statistics
    took fl(acc c1) in k_rowstats with the operands exchanged; far_emm_pv_f32 reads what far_dual_softmax_stats_f32 formed), so the
    errors of x_ij and of the normalisers do not cancel, not even where P ~ 1: |d log2 P_ij| <= 2^-24 E_ij, P moves by ln2 times that.
    The fp32 torch softmax subtracts the maximum from the very number it exponentiates, so that dev32 is exactly 0 where P ~ 1 (at N = 1
    everywhere) and cannot stand for this error."""
    sg = sig64 * (1.0 / math.log(2.0))
    r, c = s64.softmax(dim=-1), s64.softmax(dim=-2)
    E = 2.0 * sg + (r * sg).sum(dim=-1, keepdim=True) + (c * sg).sum(dim=-2, keepdim=True)
    av = vt64.abs()
    return FLOOR * ((r * c) @ av) + math.log(2.0) * 2.0 ** -24 * ((r * c * E) @ av)


def split_floor_T(s64, sig64, vt64):
    """Per-element floor of T = P v~ for the split-fp16 kernels (far_emm_pv_f16s), float64 (Z, N, 70): score_floor_T plus the resolution
    of the fp16 operands of the second contraction, derived from the number formats in emm_bilinear_f16s.hip, not from a measured error.

      2^-38 |v~_b|_1    p = 2^(2x - R_i - C_j + 15) <= 2^15 is held as fp16 hi + lo: below 2^-3 the lo part is subnormal, quantum 2^-24,
                        |p - hi - lo| <= 2^-25 (a p below 2^-25 is dropped whole: rows whose every P is below ~2^-39 come out 0).  With
                        T_ib = (2^-21 / rho_i) sum_j p_ij w_jb, w_jb = 64 v~_jb / g_j, and rho_i = sum_j 2^(x_ij - R_i), g_j = sum_i
                        2^(x_ij - C_j) both above 1/2 (R, C are the ceilings of the maxima):
                        |dT_ib| <= 2^-21 2 2^-25 64 2 sum_j |v~_jb| = 2^-38 |v~_b|_1.
      2^-31 (P g)_i     w is held the same way, |dw| <= 2^-25, i.e. |dv~_jb| <= 2^-31 g_j: |dT_ib| <= 2^-31 sum_j P_ij g_j.

    Both are absolute, about 1e-9 of max|T| at N <= 320: four decades under the old atol of 2e-5 max|T|."""
    x = s64 * (1.0 / math.log(2.0))
    P = s64.softmax(dim=-1) * s64.softmax(dim=-2)
    g = torch.exp2(x - torch.ceil(x.amax(dim=-2, keepdim=True))).sum(dim=-2)                   # (Z, N): column sums at the integer reference
    return score_floor_T(s64, sig64, vt64) + 2.0 ** -38 * vt64.abs().sum(dim=1, keepdim=True) + 2.0 ** -31 * (P @ g.unsqueeze(-1))


def floor_T(r64, split):
    return (split_floor_T if split else score_floor_T)(r64['s'], r64['sig'], r64['vt'])


def floor_F(r64, split):
    """F = v~^T T is an exact-fp32 contraction of T: the floor of T carried through it, |v~|^T floor_T."""
    return r64['vt'].abs().transpose(-2, -1) @ floor_T(r64, split)


def row_groups(n, rows=ROWS):
    return tuple((r, min(r + rows, n)) for r in range(0, n, rows))


def block_max(x, rgroups, cgroups):
    """max |x| over every (problem, row group, column group) block: (Z, len(rgroups), len(cgroups)) float64 on the CPU."""
    x = x.detach().abs().double().cpu()
    out = torch.empty(x.shape[0], len(rgroups), len(cgroups), dtype=torch.float64)
    for i, (r0, r1) in enumerate(rgroups):
        for j, (c0, c1) in enumerate(cgroups):
            out[:, i, j] = x[:, r0:r1, c0:c1].amax(dim=(1, 2))
    return out


def hidden_blocks(T64):
    """Boolean (Z, row groups, 3): the blocks of T whose largest entry is below HIDDEN max|T| -- invisible to a whole-tensor atol."""
    return block_max(T64, row_groups(T64.shape[1]), COL_GROUPS) < HIDDEN * float(T64.abs().max())


class BlockParityError(AssertionError):
    """Raised by check_blocks; .blocks lists the failing (z, (row0, row1), (col0, col1))."""

    def __init__(self, msg, blocks):
        super().__init__(msg)
        self.blocks = blocks


def check_blocks(name, got, r64, r32, floor, rgroups, cgroups, factor=FACTOR, floor_name='floor'):
    """The per-block rule: max_b |got - r64| <= max(factor max_b |r32 - r64|, max_b floor), `floor` the per-element floor
    (score_floor_T, or split_floor_T for the split-fp16 kernels).  Prints one '[parity] ...' line with the worst block (largest
    deviation / bar), its ratio and which term decided its bar, then raises BlockParityError naming every block that misses.  Returns
    (deviation, bar) of the worst block."""
    assert got.shape == r64.shape == r32.shape == floor.shape, (got.shape, r64.shape, r32.shape, floor.shape)
    if not bool(torch.isfinite(got).all()):
        raise BlockParityError(f'{name}: non-finite output', [])
    d = block_max(got.double() - r64, rgroups, cgroups)
    dev = factor * block_max(r32.double() - r64, rgroups, cgroups)
    flo = block_max(floor, rgroups, cgroups)
    bar = torch.maximum(dev, flo)
    ratio = d / bar.clamp_min(1e-300)
    ratio[(d == 0)] = 0.0
    z, ij = divmod(int(ratio.argmax()), ratio.shape[1] * ratio.shape[2])
    i, j = divmod(ij, ratio.shape[2])
    where = lambda z, i, j: f'(z {z}, rows {rgroups[i][0]}:{rgroups[i][1]}, cols {cgroups[j][0]}:{cgroups[j][1]})'
    term = f'{floor_name} decides' if flo[z, i, j] > dev[z, i, j] else f'{factor:g} x dev32'
    print(f'[parity] {name}: {ratio.numel()} blocks ({int((flo > dev).sum())} on the floor), worst {where(z, i, j)} kernel-vs-ref '
          f'{d[z, i, j]:.3e}  dev32 {dev[z, i, j] / factor:.3e}  floor {flo[z, i, j]:.3e}  bar {bar[z, i, j]:.3e}  ratio {ratio[z, i, j]:.2f} ({term})')
    idx = torch.nonzero(d > bar).tolist()
    if idx:
        bad = [(a, rgroups[b], cgroups[c]) for a, b, c in idx]
        lines = [f'{where(a, b, c)}: {d[a, b, c]:.3e} > {bar[a, b, c]:.3e}' for a, b, c in idx[:8]]
        raise BlockParityError(f'{name}: {len(bad)} of {ratio.numel()} blocks miss the per-block rule: ' + '; '.join(lines), bad)
    return float(d[z, i, j]), float(bar[z, i, j])


def check_T(name, got, r64, r32, split=False):
    """The rule on T (Z, N, 70); r64 from reference(..., sums=True).  split: the floor of the split-fp16 kernels (split_floor_T)."""
    return check_blocks(name + ' T', got, r64['T'], r32['T'], floor_T(r64, split), row_groups(got.shape[1]), COL_GROUPS,
                        floor_name='split floor' if split else 'fp32 floor')


def check_F(name, got, r64, r32, split=False):
    """The rule on F (Z, 70, 70)."""
    return check_blocks(name + ' F', got, r64['F'], r32['F'], floor_F(r64, split), COL_GROUPS, COL_GROUPS,
                        floor_name='split floor' if split else 'fp32 floor')
