"""The K2 parity cases and checker (tests/emm_inputs.py) on the float64 reference alone, without a GPU: every committed seed really
puts K2 into the regime its name promises, and the per-block rule catches an error that the whole-tensor assertion of
tests/test_emm_gpu.py (atol 2e-5 max|T|, rtol 1e-4) accepts."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import emm_inputs as ei

Z = 2


@functools.lru_cache(maxsize=None)
def _ref(N, regime):
    q, k, v, pos = ei.emm_case(Z, N, regime, ei.case_seed(N, regime))
    return ei.reference(q, k, v, pos, torch.float64, sums=True), ei.reference(q, k, v, pos, torch.float32)


def test_cases_are_seeded_and_device_agnostic():
    a = ei.emm_case(Z, 65, 'shifted', 7)
    b = ei.emm_case(Z, 65, 'shifted', 7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    q, k, v, pos = a
    assert q.shape == k.shape == v.shape == (Z, 65, 64) and pos.shape == (65, 6)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in a)
    assert float(pos.min()) < -0.5 and float(pos.max()) > 0.5 and not bool((pos[:, 5] == 1).all())       # signed, no constant column
    assert not torch.equal(ei.emm_case(Z, 65, 'shifted', 8)[0], q)


@pytest.mark.parametrize('N', [n for n in ei.KEY_COUNTS if n >= 33])
def test_negative_scores_are_far_below_the_padding_score(N):
    """A zero-padded key or query scores 0: with every real score <= -10 it would win any unmasked maximum by e^10."""
    assert float(_ref(N, 'negative')[0]['s'].max()) <= -10.0


@pytest.mark.parametrize('N', [n for n in ei.KEY_COUNTS if n >= 33])
def test_shifted_rows_peak_at_the_last_key(N):
    s = _ref(N, 'shifted')[0]['s']
    assert float((s.argmax(dim=-1) == N - 1).double().mean()) >= 0.95


@pytest.mark.parametrize('N', [n for n in ei.KEY_COUNTS if n >= 129])
def test_shifted_hides_blocks_from_a_whole_tensor_tolerance(N):
    hid = ei.hidden_blocks(_ref(N, 'shifted')[0]['T'])
    assert hid.numel() == Z * ((N + 31) // 32) * 3
    assert int(hid.sum()) >= 0.10 * hid.numel(), (int(hid.sum()), hid.numel())


@pytest.mark.parametrize('N', [n for n in ei.KEY_COUNTS if n >= 33])
def test_peaked_scores_pass_100(N):
    """(N = 1 is one score per problem, |s| ~ 36 |randn|: no claim there.)"""
    assert float(_ref(N, 'peaked')[0]['s'].abs().max()) >= 100.0


@pytest.mark.parametrize('N', ei.KEY_COUNTS)
@pytest.mark.parametrize('regime', ei.REGIMES)
def test_fp32_reference_meets_its_own_rule(N, regime):
    """The checker accepts the fp32 composition itself (its deviation is dev32 <= 3 dev32) and prints its line."""
    r64, r32 = _ref(N, regime)
    ei.check_T(f'cpu fp32 {regime} N{N}', r32['T'], r64, r32)
    ei.check_F(f'cpu fp32 {regime} N{N}', r32['F'], r64, r32)
    assert torch.isfinite(r64['T']).all() and torch.isfinite(r64['F']).all()


@pytest.mark.parametrize('N', [129, 221, 320])
def test_checker_has_teeth_where_the_old_assertion_has_none(N):
    """A relative error of 1e-4 planted in one hidden block (the largest of them) of the fp32 reference's T: the per-block rule raises
    and names that block; the whole-tensor assertion of tests/test_emm_gpu.py accepts the same tensor.  The margin is that of the
    derived floor alone: floor_b / max_b |T| is asserted below 1e-4 / 2 for the fp32 floor at every N, and for the split floor at
    N = 221 and 320.  At N = 129 the largest hidden block lies at 9e-8 max|T|, where the absolute fp16-resolution terms of the
    split floor (2^-38 |v~_b|_1 ~ 4e-10) are 3e-3 of the block: there the planted error is the smallest power of ten at least twice
    that (1e-2), still two decades under the 10 % a whole-tensor tolerance lets through."""
    r64, r32 = _ref(N, 'shifted')
    hid = ei.hidden_blocks(r64['T'])
    rgs = ei.row_groups(N)
    bm = ei.block_max(r64['T'], rgs, ei.COL_GROUPS)
    z, i, j = (int(t) for t in torch.nonzero(hid & (bm == bm[hid].max()))[0])
    rg, cg = rgs[i], ei.COL_GROUPS[j]
    Tref = r64['T'].numpy()
    for split in (False, True):
        need = float(ei.block_max(ei.floor_T(r64, split), rgs, ei.COL_GROUPS)[z, i, j] / bm[z, i, j])
        rel = 1e-4 if 2 * need <= 1e-4 else 10.0 ** math.ceil(math.log10(2 * need))
        print(f'[teeth] shifted N{N} {"split" if split else "fp32"} floor: floor_b / max_b|T| = {need:.2e} in the largest hidden block '
              f'(at {float(bm[z, i, j] / bm.max()):.1e} max|T|); planted {rel:g}')
        assert rel == 1e-4 or (split and N == 129 and rel <= 1e-2), (split, N, need)
        bad = r32['T'].clone()
        bad[z, rg[0]:rg[1], cg[0]:cg[1]] *= 1.0 + rel
        with pytest.raises(ei.BlockParityError) as exc:
            ei.check_T(f'cpu planted {rel:g} N{N}', bad, r64, r32, split=split)
        assert exc.value.blocks == [(z, rg, cg)]
        assert f'z {z}, rows {rg[0]}:{rg[1]}, cols {cg[0]}:{cg[1]}' in str(exc.value)
        np.testing.assert_allclose(bad.numpy(), Tref, atol=2e-5 * np.abs(Tref).max(), rtol=1e-4)      # the old assertion: passes
    with pytest.raises(ei.BlockParityError):                                                          # non-finite output is a miss
        ei.check_T('cpu nan', torch.full_like(bad, float('nan')), r64, r32)
