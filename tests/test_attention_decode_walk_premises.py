"""The premises of tests/test_gpu_attention_decode_walk.py, checked without a GPU: every case table there gets the plan
it states from rua_attention_decode_plan (a pure host function), and the kernel's key loop — its bounds restated by
walk_stats — turns at least twice for some wave wherever the case claims a walk of more than one step.  A case whose plan
collapsed to one step a split would test again what test_gpu_attention_decode.py already tests: it fails here instead."""
import pytest

from torchrua_amd import _ops
from test_gpu_attention_decode_walk import BAND_PLANS, EDGE_PLANS, KL, MASKS, PREMISES, QL, STEP, walk_stats


@pytest.mark.parametrize('name,ql,kl,heads,D,mask,chunk_in,plan,turns', PREMISES, ids=[p[0] for p in PREMISES])
def test_the_plan_and_the_steps_of_every_case(name, ql, kl, heads, D, mask, chunk_in, plan, turns):
    assert _ops.attention_decode_plan(len(ql), *heads, D, max(ql), max(kl), chunk_in)[:2] == plan
    most = walk_stats(ql, kl, heads[0] // heads[1], mask, *plan)[0]
    assert most >= turns and (turns >= 2 or most == 1), (most, turns)
    if mask[1] is None and mask[2] is None:                     # no band: the longest split, in steps
        assert most == max(-(-min(plan[0], S - sp * plan[0]) // STEP) for T, S in zip(ql, kl) if T for sp in range(plan[1])
                           if sp * plan[0] < S)


def test_the_issue_table_of_plans():
    for args, plan in [((14, 8, 2, 64, 32, 700, 256), (256, 3)), ((14, 8, 2, 64, 32, 700, 384), (384, 2)),
                       ((14, 8, 2, 64, 32, 700, 768), (768, 1)), ((64, 8, 8, 64, 1, 700, None), (256, 3)),
                       ((128, 8, 8, 64, 1, 700, None), (384, 2)), ((256, 8, 8, 64, 1, 700, None), (768, 1)),
                       ((1400, 4, 1, 32, 4, 600, 256), (256, 3))]:
        assert _ops.attention_decode_plan(*args)[:2] == plan, args
    assert 1400 * 1 * 1 * 3 > 4096                              # the items of the last one: more than the grid


@pytest.mark.parametrize('chunk', sorted(EDGE_PLANS))
def test_the_windows_reach_the_start_rule_and_the_cut(chunk):
    """('end', 200, 0) starts some walked split from lo_step > kbeg at every chunk; both windows let `hi` cut a walked
    split short of its end (('end', 200, 0): the column blocks below the last, eight heads a group)."""
    plan = EDGE_PLANS[chunk]
    for G in (1, 2, 8):
        most, late, cut = walk_stats(QL, KL, G, ('end', 200, 0), *plan)
        assert most >= 2 and late and cut == (G > 1), (G, most, late, cut)
        assert walk_stats(QL, KL, G, ('start', 150, 70), *plan) == (MASKS[('start', 150, 70)], False, True)


def test_the_band_test_starts_after_a_splits_first_step():
    assert walk_stats([3], [700], 2, ('end', 100, 0), *BAND_PLANS[384])[1]     # lo_step = 512 > kbeg = 384
    assert walk_stats([3], [700], 2, ('end', 100, 0), *BAND_PLANS[1024])[1]    # the single launch: lo_step > 0
    assert not walk_stats([3], [700], 2, ('end', 100, 0), *BAND_PLANS[256])[1]  # 256: lo_step is split 2's own start
