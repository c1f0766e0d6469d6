"""attention_decode where a split walks MORE THAN ONE 128-key step (`while (ks < kend)` of seg_attn_decode_kernel turns
twice or more): the rescale against a running max carried over, the prefetch once it is live, the V tile overwritten, the
start rule with lo_step > kbeg, `kend = hi` cutting a split, the single launch with S > 128 and the item stride with
splits.  The yardsticks, `run` and `check` are test_gpu_attention_decode's, unchanged; test_gpu_attention_decode.py keeps
every split at one step.  Every case table stands at module level next to the plan it expects and is listed in PREMISES;
tests/test_attention_decode_walk_premises.py checks those without a GPU, and the GPU tests read the plan off the trace."""
import pytest
import torch

import attention_band_util as U
from gpu_util import dispatch_trace
from test_gpu_attention import build, padding
from test_gpu_attention_decode import check, draw_case, kw, run

pytestmark = pytest.mark.gpu

STEP, COLS = 128, 32                                            # rua_attention_decode_plan.h: DEC_STEP, DEC_COLS


def walk_stats(ql, kl, G, mask, chunk, n_split):
    """The bounds of the kernel's key loop, restated: (the most turns any wave takes in any work item, whether a walked
    item starts from lo_step > kbeg, whether `hi` cuts a walked item short of its split's end)."""
    align, left, right = mask
    most, late, cut = 0, False, False
    for T, S in zip(ql, kl):
        shift = S - T if align == 'end' else 0
        for cb in range(-(-T * G // COLS)):
            a, c = cb * COLS // G + shift, min((cb * COLS + COLS - 1) // G, T - 1) + shift
            lo = 0 if left is None or a <= left else a - left
            hi = S if right is None or right >= S - 1 - c else c + right + 1
            for sp in range(n_split):
                kbeg = sp * chunk
                if n_split > 1 and kbeg >= S:
                    continue
                whole, lo_step = min(kbeg + chunk, S), lo // STEP * STEP
                kend = min(whole, hi)
                for wv in range(4):
                    ks = max(kbeg, lo_step) + 32 * wv
                    ks += STEP if ks + 31 < lo else 0
                    turns = max(0, -(-(kend - ks) // STEP))
                    most, late, cut = max(most, turns), late or (turns > 0 and lo_step > kbeg), cut or (turns > 0 and hi < whole)
    return most, late, cut


PREMISES = []   # (name, ql, kl, heads, D, mask, kv_chunk in, the plan (kv_chunk, n_split), the least `most turns` claimed)


def premise(name, ql, kl, heads, D, mask, chunk_in, plan, turns=2):
    PREMISES.append((name, ql, kl, heads, D, mask, chunk_in, plan, turns))
    return plan


def run_planned(plan, *args, **kwargs):
    """`run`, after reading the plan off the stream: one walk record with this chunk and these splits, and the combine
    kernel exactly when the keys are split."""
    with dispatch_trace() as tr:
        got = run(*args, **kwargs)
    walks = tr.matching('seg_attn_decode_kernel')
    assert len(walks) == 1 and {f'chunk={plan[0]}', f'splits={plan[1]}'} <= set(walks[0].split()), tr.records
    assert len(tr.matching('seg_attn_decode_combine_kernel')) == (plan[1] > 1), tr.records
    return got, walks[0]


# ------------------------------------------------------------------ 1. step and sub-tile edges of a long split
KL = [0, 1, 128, 129, 255, 256, 257, 300, 383, 384, 385, 513, 640, 700]
QL = [1, 0, 4, 32, 2, 1, 7, 1, 1, 3, 32, 1, 5, 1]
EDGE_PLANS = {256: (256, 3), 384: (384, 2), 768: (768, 1)}     # 768: the single launch
# ('start', 150, 70) keeps every query inside keys 0 .. 101: one step, `hi` cutting split 0 and the later splits writing
# empty states; the other three walk two steps or more
MASKS = {('end', None, 0): 2, ('end', 200, 0): 2, ('start', None, None): 2, ('start', 150, 70): 1}
EDGES = [(64, U.BF16, hd, m, ch) for hd in ((4, 4), (4, 2), (8, 1)) for m in MASKS for ch in EDGE_PLANS]
EDGES += [c for c in ((D, dt, (8, 1), ('end', 200, 0), ch) for D in (32, 64, 128) for dt in (U.BF16, U.F16) for ch in (256, 768))
          if c not in EDGES]
for D_, dt_, hd_, m_, ch_ in EDGES:
    premise(f'edges D={D_} {hd_} {m_} {ch_}', QL, KL, hd_, D_, m_, ch_, EDGE_PLANS[ch_], MASKS[m_])


@pytest.mark.parametrize('D,dtype,heads,mask,kv_chunk', EDGES, ids=str)
def test_step_and_sub_tile_edges_of_a_long_split_forward_and_lse(D, dtype, heads, mask, kv_chunk):
    q, k, v = draw_case(QL, KL, heads, D, dtype, 10 * D + 3)
    got, _ = run_planned(EDGE_PLANS[kv_chunk], 'LC' if D == 32 else 'CC', q, QL, k, v, KL, kv_chunk=kv_chunk, **kw(*mask))
    key = f'walk {str(dtype)[6:]} D={D} heads={heads[0]}/{heads[1]} {mask[0]} {mask[1]} {mask[2]} chunk={kv_chunk}'
    assert bool(check(key, got, q, QL, k, v, KL, mask, None, dtype, kv_chunk).any()), 'a query without a visible key'


# ------------------------------------------------------------------ 2. a running max that moves, planted
PT, PS, PHEADS, PD, PMASK = 2, 600, (4, 2), 64, ('end', None, 0)
PLANT_PLANS = {128: (128, 5), 256: (256, 3), 768: (768, 1)}    # 128: one step a split — the combine's factor moves
PLANT_AT = {5: 'step 0 wave 0', 100: 'step 0 wave 3', 300: 'step 2', 500: 'the last full step', 599: 'the partial last sub-tile'}
PLANT_SEED = 43                                                 # one whose reference rows clear the premise below, both types
for ch_, plan_ in PLANT_PLANS.items():
    premise(f'planted {ch_}', [PT], [PS], PHEADS, PD, PMASK, ch_, plan_, 2 if ch_ > STEP else 1)


def planted(dtype, at):
    """q, k, v of one sequence whose key `at` is 1.25 q[t0, hk G] for each kv head hk (a scaled score near 10 against
    N(0, 1)) and whose value row `at` is all 3.0; t0 is the last query, which sees every key."""
    q, k, v = draw_case([PT], [PS], PHEADS, PD, dtype, PLANT_SEED)
    G = PHEADS[0] // PHEADS[1]
    for hk in range(PHEADS[1]):
        k[at, hk] = (1.25 * q[PT - 1, hk * G].float()).to(dtype)
        v[at, hk] = 3.0
    return q, k, v


def planted_reference(q, k, v, dtype, at):
    """Per kv head hk: (the float64 weight of the planted key for query t0 and head hk G, that head's float64 output row,
    whether the row stays further from a one-decimal rounding edge than its error bound) — from the yardstick alone."""
    G, t0 = PHEADS[0] // PHEADS[1], PT - 1
    (want, *_), (b_out, *_), _ = U.reference(q, [PT], k, v, [PS], torch.zeros_like(q), PMASK, None, dtype)
    res = []
    for hk in range(PHEADS[1]):
        w = (PD ** -0.5 * k[:, hk].to(U.F64) @ q[t0, hk * G].to(U.F64)).softmax(0)[at]
        row = want[t0, hk * G]
        edge = 0.05 - (row * 10 - (row * 10).round()).abs() / 10
        res.append((float(w), row, bool((edge > b_out[t0, hk * G] * (1 + 2.0 ** -10)).all())))
    return res


@pytest.mark.parametrize('at', sorted(PLANT_AT))
@pytest.mark.parametrize('dtype', [U.BF16, U.F16], ids=str)
def test_a_planted_key_moves_the_running_max(dtype, at):
    q, k, v = planted(dtype, at)
    ref = planted_reference(q, k, v, dtype, at)
    assert all(w > 0.5 and clear for w, _, clear in ref), 'the planted key carries the row, away from a rounding edge'
    for kv_chunk, plan in PLANT_PLANS.items():
        got, _ = run_planned(plan, 'CC', q, [PT], k, v, [PS], kv_chunk=kv_chunk, **kw(*PMASK))
        for hk, (_, row, _) in enumerate(ref):
            h = hk * (PHEADS[0] // PHEADS[1])
            assert torch.equal(got[0][PT - 1, h].to(U.F64).round(decimals=1), row.round(decimals=1)), (kv_chunk, h, got[0][PT - 1, h], row)
        check(f'walk planted {str(dtype)[6:]} at={at} chunk={kv_chunk}', got, q, [PT], k, v, [PS], PMASK, None, dtype, kv_chunk)


# ------------------------------------------------------------------ 3. the plan's own choices on the stream
SQL, SKL, SHEADS = [1] * 8, [700, 129, 0, 257, 31, 512, 385, 64], (8, 8)
STREAM = [(8, 64, U.BF16, (256, 3)), (16, 128, U.F16, (384, 2)), (32, 32, U.BF16, (768, 1))]   # tiles, D, dtype, the plan
for n_, D_, dt_, plan_ in STREAM:
    premise(f'stream x{n_}', SQL * n_, SKL * n_, SHEADS, D_, ('end', None, 0), None, plan_)


@pytest.mark.parametrize('tiles,D,dtype,plan', STREAM, ids=str)
def test_the_plan_chooses_longer_chunks_as_the_batch_grows(tiles, D, dtype, plan):
    q, k, v = draw_case(SQL, SKL, SHEADS, D, dtype, 21)
    got, _ = run_planned(plan, 'CC', q.repeat(tiles, 1, 1), SQL * tiles, k.repeat(tiles, 1, 1), v.repeat(tiles, 1, 1), SKL * tiles)
    n = sum(SQL)
    for i in (0, 1, tiles - 1):
        assert torch.equal(got[0][i * n:(i + 1) * n], got[0][:n]) and torch.equal(got[1][i * n:(i + 1) * n], got[1][:n]), i
    key = f'walk stream B={8 * tiles} {str(dtype)[6:]} D={D} chunk={plan[0]}'
    assert bool(check(key, [g[:n] for g in got], q, SQL, k, v, SKL, ('end', None, 0), None, dtype, plan[0]).any())


# ------------------------------------------------------------------ 4. more items than the grid, with splits and long walks
GQL = [1, 4, 0, 2, 3, 1, 4, 1, 2, 1, 3, 1, 4, 2]
GKL = [600, 129, 57, 0, 513, 256, 385, 31, 600, 128, 300, 257, 1, 470]
GTILES, GHEADS, GD, GCHUNK, GWINDOW = 100, (4, 1), 32, 256, 300     # 1 400 sequences x 1 kv head x 3 splits > 4 096 workgroups
GPLAN = premise('grid', GQL * GTILES, GKL * GTILES, GHEADS, GD, ('end', GWINDOW, 0), GCHUNK, (256, 3))


def test_more_work_items_than_the_grid_with_splits_and_long_walks():
    q, k, v = draw_case(GQL, GKL, GHEADS, GD, U.F16, 60)
    got, walk = run_planned(GPLAN, 'CP', q.repeat(GTILES, 1, 1), GQL * GTILES, k.repeat(GTILES, 1, 1), v.repeat(GTILES, 1, 1),
                            GKL * GTILES, kv_chunk=GCHUNK, window=GWINDOW)
    assert {'heads=4', 'kvheads=1', f'left={GWINDOW}', 'right=0', 'end=1', 'splits=3', 'grid=4096'} <= set(walk.split()), walk
    n = sum(GQL)
    for i in (0, 1, 50, GTILES - 1):
        assert torch.equal(got[0][i * n:(i + 1) * n], got[0][:n]) and torch.equal(got[1][i * n:(i + 1) * n], got[1][:n]), i
    assert bool(check('walk large batch', [g[:n] for g in got], q, GQL, k, v, GKL, ('end', GWINDOW, 0), None, U.F16, GCHUNK).any())


# ------------------------------------------------------------------ 5. layouts and storage on a long walk
PQ, PK = [30, 0, 5, 32], [515, 3, 0, 257]
PAIR_PLANS = {256: (256, 3), 768: (768, 1)}
for ch_, plan_ in PAIR_PLANS.items():
    premise(f'pairs {ch_}', PQ, PK, (4, 2), 32, ('end', None, 0), ch_, plan_)


@pytest.mark.parametrize('kv_chunk', sorted(PAIR_PLANS))
def test_layouts_and_padding_storage_on_a_long_walk(kv_chunk):
    q, k, v = draw_case(PQ, PK, (4, 2), 32, U.F16, 8)
    base, _ = run_planned(PAIR_PLANS[kv_chunk], 'CC', q, PQ, k, v, PK, kv_chunk=kv_chunk)
    check(f'walk pairs chunk={kv_chunk}', base, q, PQ, k, v, PK, ('end', None, 0), None, U.F16, kv_chunk)
    for pair, host in [(p, True) for p in ('PL', 'RP', 'LR', 'PP')] + [('CC', False)]:
        for got, exp, what in zip(run(pair, q, PQ, k, v, PK, host=host, kv_chunk=kv_chunk), base, ('out', 'lse')):
            assert torch.equal(got, exp), (pair, host, what)
    # NaN in the padding rows of K and V: attn_row answers -1 past the end, so no load — not the prefetch of the step
    # past kend either — may bring one in (a masked score would be selected away, 0 x NaN in P V would not)
    qc = build('C', q, PQ)
    for kind in 'LR':
        kc, vc = build(kind, k, PK), build(kind, v, PK)
        for z in (kc, vc):
            z.data[padding(z)] = float('nan')
            assert bool(z.data.isnan().any())
        out, lse = qc.attention_decode(kc, vc, return_lse=True, kv_chunk=kv_chunk)
        assert torch.equal(out.data.cpu(), base[0]) and torch.equal(lse.cpu(), base[1]), kind


# ------------------------------------------------------------------ 6. the band's two edges on a long walk
BT, BS, BW = 3, 700, 100
BAND_PLANS = {256: (256, 3), 384: (384, 2), 1024: (1024, 1)}   # 384: lo in the step after split 1's first; 1024: mid-walk
for ch_, plan_ in BAND_PLANS.items():
    premise(f'band {ch_}', [BT], [BS], (2, 1), 64, ('end', BW, 0), ch_, plan_, 1)   # a band of 103 keys: one turn a wave


@pytest.mark.parametrize('kv_chunk', sorted(BAND_PLANS))
def test_rows_see_their_band_and_nothing_else_on_a_long_walk(kv_chunk):
    T, S, W = BT, BS, BW
    q, k, v = draw_case([T], [S], (2, 1), 64, U.BF16, 5)
    other_k, other_v = U.draw([S], 1, 64, U.BF16, 55), U.draw([S], 1, 64, U.BF16, 56)
    zq = build('C', q, [T])
    att = lambda k_, v_: zq.attention_decode(build('C', k_, [S]), build('C', v_, [S]), causal=True, window=W, align='end',  # noqa: E731
                                             kv_chunk=kv_chunk).data
    with dispatch_trace() as tr:
        base = att(k, v)
    plan = BAND_PLANS[kv_chunk]
    assert tr.matching(f'seg_attn_decode_kernel left={W} right=0 end=1 chunk={plan[0]} splits={plan[1]}'), tr.records
    assert len(tr.matching('seg_attn_decode_combine_kernel')) == (plan[1] > 1), tr.records
    for t in range(T):
        lo, hi = t + S - T - W, t + S - T                       # the first and the last visible key of row t
        outside = torch.ones(S, dtype=torch.bool)
        outside[lo:hi + 1] = False
        assert torch.equal(att(torch.where(outside[:, None, None], other_k, k), torch.where(outside[:, None, None], other_v, v))[t], base[t]), t
        for edge in (lo, hi):
            k2 = k.clone()
            k2[edge] = other_k[edge]
            assert not torch.equal(att(k2, v)[t], base[t]), (t, edge)


def test_zz_report():
    for key in sorted(k for k in U.REPORT if k.startswith('decode walk ')):
        print(f'attention report: {key} {U.REPORT[key]:.4f}')
