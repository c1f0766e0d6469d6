"""Per-sequence edit distance and alignment on the GPU against the yardstick of tests/edit_util.py, bit for bit: the column
buckets and both kernel forms, chains that cross lane, wave and R boundaries, ties, 64-bit tokens, the 4 x 4 pairs of
layouts, batches larger than the launch, degenerate batches, the read-backs and the library's own CTC collapse."""
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _meta
import edit_util as U
from edit_util import I64
from gpu_util import DEV, dispatch_trace

pytestmark = pytest.mark.gpu

KINDS = ('C', 'L', 'P', 'R')


# ------------------------------------------------------------------ helpers
def build(kind, x, lens_host, host_sizes=True):
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def padding_mask(z):
    T = z.data.size(1)
    pos, n = torch.arange(T, device=DEV).unsqueeze(0), z.token_sizes.to(DEV).unsqueeze(1)
    return pos >= n if isinstance(z, ta.L) else pos < T - n


def containers(hyps, refs, kinds='CC'):
    return (build(kinds[0], U.cat_of(hyps).to(DEV), U.lens_of(hyps)), build(kinds[1], U.cat_of(refs).to(DEV), U.lens_of(refs)))


def run(hyps, refs, kinds='CC'):
    """Want-shaped results of the GPU (positions in cat form), after the checks every call must pass."""
    z, rf = containers(hyps, refs, kinds)
    B = len(hyps)
    dist = z.edit_distance(rf)
    assert dist.dtype == I64 and dist.shape == (B,) and not dist.requires_grad
    al = z.edit_align(rf)
    assert isinstance(al, ta.SeqEdit) and type(al.positions) is type(z)
    assert al.positions.data.dtype == I64 and al.positions.data.shape == z.data.shape
    for t in al[1:]:
        assert t.dtype == I64 and t.shape == (B,)
    if isinstance(z, ta.P):
        assert al.positions.batch_sizes is z.batch_sizes and al.positions.unsorted_indices is z.unsorted_indices
        assert al.positions.sorted_indices is z.sorted_indices
    else:
        assert al.positions.token_sizes is z.token_sizes
    if kinds[0] in 'LR' and z.data.numel():
        assert bool((al.positions.data[padding_mask(z)] == 0).all()), 'padding rows of positions are zeros'
    assert torch.equal(dist, al.distance), 'the distance-only launch and the alignment launch agree'
    pos = al.positions.cat().data if kinds[0] != 'C' else al.positions.data
    return U.Want(pos.cpu(), *(t.cpu() for t in al[1:]))


def check(hyps, refs, kinds='CC', want=None):
    got = run(hyps, refs, kinds)
    want = U.want_of(hyps, refs) if want is None else want
    for g, w, what in zip(got, want, U.Want._fields):
        assert torch.equal(g, w), (kinds, what)
    return got


def form_of(s_max):
    return 'form=workgroup' if U.bucket(s_max) == 'WG' else f'form=lanes R={U.bucket(s_max)[1:]}'


# ------------------------------------------------------------------ the column buckets and both forms
EDGES = (0, 1, 63, 64, 65, 128, 129, 256, 257, 512, 513, 2047, 2048)


@pytest.mark.parametrize('s_max', EDGES)
def test_bucket_edges(s_max):
    hyps, refs = U.edge_case(s_max)
    with dispatch_trace() as tr:
        check(hyps, refs)
    assert tr.matching(f'seg_edit_forward_kernel {form_of(s_max)} S_max={s_max} codes=0'), tr.records
    if s_max:
        assert tr.matching(f'seg_edit_forward_kernel {form_of(s_max)} S_max={s_max} codes=1'), tr.records
    assert 'seg_edit_backtrace_kernel' in tr.kernels


def test_ref_of_2049_tokens_is_refused():
    y = torch.ones(2049, dtype=I64, device=DEV)
    z = ta.with_host_sizes(torch.zeros(4, dtype=I64, device=DEV), torch.tensor([4]))
    for rf in (ta.with_host_sizes(y, torch.tensor([2049])), ta.C(y, torch.tensor([2049], device=DEV))):
        with pytest.raises(ta.RuaError, match='`ref` has 2049 tokens'):
            z.edit_distance(rf)
        with pytest.raises(ta.RuaError, match='`ref` has 2049 tokens'):
            z.edit_align(rf)
    # the limit is asymmetric: the same long sequence is a fine hyp
    long_hyp = ta.with_host_sizes(y, torch.tensor([2049]))
    assert z.edit_distance(z).tolist() == [0] and long_hyp.edit_distance(z).tolist() == [2049]


# ------------------------------------------------------------------ carry paths
@pytest.mark.parametrize('s_max', (130, 600))
def test_carry_paths_across_lanes_waves_and_registers(s_max):
    ref = U.draw(s_max, 50, s_max)
    other = U.draw(s_max, 50, s_max + 1) + 100                 # a disjoint alphabet
    long = U.draw(s_max + 7, 50, 3)
    hyps = [ref[40:41], long, ref[:s_max - 9], ref[11:], ref[5:s_max - 6], ref.clone(), other,
            torch.cat([ref[:s_max // 2], ref[s_max // 2 + 1:]])]
    refs = [ref, long[20:21], ref, ref, ref, ref, ref, ref]
    got = check(hyps, refs)
    # a left chain across the whole team; an up chain; prefix, suffix, interior; identical; disjoint; one deletion
    assert got.distance.tolist() == [s_max - 1, s_max + 6, 9, 11, 11, 0, s_max, 1]
    assert got.deletions.tolist()[:1] == [s_max - 1] and got.insertions.tolist()[1] == s_max + 6
    assert got.substitutions.tolist()[6] == s_max


# ------------------------------------------------------------------ ties
@pytest.mark.parametrize('alphabet', (1, 2, 3))
def test_ties_follow_the_backtrace_rule(alphabet):
    gen = torch.Generator().manual_seed(alphabet)
    hyps, refs = [], []
    for k in range(24):
        T, S = (int(v) for v in torch.randint(0, 90 if k % 3 else 12, (2,), generator=gen))
        hyps.append(U.draw(T, alphabet, 10 * k + alphabet))
        refs.append(U.draw(S, alphabet, 10 * k + alphabet + 5))
    check(hyps, refs)
    hyps.append(U.draw(140, alphabet, 7))
    refs.append(U.draw(520, alphabet, 8))                       # ... and in the workgroup form
    check(hyps, refs)


# ------------------------------------------------------------------ 64-bit tokens
def test_tokens_are_compared_as_64_bit_values():
    big, low = 2 ** 63 - 1, -2 ** 63
    a = torch.tensor([5, 5 + 2 ** 32, -1, big, low, 7 - 2 ** 40, 0], dtype=I64)
    b = torch.tensor([5 + 2 ** 32, 5, -1 + 2 ** 32, big, low, 7, 2 ** 32], dtype=I64)      # differ in the high words only
    hyps, refs = [a, a, b[:3], torch.tensor([big, low], dtype=I64)], [b, a, a[:3], torch.tensor([low, big], dtype=I64)]
    got = check(hyps, refs)
    assert got.distance.tolist() == [5, 0, 3, 2] and got.substitutions.tolist()[0] == 5


# ------------------------------------------------------------------ the same bits in every bucket and both forms
def test_same_bits_in_every_bucket_and_form():
    hyps, refs = U.edge_case(40, alphabet=3)
    want = check(hyps, refs)
    n = int(U.lens_of(hyps).sum())
    for filler in (100, 200, 400, 700, 2048):
        got = run(hyps + [U.draw(9, 3, 1)], refs + [U.draw(filler, 3, filler)])
        assert torch.equal(got.positions[:n], want.positions), filler
        for g, w, what in zip(got[1:], want[1:], U.Want._fields[1:]):
            assert torch.equal(g[:-1], w), (filler, what)


# ------------------------------------------------------------------ the 4 x 4 pairs of layouts
def test_all_sixteen_pairs_of_layouts_give_the_same_bits():
    hyps = [U.draw(n, 4, 40 + n) for n in (9, 0, 70, 3, 12, 1)]
    refs = [U.draw(n, 4, 80 + n) for n in (7, 5, 66, 0, 12, 130)]
    want = U.want_of(hyps, refs)
    for a in KINDS:
        for b in KINDS:
            check(hyps, refs, a + b, want)
    # device-only lengths on both sides give the same bits as well
    z = build('L', U.cat_of(hyps).to(DEV), U.lens_of(hyps), False)
    rf = build('C', U.cat_of(refs).to(DEV), U.lens_of(refs), False)
    assert torch.equal(z.edit_distance(rf).cpu(), want.distance)
    assert torch.equal(ta.edit_align(z, rf).positions.cat().data.cpu(), want.positions)


def test_segment_form_equals_the_container_form():
    hyps, refs = U.edge_case(65)
    z, rf = containers(hyps, refs)
    seg = ta.segment_edit_distance(z.data, U.lens_of(hyps).to(DEV), rf.data, U.lens_of(refs).to(DEV))
    assert seg.dtype == I64 and torch.equal(seg, z.edit_distance(rf)) and torch.equal(seg.cpu(), U.want_of(hyps, refs).distance)


# ------------------------------------------------------------------ more sequences than the launch has teams
@pytest.mark.parametrize('form', ['lanes', 'workgroup'])
def test_more_sequences_than_the_launch_has_teams(form):
    POOL, TILES = 100, 43                                       # 4 300 pairs > 1 024 workgroups x 4 teams
    gen = torch.Generator().manual_seed(8)
    lens = torch.randint(0, 7, (2, POOL), generator=gen)
    hyps = [U.draw(int(n), 3, 300 + k) for k, n in enumerate(lens[0])]
    refs = [U.draw(int(n), 3, 600 + k) for k, n in enumerate(lens[1])]
    pool = U.want_of(hyps, refs)                                # (a pair does not depend on its neighbours)
    hyps, refs = hyps * TILES, refs * TILES
    want = U.Want(pool.positions.repeat(TILES), *(t.repeat(TILES) for t in pool[1:]))
    if form == 'workgroup':                                     # one long ref in the middle, against a hyp of 2
        b = 2050
        refs[b] = U.draw(600, 3, 9)
        one = U.want_of(hyps[b:b + 1], refs[b:b + 1])
        start = int(U.lens_of(hyps[:b]).sum())
        pos = want.positions.clone()
        pos[start:start + one.positions.numel()] = one.positions
        rest = []
        for w, o in zip(want[1:], one[1:]):
            w = w.clone()
            w[b] = o[0]
            rest.append(w)
        want = U.Want(pos, *rest)
    with dispatch_trace() as tr:
        check(hyps, refs, 'CC', want)
    assert tr.matching(f'seg_edit_forward_kernel form={form} grid=1024 codes=1'), tr.records
    assert tr.matching(f'seg_edit_forward_kernel form={form} grid=1024 codes=0'), tr.records


# ------------------------------------------------------------------ degenerate batches
def test_degenerate_batches():
    none = torch.zeros(0, dtype=I64)
    some = [U.draw(n, 3, n) for n in (4, 1, 70)]
    for kinds in ('CC', 'LR', 'PC', 'RP'):
        got = check([none] * 3, some, kinds)                    # all hyps empty: deletions
        assert got.distance.tolist() == got.deletions.tolist() == [4, 1, 70] and got.positions.numel() == 0
        got = check(some, [none] * 3, kinds)                    # all refs empty: insertions, every position -1
        assert got.distance.tolist() == got.insertions.tolist() == [4, 1, 70] and bool((got.positions == -1).all())
        got = check([none] * 3, [none] * 3, kinds)
        assert got.distance.tolist() == [0, 0, 0]
    # B = 0
    z = ta.with_host_sizes(torch.zeros(0, dtype=I64, device=DEV), torch.zeros(0, dtype=I64))
    for a in (z, z.left(0), z.right(0)):
        for b in (z, z.left(0)):
            assert a.edit_distance(b).shape == (0,) and a.edit_distance(b).dtype == I64
            al = a.edit_align(b)
            assert al.positions.data.numel() == 0 and all(t.shape == (0,) and t.dtype == I64 for t in al[1:])


# ------------------------------------------------------------------ synchronisation
def test_read_backs(monkeypatch):
    hyps, refs = U.edge_case(63)
    built = {k: containers(hyps, refs, k + k) for k in KINDS}
    want = built['C'][0].edit_distance(built['C'][1])
    torch.cuda.synchronize()
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    for a in KINDS:
        for b in KINDS:
            z, rf = built[a][0], built[b][1]
            z.edit_distance(rf), z.edit_align(rf)
            assert calls == [], (a, b, calls)
    # device-only ref lengths: exactly ONE read-back of [B], attached to the container
    rf = ta.C(U.cat_of(refs).to(DEV), U.lens_of(refs).to(DEV))
    z = ta.C(U.cat_of(hyps).to(DEV), U.lens_of(hyps).to(DEV))    # (the hyp lengths are never needed on the host)
    dist = z.edit_distance(rf)
    assert calls == [(len(refs),)], calls
    z.edit_align(rf), z.edit_distance(rf), rf.left(0)
    assert calls == [(len(refs),)], calls
    assert torch.equal(dist, want)


# ------------------------------------------------------------------ end to end with the library's own collapse
def test_error_count_of_a_greedy_ctc_decode():
    V, blank = 6, 0
    gen = torch.Generator().manual_seed(21)
    lens = torch.tensor([30, 0, 75, 12, 64, 1])
    lp = torch.randn(int(lens.sum()), V, generator=gen)
    tlens = torch.tensor([9, 3, 20, 0, 31, 2])
    targets = torch.randint(1, V, (int(tlens.sum()),), generator=gen)
    # the greedy decode: the best class of every frame (torch's argmax over the V classes; the library's own `argmax` is
    # over time), then the library's collapse
    ids = ta.with_host_sizes(lp.to(DEV).argmax(-1), lens)
    runs = ids.unique_consecutive().values
    hyp = runs.compress(runs.data != blank)
    got = hyp.edit_distance(ta.with_host_sizes(targets.to(DEV), tlens))
    # the same pipeline with Python lists on the host
    want = []
    for frames, tgt in zip(torch.split(lp, lens.tolist()), torch.split(targets, tlens.tolist())):
        best = frames.argmax(1).tolist() if frames.size(0) else []
        collapsed = [c for k, c in enumerate(best) if k == 0 or c != best[k - 1]]
        want.append(U.edit_loop([c for c in collapsed if c != blank], tgt.tolist()).distance)
    assert got.tolist() == want
