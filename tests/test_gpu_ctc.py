"""Per-sequence CTC on the GPU: loss, gradient and alignment against the float64 DP of tests/ctc_util.py at the bound
derived there — the state buckets and both kernel forms, the 4 x 4 pairs of layouts bit for bit, degenerate sequences,
forbidden (-inf) and poisoned (NaN, out-of-range labels) inputs, batches larger than the launch, and the read-backs."""
import math

import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
from torchrua_amd import _meta
import ctc_util as U
from ctc_util import BF16, F16, F32, F64, I64
from gpu_util import DEV, dispatch_trace

pytestmark = pytest.mark.gpu

NAN, NINF, INF = float('nan'), -math.inf, math.inf
KINDS = ('C', 'L', 'P', 'R')


# ------------------------------------------------------------------ helpers
def build(kind, x, lens_host, host_sizes=True):
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        w = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(w), b.view(w))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def padding_mask(z):
    T = z.data.size(1)
    pos, n = torch.arange(T, device=DEV).unsqueeze(0), z.token_sizes.to(DEV).unsqueeze(1)
    return pos >= n if isinstance(z, ta.L) else pos < T - n


def weights(B):
    return torch.linspace(0.5, 2.0, B, dtype=F64) if B else torch.zeros(0, dtype=F64)


def run(lp, lens, y, ylens, blank=0, kinds='CC', zero_infinity=False, w=None, align=True):
    """(loss, gradient in cat form, labels / positions in cat form, score) from the GPU."""
    z = build(kinds[0], lp.to(DEV).requires_grad_(True), lens)
    leaf = z.data
    if kinds[0] != 'C':                                       # the leaf is the container's own storage
        z = type(z)(*((leaf.detach().requires_grad_(True),) + tuple(z[1:])))
        leaf = z.data
    tg = build(kinds[1], y.to(DEV), ylens)
    acc = F64 if lp.dtype == F64 else F32
    loss = z.ctc_loss(tg, blank, zero_infinity)
    assert loss.dtype == acc and loss.shape == (len(lens),)
    w = weights(len(lens)) if w is None else w
    (loss * w.to(DEV, acc)).sum().backward()
    grad = type(z)(*((leaf.grad,) + tuple(z[1:])))
    assert leaf.grad.dtype == lp.dtype and leaf.grad.shape == leaf.shape
    if kinds[0] in 'LR':
        assert bool((leaf.grad[padding_mask(z)] == 0).all()), 'padding rows of the gradient are zeros'
    out = [loss.detach(), grad.cat().data if kinds[0] != 'C' else leaf.grad]
    if align:
        al = z.ctc_align(tg, blank)
        assert isinstance(al, ta.SeqAlign) and type(al.labels) is type(z) and type(al.positions) is type(z)
        assert al.labels.data.dtype == I64 and al.labels.data.shape == z.data.shape[:-1] == al.positions.data.shape
        assert al.score.dtype == acc and not al.score.requires_grad
        if isinstance(z, ta.P):
            assert al.labels.batch_sizes is z.batch_sizes and al.positions.unsorted_indices is z.unsorted_indices
        else:
            assert al.labels.token_sizes is z.token_sizes and al.positions.token_sizes is z.token_sizes
        if kinds[0] in 'LR':
            pad = padding_mask(z)
            assert bool((al.labels.data[pad] == 0).all()) and bool((al.positions.data[pad] == 0).all())
        out += [al.labels.cat().data, al.positions.cat().data, al.score]
    return out


_want = {}


def want_of(lp, lens, y, ylens, blank, w=None):
    """(loss64, grad64) of the batch, computed once per (never modified) input."""
    key = (id(lp), id(y), blank, None if w is None else id(w))
    if key not in _want:
        _want[key] = U.grads64(lp, lens, y, ylens, blank, weights(len(lens)) if w is None else w) + ((lp, y, w),)
    return _want[key][:2]


def check_values(got, loss64, grad64, bd_z, bd_g, lens, w, dtype, what):
    """achieved / bound <= 1 for the loss, the gradient and the per-frame sums of the gradient."""
    r_loss = U.ratio(got[0], loss64, bd_z)
    scale = torch.repeat_interleave(w, lens).unsqueeze(1)
    gb = bd_g * scale + U.half_ulp(grad64, dtype)
    r_grad = U.ratio(got[1], grad64, gb)
    # sum_c grad[t, c] == -g[b] in every frame of a sequence that has an alignment
    live = torch.repeat_interleave(torch.isfinite(loss64), lens)
    gsum = torch.where(live, -scale.squeeze(1), torch.zeros(int(lens.sum()), dtype=F64))
    r_sum = U.ratio(got[1].double().sum(1), gsum, gb.sum(1) + 2.0 ** -40)
    U.note(f'{what} loss', r_loss)
    U.note(f'{what} grad', r_grad)
    U.note(f'{what} frame sum', r_sum)
    assert r_loss <= 1.0 and r_grad <= 1.0 and r_sum <= 1.0, (r_loss, r_grad, r_sum)


def check(lp, lens, y, ylens, blank, dtype, what, kinds='CC', zero_infinity=False):
    """Loss and gradient of the GPU against the float64 DP, achieved / bound <= 1; returns what run() returned."""
    got = run(lp, lens, y, ylens, blank, kinds, zero_infinity, align=False)
    loss64, grad64 = want_of(lp, lens, y, ylens, blank)
    if zero_infinity:
        loss64 = torch.where(loss64 == INF, torch.zeros_like(loss64), loss64)
    bd = U.bounds(lp, lens, y, ylens, blank, dtype)
    check_values(got, loss64, grad64, bd['z'], bd['g'], lens, weights(len(lens)), dtype, what)
    return got


def check_align(lp, lens, y, ylens, blank, kinds='CC'):
    """On integer-valued log-probabilities: labels, positions and score equal the float64 Viterbi exactly."""
    z = build(kinds[0], lp.to(DEV), lens)
    al = z.ctc_align(build(kinds[1], y.to(DEV), ylens), blank)
    labels, positions, score = al.labels.cat().data.cpu(), al.positions.cat().data.cpu(), al.score.cpu().double()
    want = [U.viterbi_seq(p, q, blank) for p, q in zip(U.pieces(lp, lens), U.pieces(y, ylens))]
    assert torch.equal(labels, torch.cat([v[0] for v in want]))
    assert torch.equal(positions, torch.cat([v[1] for v in want]))
    assert torch.equal(score, torch.stack([v[2] for v in want]))
    # score == the sum of lp along labels (exact on integers)
    picked = lp.double().gather(1, labels.unsqueeze(1)).squeeze(1)
    for b, (p, l) in enumerate(zip(U.pieces(picked, lens), lens.tolist())):
        if torch.isfinite(score[b]):
            assert float(p.sum()) == float(score[b]), b
    return al, z


# ------------------------------------------------------------------ the state buckets and both forms
EDGES = (0, 1, 31, 32, 63, 64, 127, 128, 255, 256, 1023)
EDGE_CASES = [(s, F32) for s in EDGES] + [(s, d) for s in (31, 64, 256) for d in (F64, BF16, F16)]


@pytest.mark.parametrize('s_max,dtype', EDGE_CASES, ids=[f'S{s}-{U.name(d)}' for s, d in EDGE_CASES])
def test_bucket_edges(s_max, dtype):
    lp, lens, y, ylens = U.edge_case(s_max, dtype)
    with dispatch_trace() as tr:
        check(lp, lens, y, ylens, 0, dtype, f'{U.bucket(s_max)} {U.name(dtype)}')
    form = 'form=workgroup' if U.bucket(s_max) == 'WG' else f'form=lanes R={U.bucket(s_max)[1:]}'
    assert tr.matching(f'seg_ctc_forward_kernel {form} S_max={s_max} semiring=log'), tr.records
    assert tr.matching(f'seg_ctc_backward_kernel {form} S_max={s_max}'), tr.records
    lpi = U.draw_lp(int(lens.sum()), lp.size(1), dtype, 77, integers=True)
    with dispatch_trace() as tr:
        check_align(lpi, lens, y, ylens, 0)
    assert tr.matching(f'seg_ctc_forward_kernel {form} semiring=max') and 'seg_ctc_backtrace_kernel' in tr.kernels


def test_target_of_1024_labels_is_refused():
    y = torch.ones(1024, dtype=I64, device=DEV)
    z = ta.with_host_sizes(torch.zeros(4, 3, device=DEV), torch.tensor([4]))
    for tg in (ta.with_host_sizes(y, torch.tensor([1024])), ta.C(y, torch.tensor([1024], device=DEV))):
        with pytest.raises(ta.RuaError, match='`targets` has 1024 labels'):
            z.ctc_loss(tg)
        with pytest.raises(ta.RuaError, match='`targets` has 1024 labels'):
            z.ctc_align(tg)


def test_same_bits_in_every_bucket_and_form():
    """One short sequence next to a filler whose target decides the bucket: the same loss, gradient and alignment bits."""
    V, blank = 6, 2
    y0 = torch.tensor([1, 1, 3, 0, 5], dtype=I64)
    lp0 = U.draw_lp(11, V, F32, 3)
    ref = None
    for filler in (5, 40, 100, 200, 300):
        yf = U.draw_target(filler, V, blank, 9)
        lens, ylens = torch.tensor([11, filler + 2]), torch.tensor([5, filler])
        lp = torch.cat([lp0, U.draw_lp(filler + 2, V, F32, 4)])
        loss, grad, labels, positions, score = run(lp, lens, torch.cat([y0, yf]), ylens, blank)
        got = (loss[:1], grad[:11], labels[:11], positions[:11], score[:1])
        if ref is None:
            ref = got
        for g, r, what in zip(got, ref, ('loss', 'grad', 'labels', 'positions', 'score')):
            assert same_bits(g, r), (filler, what)


# ------------------------------------------------------------------ degenerate sequences
def _one(lp, y, blank=0, **kw):
    return run(lp, torch.tensor([lp.size(0)]), torch.tensor(y, dtype=I64), torch.tensor([len(y)]), blank, **kw)


@pytest.mark.parametrize('dtype', [F32, F64, BF16, F16], ids=U.name)
def test_degenerate_sequences(dtype):
    lp = U.draw_lp(9, 3, dtype, 1, integers=True) - 1
    acc = F64 if dtype == F64 else F32
    loss, grad, labels, positions, score = _one(lp[:0], [])
    assert loss.tolist() == [0.0] and score.tolist() == [0.0] and labels.numel() == 0
    loss, grad, labels, positions, score = _one(lp[:0], [1, 2])
    assert loss.tolist() == [INF] and score.tolist() == [NINF]
    assert _one(lp[:0], [1, 2], zero_infinity=True)[0].tolist() == [0.0]
    loss, grad, labels, positions, score = _one(lp[:1], [2])
    assert loss.item() == -lp[0, 2].item() and labels.tolist() == [2] and positions.tolist() == [0]
    assert grad.cpu().tolist() == [[0.0, 0.0, -0.5]]            # the cotangent of a single sequence is weights(1) = 0.5
    # "aa" needs a blank between: no alignment at T = 2, one path at T = 3
    loss, grad, labels, positions, score = _one(lp[:2], [1, 1])
    assert loss.tolist() == [INF] and score.tolist() == [NINF] and not grad.any()
    assert labels.tolist() == [0, 0] and positions.tolist() == [-1, -1]
    loss, grad, labels, positions, score = _one(lp[:3], [1, 1])
    one_path = -(lp[0, 1] + lp[1, 0] + lp[2, 1]).item()
    assert loss.item() == one_path and score.item() == -one_path
    assert labels.tolist() == [1, 0, 1] and positions.tolist() == [0, -1, 1]
    # five equal labels at exactly T = 9: one path, the loss is minus the sum of nine known entries
    loss, grad, labels, positions, score = _one(lp, [2] * 5)
    want = -sum(lp[t, 2 if t % 2 == 0 else 0].item() for t in range(9))
    assert loss.item() == want and loss.dtype == acc
    assert labels.tolist() == [2, 0] * 4 + [2] and positions.tolist() == [0, -1, 1, -1, 2, -1, 3, -1, 4]
    # S = 0: minus the sum of the blank column
    loss = _one(lp, [], blank=1)[0]
    assert loss.item() == -lp[:, 1].double().sum().item()


def test_zero_infinity_and_zero_gradients_next_to_nan():
    V = 4
    lens, ylens = torch.tensor([2, 5, 3]), torch.tensor([2, 2, 1])
    y = torch.tensor([1, 1, 2, 3, 1], dtype=I64)                # "aa" at T = 2: no alignment
    lp = U.draw_lp(10, V, F32, 5).clone()
    lp[8] = NAN                                                 # poisons the third sequence alone
    for zi in (False, True):
        loss, grad = run(lp, lens, y, ylens, 0, zero_infinity=zi, align=False)
        assert loss[0].item() == (0.0 if zi else INF)
        assert not grad[:2].any(), 'the gradient of a sequence without alignment is exact zeros'
        assert math.isnan(loss[2].item()) and torch.isfinite(loss[1]) and bool(torch.isfinite(grad[2:7]).all())
    clean = run(lp[:7], lens[:2], y[:4], ylens[:2], 0, align=False, w=weights(3)[:2])
    assert same_bits(clean[0][1:2], loss[1:2]) and same_bits(clean[1][2:7], grad[2:7])


# ------------------------------------------------------------------ classes
@pytest.mark.parametrize('V,blank,dtype', [(1, 0, F32), (2, 0, F32), (2, 1, BF16), (37, 0, F32), (37, 36, F16), (37, 17, F64),
                                           (5003, 2501, BF16), (5003, 0, F32)])
def test_classes_and_blank(V, blank, dtype):
    seed = V + blank
    if V == 1:
        ys = [U.draw_target(0, V, blank, seed)] * 3
    else:
        ys = [U.draw_target(4, V, blank, seed, repeats=1), U.draw_target(0, V, blank, seed),
              U.draw_target(6, V, blank, seed + 1, with_blank=True), torch.tensor([blank, blank, (blank + 1) % V], dtype=I64)]
    ts = [int(q.numel()) + U.n_repeats(q) + 2 for q in ys]
    lens, ylens = torch.tensor(ts), torch.tensor([int(q.numel()) for q in ys])
    lp, y = U.draw_lp(sum(ts), V, dtype, seed), torch.cat(ys)
    check(lp, lens, y, ylens, blank, dtype, f'V={V} {U.name(dtype)}', kinds='CP' if V > 1 else 'CC')
    check_align(U.draw_lp(sum(ts), V, dtype, seed + 1, integers=True), lens, y, ylens, blank)


# ------------------------------------------------------------------ forbidden and poisoned inputs
def test_forbidden_classes_nan_frames_and_labels_out_of_range():
    V = 6
    ys = [torch.tensor([1, 2, 3], dtype=I64), torch.tensor([4, 4], dtype=I64), torch.tensor([2, 5, 1], dtype=I64),
          torch.tensor([3], dtype=I64)]
    ts = [6, 5, 7, 3]
    lens, ylens, y = torch.tensor(ts), torch.tensor([3, 2, 3, 1]), torch.cat(ys)
    base = U.draw_lp(sum(ts), V, F32, 21)
    # -inf columns: class 5 is forbidden everywhere (sequence 2 loses every path), class 0 (blank) in sequence 0
    lp = base.clone()
    lp[:, 5] = NINF
    lp[:6, 0] = NINF
    got = check(lp, lens, y, ylens, 0, F32, 'forbidden classes')
    assert got[0][2].item() == INF and not got[1][11:18].any() and bool(torch.isfinite(got[0][[0, 1, 3]]).all())
    assert not torch.isnan(got[1]).any()
    # a NaN frame poisons its own sequence alone; labels -1 and V in one sequence: NaN, zero gradient, no fault
    lp = base.clone()
    lp[7] = NAN
    bad = y.clone()
    bad[5], bad[7] = -1, V
    loss, grad, labels, positions, score = run(lp, lens, bad, ylens, 0)
    clean = run(base, lens, y, ylens, 0)
    assert math.isnan(loss[1].item()) and math.isnan(loss[2].item()) and math.isnan(score[2].item())
    assert not grad[11:18].any() and bool((labels[11:18] == 0).all()) and bool((positions[11:18] == -1).all())
    for b, rows in ((0, slice(0, 6)), (3, slice(18, 21))):
        assert same_bits(loss[b:b + 1], clean[0][b:b + 1]) and same_bits(grad[rows], clean[1][rows])
        assert same_bits(labels[rows], clean[2][rows]) and same_bits(score[b:b + 1], clean[4][b:b + 1])


# ------------------------------------------------------------------ more sequences than the launch has teams
_big = {}
POOL, TILES = 100, 41                                           # 4 100 sequences: a pool of 100, 41 times over


def big_batch():
    """4 100 sequences of T = U(0, 6), V = 4 with their yardsticks — computed on the 100 distinct sequences and tiled (the
    DP of a sequence does not depend on its neighbours; the gradient is linear in the cotangent)."""
    if not _big:
        gen = torch.Generator().manual_seed(8)
        V = 4
        lens = torch.randint(0, 7, (POOL,), generator=gen)
        ylens = torch.minimum(torch.randint(0, 4, (POOL,), generator=gen), lens)
        y = torch.randint(1, V, (int(ylens.sum()),), generator=gen)
        lp = U.draw_lp(int(lens.sum()), V, F32, 9)
        loss64, grad64 = U.grads64(lp, lens, y, ylens, 0, torch.ones(POOL, dtype=F64))
        bd = U.bounds(lp, lens, y, ylens, 0, F32)
        w = weights(POOL * TILES)
        scale = torch.repeat_interleave(w, lens.repeat(TILES)).unsqueeze(1)
        _big.update(case=(lp.repeat(TILES, 1), lens.repeat(TILES), y.repeat(TILES), ylens.repeat(TILES)),
                    want=(loss64.repeat(TILES), grad64.repeat(TILES, 1) * scale, bd['z'].repeat(TILES),
                          bd['g'].repeat(TILES, 1), w))
    return _big['case'], _big['want']


@pytest.mark.parametrize('form', ['lanes', 'workgroup'])
def test_more_sequences_than_the_launch_has_teams(form):
    (lp, lens, y, ylens), (loss64, grad64, bz, bg, w) = big_batch()
    b = 2050
    rows = slice(int(lens[:b].sum()), int(lens[:b + 1].sum()))
    if form == 'workgroup':                                     # one target of 256 labels (no alignment at T <= 6)
        before = int(ylens[:b].sum())
        y = torch.cat([y[:before], torch.ones(256, dtype=I64), y[before + int(ylens[b]):]])
        ylens, loss64, grad64, bg = ylens.clone(), loss64.clone(), grad64.clone(), bg.clone()
        ylens[b], loss64[b], grad64[rows], bg[rows] = 256, INF, 0.0, 0.0
    with dispatch_trace() as tr:
        got = run(lp, lens, y, ylens, 0, align=False)
    check_values(got, loss64, grad64, bz, bg, lens, w, F32, f'4100 sequences {form}')
    assert tr.matching(f'seg_ctc_forward_kernel form={form} grid=1024'), tr.records
    assert tr.matching(f'seg_ctc_backward_kernel form={form} grid=1024'), tr.records
    if form == 'workgroup':                                     # ... and the same bits as the lanes form everywhere else
        lanes = run(*big_batch()[0], 0, align=False)
        keep = torch.arange(POOL * TILES) != b
        assert same_bits(got[0][keep.to(DEV)], lanes[0][keep.to(DEV)])
        keep_rows = torch.repeat_interleave(keep, lens).to(DEV)
        assert same_bits(got[1][keep_rows], lanes[1][keep_rows]) and got[0][b].item() == INF


# ------------------------------------------------------------------ the 4 x 4 pairs of layouts
@pytest.mark.parametrize('dtype', [F32, BF16], ids=U.name)
def test_all_sixteen_pairs_of_layouts_give_the_same_bits(dtype):
    V, blank = 7, 3
    ys = [U.draw_target(5, V, blank, 1, repeats=1), U.draw_target(0, V, blank, 1), U.draw_target(9, V, blank, 2),
          U.draw_target(2, V, blank, 3), U.draw_target(4, V, blank, 4)]
    ts = [9, 3, 12, 0, 3]                                       # (the last one has no alignment: T < S)
    lens, ylens, y = torch.tensor(ts), torch.tensor([int(q.numel()) for q in ys]), torch.cat(ys)
    lp = U.draw_lp(sum(ts), V, dtype, 31, integers=True)
    want = run(lp, lens, y, ylens, blank, 'CC')
    seg = ta.segment_ctc_loss(lp.to(DEV), lens.to(DEV), y.to(DEV), ylens.to(DEV), blank)
    assert same_bits(seg, want[0])
    for a in KINDS:
        for b in KINDS:
            got = run(lp, lens, y, ylens, blank, a + b)
            for g, w, what in zip(got, want, ('loss', 'grad', 'labels', 'positions', 'score')):
                assert same_bits(g, w), (a, b, what)
    check_align(lp, lens, y, ylens, blank, 'PR')
    # device-only lengths on both sides give the same bits as well
    z, tg = build('L', lp.to(DEV), lens, False), build('C', y.to(DEV), ylens, False)
    assert same_bits(z.ctc_loss(tg, blank), want[0]) and same_bits(ta.ctc_align(z, tg, blank).labels.cat().data, want[2])


# ------------------------------------------------------------------ gradients
def test_gradient_behind_a_class_log_softmax_equals_torchs():
    """x.log_softmax(-1) -> container -> pack() -> ctc_loss -> backward: x.grad equals the gradient torch's CPU float64
    F.ctc_loss gives with respect to the logits (there, and only there, torch's `grad` is right)."""
    V, blank = 9, 0
    ys = [U.draw_target(4, V, blank, 5, repeats=1), U.draw_target(2, V, blank, 6), U.draw_target(0, V, blank, 7)]
    ts = [8, 5, 3]
    lens, ylens, y = torch.tensor(ts), torch.tensor([4, 2, 0]), torch.cat(ys)
    x = torch.randn(sum(ts), V, dtype=F64, generator=torch.Generator().manual_seed(2))
    w = weights(3)
    # torch, CPU, float64, padded
    xc = x.clone().requires_grad_(True)
    pad = torch.zeros(max(ts), 3, V, dtype=F64)
    rows = torch.cat([torch.arange(t) for t in ts]), torch.repeat_interleave(torch.arange(3), lens)
    pad = pad.index_put(rows, xc).log_softmax(-1)
    ypad = torch.zeros(3, 4, dtype=I64)
    for b, q in enumerate(ys):
        ypad[b, :q.numel()] = q
    want_loss = F.ctc_loss(pad, ypad, lens, ylens, blank=blank, reduction='none')
    (want_loss * w).sum().backward()
    # the library
    xg = x.to(DEV).requires_grad_(True)
    z = ta.with_host_sizes(xg.log_softmax(-1), lens).pack()
    loss = z.ctc_loss(ta.with_host_sizes(y.to(DEV), ylens), blank)
    (loss * w.to(DEV)).sum().backward()
    lp = x.log_softmax(-1)
    bd = U.bounds(lp, lens, y, ylens, blank, F64)
    gb = U.grad_bound(torch.zeros_like(lp), bd, F64, lens, w)
    # d/dx = grad_lp - softmax * sum_c grad_lp: both terms carry the bound; torch's own log_softmax on the two devices
    # differs by a few ulps of float64 and its backward adds V terms: 64 V u (1 + |g|) on top
    slack = 64 * V * 2.0 ** -53 * (1 + float(w.max()))
    r = U.ratio(xg.grad, xc.grad, gb + gb.sum(1, keepdim=True) + slack)
    r_loss = U.ratio(loss.detach(), want_loss.detach(), bd['z'] + slack)
    U.note('composed with log_softmax f64 grad', r)
    assert r <= 1.0 and r_loss <= 1.0


def test_gradient_is_reproducible_and_second_order_raises():
    lp, lens, y, ylens = U.edge_case(64, F32)
    a, b = run(lp, lens, y, ylens, 0, 'PL', align=False), run(lp, lens, y, ylens, 0, 'PL', align=False)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    z = build('C', lp.to(DEV).requires_grad_(True), lens)
    loss = z.ctc_loss(build('C', y.to(DEV), ylens)).sum()
    with pytest.raises(ta.RuaError, match='second derivatives'):
        torch.autograd.grad(loss, z.data, create_graph=True)
    # without a graph there is no Function at all
    assert not build('C', lp.to(DEV), lens).ctc_loss(build('C', y.to(DEV), ylens)).requires_grad


# ------------------------------------------------------------------ alignment
def test_alignment_on_real_ties_and_by_the_librarys_own_collapse():
    V, blank = 5, 0
    gen = torch.Generator().manual_seed(13)
    ys, ts = [], []
    for b in range(12):
        S = int(torch.randint(0, 7, (1,), generator=gen))
        q = U.draw_target(S, V, blank, 100 + b, repeats=min(b % 3, max(S - 1, 0)))
        ys.append(q)
        ts.append(S + U.n_repeats(q) + int(torch.randint(0, 5, (1,), generator=gen)))
    lens, ylens, y = torch.tensor(ts), torch.tensor([int(q.numel()) for q in ys]), torch.cat(ys)
    gen = torch.Generator().manual_seed(14)
    lp = torch.randint(-1, 1, (sum(ts), V), generator=gen).float()     # {-1, 0}: ties everywhere
    for kinds in ('CC', 'LP', 'RC', 'PL'):
        al, z = check_align(lp, lens, y, ylens, blank, kinds)
    # labels.unique_consecutive().values.compress(values != blank) is the target of every sequence
    al, z = check_align(lp, lens, y, ylens, blank, 'CC')
    runs = al.labels.unique_consecutive().values
    back = runs.compress(runs.data != blank).cat()
    assert torch.equal(back.data.cpu(), y) and torch.equal(back.token_sizes.cpu(), ylens)


# ------------------------------------------------------------------ synchronisation
def test_read_backs(monkeypatch):
    lp, lens, y, ylens = U.edge_case(31, F32)
    built = {k: (build(k, lp.to(DEV), lens), build(k, y.to(DEV), ylens)) for k in KINDS}
    want = built['C'][0].ctc_loss(built['C'][1])
    torch.cuda.synchronize()
    calls = []
    real = _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    for a in KINDS:
        for b in KINDS:
            z, tg = built[a][0], built[b][1]
            z.ctc_loss(tg), z.ctc_align(tg)
            assert calls == [], (a, b, calls)
    # device-only target lengths: exactly ONE read-back of [B], attached to the container
    tg = ta.C(y.to(DEV), ylens.to(DEV))
    z = ta.C(lp.to(DEV), lens.to(DEV))                          # (the frame lengths are never needed on the host)
    loss = z.ctc_loss(tg)
    assert calls == [(len(ylens),)], calls
    z.ctc_align(tg), z.ctc_loss(tg), tg.left(0)
    assert calls == [(len(ylens),)], calls
    assert same_bits(loss, want)
