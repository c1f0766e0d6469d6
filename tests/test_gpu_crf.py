"""The per-sequence linear-chain CRF on the GPU: the four layouts bit for bit, logZ / marginals / Viterbi / gradients
against the float64 yardsticks of tests/crf_util.py at the bound derived there, forbidden moves (-inf), NaN, ties, empty
sequences and the grid shapes (more sequences than waves, one long sequence, B = 1, B = 0)."""
import math

import pytest
import torch

import torchrua_amd as ta
import crf_util as U
from crf_util import BF16, F16, F32, F64, I64, BASE_LENS, TAGS
from gpu_util import DEV

pytestmark = pytest.mark.gpu

NAN, NINF = float('nan'), -math.inf
KINDS = ('C', 'L', 'P', 'R')


# ------------------------------------------------------------------ helpers
def build(kind, x, lens_host, host_sizes=True):
    c = ta.with_host_sizes(x, lens_host) if host_sizes else ta.C(x, lens_host.to(DEV))
    return {'C': lambda: c, 'L': lambda: c.left(0), 'R': lambda: c.right(0), 'P': c.pack}[kind]()


def rewrap(z, data):
    if isinstance(z, ta.P):
        return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
    return z._replace(data=data)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.is_floating_point():
        w = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(w), b.view(w))
    return a.shape == b.shape and torch.equal(a, b)


def gpu(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def padding_mask(z):
    """True at the padding positions [B, T_phys] of an L / R."""
    T = z.data.size(1)
    pos, n = torch.arange(T, device=DEV).unsqueeze(0), z.token_sizes.to(DEV).unsqueeze(1)
    return pos >= n if isinstance(z, ta.L) else pos < T - n


def run_all(z, tr, st, en):
    """(logZ, marginals in cat form, tags in cat form, score) of the container z, with the surface checks."""
    acc = F64 if z.data.dtype == F64 else F32
    logz = z.crf_partition(tr, st, en)
    marg = z.crf_marginals(tr, st, en)
    path = z.crf_decode(tr, st, en)
    assert isinstance(path, ta.SeqPath) and type(marg) is type(z) and type(path.tags) is type(z)
    assert marg.data.shape == z.data.shape and marg.data.dtype == z.data.dtype
    assert path.tags.data.shape == z.data.shape[:-1] and path.tags.data.dtype == I64
    assert logz.dtype == acc and path.score.dtype == acc and logz.dim() == 1 and logz.shape == path.score.shape
    assert not logz.requires_grad and not path.score.requires_grad and not marg.data.requires_grad
    if not isinstance(z, ta.P):
        assert marg.token_sizes is z.token_sizes and path.tags.token_sizes is z.token_sizes
    else:
        assert path.tags.batch_sizes is z.batch_sizes and path.tags.unsorted_indices is z.unsorted_indices
    if isinstance(z, (ta.L, ta.R)):
        pad = padding_mask(z)
        assert bool((marg.data[pad] == 0).all()) and bool((path.tags.data[pad] == 0).all()), 'padding rows are zeros'
    return logz, marg.cat().data, path.tags.cat().data, path.score


def case_gpu(K, dtype, **kw):
    x, tr, st, en, lens = U.case(K, dtype, **kw)
    return (x, tr, st, en, lens), gpu(x, tr, st, en)


# ------------------------------------------------------------------ layouts
@pytest.mark.parametrize('K,dtype', [(K, F32) for K in TAGS] + [(9, BF16), (5, F64), (33, F16)])
def test_layouts_give_the_same_bits(K, dtype):
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(K, dtype)
    want = run_all(build('C', xg, lens), trg, stg, eng)
    seg = ta.segment_crf_partition(xg, trg, lens.to(DEV), stg, eng)
    assert same_bits(seg, want[0])
    for kind in KINDS:
        for host_sizes in (True, False):
            z = build(kind, xg, lens, host_sizes)
            if kind in 'LR':                                    # padding rows are never read
                z = z._replace(data=z.data.masked_fill(padding_mask(z).unsqueeze(-1), NAN))
            got = run_all(z, trg, stg, eng)
            for g, w, what in zip(got, want, ('logZ', 'marginals', 'tags', 'score')):
                assert same_bits(g, w), f'{kind} host_sizes={host_sizes}: {what} differs from the CattedSequence'
    # a P of a batch in another order answers in ITS batch order
    perm = torch.tensor([7, 0, 3, 9, 1, 5, 8, 2, 6, 4])
    xs = torch.cat([U.pieces(x, lens)[i] for i in perm.tolist()]).to(DEV)
    got = run_all(build('P', xs, lens[perm]), trg, stg, eng)
    assert same_bits(got[0], want[0][perm.to(DEV)]) and same_bits(got[3], want[3][perm.to(DEV)])


# ------------------------------------------------------------------ values
@pytest.mark.parametrize('dtype', (F32, F64, BF16, F16), ids=U.name)
@pytest.mark.parametrize('K', TAGS)
def test_values_against_the_float64_yardstick(K, dtype):
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(K, dtype)
    logz, marg, _, _ = run_all(build('C', xg, lens), trg, stg, eng)
    bd = U.bounds(x, tr, st, en, lens, dtype)
    want = U.logz64(x, tr, st, en, lens)
    r = U.ratio(logz, want, bd['z'])
    U.note(f'logZ {U.name(dtype)} bucket={U.bucket(K)}', r)
    assert r <= 1.0, f'logZ: {r:.3f} x the derived bound'
    assert logz[0].item() == 0 and logz[8].item() == 0, 'an empty sequence has logZ = 0'
    p = U.marginals64(x, tr, st, en, lens)
    mb = U.marginal_bound(p, bd, dtype, lens)
    r = U.ratio(marg, p, mb)
    U.note(f'marginals {U.name(dtype)} bucket={U.bucket(K)}', r)
    assert r <= 1.0, f'marginals: {r:.3f} x the derived bound'
    # every token's marginals sum to 1 (K terms, each inside its bound, and the sum of K roundings)
    err = (marg.double().cpu().sum(1) - 1).abs()
    assert bool((err <= mb.sum(1) + K * 2.0 ** -24).all())
    if K == 1:
        plain = torch.stack([q.double().sum() + (st.double() + en.double()).sum() * (len(q) > 0)
                             + tr.double().sum() * max(len(q) - 1, 0) for q in U.pieces(x, lens)])
        assert U.ratio(logz, plain, bd['z']) <= 1.0


def test_none_equals_a_zeros_tensor_bit_for_bit():
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(5, F32)
    xg = xg.clone()
    xg[::7] = -0.0                                             # (0 + -0.0 is +0.0: a skipped addition would show)
    zero = torch.zeros(5, device=DEV)
    for kind in ('C', 'R'):
        z = build(kind, xg, lens)
        for a, b in (((None, None), (zero, zero)), ((stg, None), (stg, zero)), ((None, eng), (zero, eng))):
            for g, w in zip(run_all(z, trg, *a), run_all(z, trg, *b)):
                assert same_bits(g, w)


# ------------------------------------------------------------------ -inf: forbidden moves
def test_bio_constraints():
    B_, I_, O_ = 0, 1, 2
    (x, tr, st, en, lens), _ = case_gpu(3, F32)
    tr, st = tr.clone(), st.clone()
    tr[O_, I_] = NINF
    st[I_] = NINF
    xg, trg, stg, eng = gpu(x, tr, st, en)
    for kind in ('C', 'P'):
        logz, marg, tags, score = run_all(build(kind, xg, lens), trg, stg, eng)
        bd = U.bounds(x, tr, st, en, lens, F32)
        want = U.logz64(x, tr, st, en, lens)
        assert bool(torch.isfinite(logz).all())
        r = U.ratio(logz, want, bd['z'])
        U.note('logZ float32 BIO', r)
        assert r <= 1.0
        r = U.ratio(marg, U.marginals64(x, tr, st, en, lens), U.marginal_bound(U.marginals64(x, tr, st, en, lens), bd, F32, lens))
        assert r <= 1.0
        off = 0
        for n in lens.tolist():
            seq = tags[off:off + n].tolist()
            if n:
                assert seq[0] != I_ and marg[off, I_].item() == 0, 'a forbidden state has marginal exactly 0'
            assert all(not (a == O_ and b == I_) for a, b in zip(seq, seq[1:])), 'a decoded path takes a forbidden move'
            off += n
        assert bool(torch.isfinite(score).all())


def test_a_sequence_with_every_path_forbidden():
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(5, F32)
    dead, start_row = 3, sum(BASE_LENS[:3])                     # the sequence of 5 tokens
    xd = x.clone()
    xd[start_row + 2] = NINF
    w = U.draw((len(lens),), F32, 77)
    outs = []
    for data in (x, xd):
        leaves = [t.to(DEV).requires_grad_(True) for t in (data, tr, st, en)]
        z = build('C', leaves[0], lens)
        logz = z.crf_partition(*leaves[1:])
        logz.backward(w.to(DEV))                               # (a cotangent that is NOT zero at the dead sequence)
        with torch.no_grad():
            marg = z.crf_marginals(*leaves[1:]).data
        outs.append((logz.detach(), marg, [l.grad for l in leaves]))
    (lz, mg, gr), (lzd, mgd, grd) = outs
    rows = slice(start_row, start_row + 5)
    assert lzd[dead].item() == NINF
    assert bool((mgd[rows] == 0).all()) and bool((grd[0][rows] == 0).all()), 'its marginals and gradients are exact zeros'
    keep = torch.ones(len(lens), dtype=torch.bool)
    keep[dead] = False
    keep_rows = torch.ones(x.size(0), dtype=torch.bool)
    keep_rows[rows] = False
    assert same_bits(lzd[keep], lz[keep]) and same_bits(mgd[keep_rows], mg[keep_rows])
    assert same_bits(grd[0][keep_rows], gr[0][keep_rows])
    want = U.grads64(xd, tr, st, en, lens, w)
    bd = U.bounds(x, tr, st, en, lens, F32)                      # (of the live batch: the dead sequence adds nothing)
    want_abs = U.grads64(xd, tr, st, en, lens, w.abs())
    for i, what in ((2, 'transitions'), (3, 'start'), (4, 'end')):
        assert bool(torch.isfinite(grd[i - 1]).all())
        assert U.ratio(grd[i - 1], want[i], U.param_bound(want[i], want_abs[i], bd, F32, x.size(0))) <= 1.0, what


# ------------------------------------------------------------------ NaN
def test_a_nan_poisons_only_its_own_sequence():
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(9, F32)
    sick, start_row = 4, sum(BASE_LENS[:4])                      # the sequence of 63 tokens
    xn = xg.clone()
    xn[start_row + 30, 2] = NAN
    rows = torch.zeros(x.size(0), dtype=torch.bool)
    rows[start_row:start_row + 63] = True
    seqs = torch.zeros(len(lens), dtype=torch.bool)
    seqs[sick] = True
    for kind in ('C', 'L'):
        clean = run_all(build(kind, xg, lens), trg, stg, eng)
        got = run_all(build(kind, xn, lens), trg, stg, eng)
        assert math.isnan(got[0][sick].item()) and math.isnan(got[3][sick].item())
        assert bool(torch.isnan(got[1][rows]).all())
        assert same_bits(got[0][~seqs], clean[0][~seqs]) and same_bits(got[3][~seqs], clean[3][~seqs])
        assert same_bits(got[1][~rows], clean[1][~rows]) and torch.equal(got[2][~rows], clean[2][~rows])
    leaf = xn.clone().requires_grad_(True)
    build('C', leaf, lens).crf_partition(trg, stg, eng).sum().backward()
    assert bool(torch.isnan(leaf.grad[rows]).all()) and bool(torch.isfinite(leaf.grad[~rows]).all())


# ------------------------------------------------------------------ Viterbi
@pytest.mark.parametrize('dtype', (F32, BF16, F16, F64), ids=U.name)
@pytest.mark.parametrize('K', TAGS)
def test_viterbi_on_integer_scores_is_exact(K, dtype):
    """Integer scores of [-3, 3]: every sum is exact in fp32 (and the inputs in bf16), so the ties are real."""
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(K, dtype, integers=True, seed=9)
    want_tags, want_score = U.viterbi64(x, tr, st, en, lens)
    for kind in ('C', 'R'):
        path = build(kind, xg, lens).crf_decode(trg, stg, eng)
        assert torch.equal(path.tags.cat().data.cpu(), want_tags), f'{kind}: tags'
        assert torch.equal(path.score.double().cpu(), want_score), f'{kind}: score'
    none = build('C', xg, lens).crf_decode(trg)
    w_tags, w_score = U.viterbi64(x, tr, None, None, lens)
    assert torch.equal(none.tags.data.cpu(), w_tags) and torch.equal(none.score.double().cpu(), w_score)


@pytest.mark.parametrize('K,dtype', [(K, F32) for K in TAGS] + [(9, BF16), (33, F64)])
def test_viterbi_on_random_scores(K, dtype):
    """With d the bound of one path's score in the recursion's arithmetic (the LOG bound d_Z covers it: a max rounds
    nothing and |max| <= |logsumexp| + log K): the kernel's score is the fp32 score of ITS path and at least the fp32
    score of the optimum, so |score - opt| <= d and the true score of its path is >= opt - 2 d."""
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(K, dtype)
    path = build('P', xg, lens).crf_decode(trg, stg, eng)
    tags = path.tags.cat().data.cpu()
    assert bool(((tags >= 0) & (tags < K)).all())
    _, opt = U.viterbi64(x, tr, st, en, lens)
    d = U.bounds(x, tr, st, en, lens, dtype)['z']
    mine = U.path_score64(x, tags, tr, st, en, lens)
    r = U.ratio(path.score, opt, d)
    U.note(f'viterbi score {U.name(dtype)} bucket={U.bucket(K)}', r)
    assert r <= 1.0
    assert bool((opt - mine <= 2 * d).all()) and bool((mine <= opt + 1e-9).all())


# ------------------------------------------------------------------ autograd
def grads_gpu(kind, x, tr, st, en, lens, w, host_sizes=True):
    z = build(kind, x.to(DEV), lens, host_sizes)
    leaves = [z.data.detach().clone().requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (tr, st, en)]
    logz = rewrap(z, leaves[0]).crf_partition(*leaves[1:])
    assert logz.requires_grad
    (logz * w.to(DEV).to(logz.dtype)).sum().backward()
    return [rewrap(z, leaves[0].grad).cat().data] + [l.grad for l in leaves[1:]], rewrap(z, leaves[0].grad)


@pytest.mark.parametrize('kind,K,dtype', [('C', 5, F32), ('C', 9, F32), ('C', 33, F32), ('C', 64, F32), ('C', 8, F64),
                                          ('C', 9, BF16), ('C', 5, F16), ('L', 9, F32), ('P', 33, BF16), ('R', 5, F64)])
def test_gradients_of_the_partition(kind, K, dtype):
    x, tr, st, en, lens = U.case(K, dtype)
    w = U.draw((len(lens),), F64 if dtype == F64 else F32, 31)
    got, gz = grads_gpu(kind, x, tr, st, en, lens, w)
    again, _ = grads_gpu(kind, x, tr, st, en, lens, w)
    for a, b in zip(got, again):
        assert same_bits(a, b), 'two runs on the same container give the same bits'
    if kind in 'LR':
        assert bool((gz.data[padding_mask(gz)] == 0).all()), 'padding rows of grad_emissions are zeros'
    for g, like in zip(got, (x, tr, st, en)):
        assert g.dtype == dtype and g.shape == like.shape
    bd = U.bounds(x, tr, st, en, lens, dtype)
    want = U.grads64(x, tr, st, en, lens, w)
    want_abs = U.grads64(x, tr, st, en, lens, w.abs())
    p = U.marginals64(x, tr, st, en, lens)
    r = U.ratio(got[0], want[1], U.marginal_bound(p, bd, dtype, lens, g=w))
    U.note(f'grad emissions {U.name(dtype)} bucket={U.bucket(K)}', r)
    assert r <= 1.0
    for i, what in ((1, 'transitions'), (2, 'start'), (3, 'end')):
        r = U.ratio(got[i], want[i + 1], U.param_bound(want[i + 1], want_abs[i + 1], bd, dtype, x.size(0)))
        U.note(f'grad {what} {U.name(dtype)} bucket={U.bucket(K)}', r)
        assert r <= 1.0, what


def test_create_graph_raises_and_partial_gradients():
    (x, tr, st, en, lens), (xg, trg, stg, eng) = case_gpu(5, F32)
    leaf = xg.clone().requires_grad_(True)
    logz = build('C', leaf, lens).crf_partition(trg, stg, eng)
    with pytest.raises(ta.RuaError, match='second derivatives'):
        torch.autograd.grad(logz.sum(), leaf, create_graph=True)
    # only a parameter wants a gradient; start / end None
    t_leaf = trg.clone().requires_grad_(True)
    build('P', xg, lens).crf_partition(t_leaf).sum().backward()
    want = U.grads64(x, tr, None, None, lens, torch.ones(len(lens)))
    bd = U.bounds(x, tr, None, None, lens, F32)
    assert U.ratio(t_leaf.grad, want[2], U.param_bound(want[2], want[2], bd, F32, x.size(0))) <= 1.0
    with torch.no_grad():
        assert not build('C', leaf, lens).crf_partition(trg).requires_grad


@pytest.mark.parametrize('kind,K,dtype', [('C', 9, F32), ('L', 5, BF16), ('P', 33, F32)])
def test_non_contiguous_parameters_give_the_bits_of_contiguous_ones(kind, K, dtype):
    """transitions = W.t(), start / end = columns of a matrix, and the stride-0 cotangent of .sum(): the launchers make
    contiguous copies, and every copy has to live until its launch is queued."""
    x, tr, st, en, lens = U.case(K, dtype)
    wt = tr.t().contiguous().to(DEV)                             # wt.t() is `tr`, non-contiguous
    cols = torch.stack([st, en, st], 1).contiguous().to(DEV)     # cols[:, 0] is `st`, cols[:, 1] is `en`
    z = build(kind, x.to(DEV), lens)

    def grads(tr_, st_, en_):
        leaves = [z.data.detach().clone().requires_grad_(True)] + [t.detach().requires_grad_(True) for t in (tr_, st_, en_)]
        logz = rewrap(z, leaves[0]).crf_partition(*leaves[1:])
        logz.sum().backward()
        return [logz.detach()] + [l.grad for l in leaves]

    want = grads(*gpu(tr, st, en))
    for _ in range(3):                                           # (the allocator's free list differs from call to call)
        got = grads(wt.t(), cols[:, 0], cols[:, 1])
        assert not wt.t().is_contiguous() and not cols[:, 1].is_contiguous()
        for g, w, what in zip(got, want, ('logZ', 'emissions', 'transitions', 'start', 'end')):
            assert same_bits(g.contiguous(), w), f'{what} differs with non-contiguous parameters'
    clean = run_all(z, *gpu(tr, st, en))
    for _ in range(3):
        for g, w in zip(run_all(z, wt.t(), cols[:, 0], cols[:, 1]), clean):
            assert same_bits(g, w)


@pytest.mark.parametrize('kind,K,dtype', [('C', 5, F32), ('L', 9, F32), ('P', 8, BF16), ('R', 33, F64)])
def test_score_and_the_nll(kind, K, dtype):
    x, tr, st, en, lens = U.case(K, dtype)
    acc = F64 if dtype == F64 else F32
    u = 2.0 ** -53 if dtype == F64 else 2.0 ** -24
    tags, _ = U.viterbi64(x, tr, st, en, lens)
    w = U.draw((len(lens),), acc, 41)
    z = build(kind, x.to(DEV), lens)
    zt = build(kind, tags.to(DEV), lens)
    leaves = [z.data.detach().clone().requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in (tr, st, en)]
    score = rewrap(z, leaves[0]).crf_score(zt, *leaves[1:])
    assert score.dtype == acc and score.shape == (len(lens),) and score.requires_grad
    want = U.path_score64(x, tags, tr, st, en, lens)
    # 2 n + 2 terms added in the accumulator type: (2 n + 2) u sum |terms| <= (2 n + 2) u (n + 1) * the largest term
    big = max(U._fmax(x.double()), U._fmax(tr.double()), U._fmax(st), U._fmax(en))
    sb = (2 * lens + 2).double() * u * (2 * lens + 2).double() * big
    assert U.ratio(score.detach(), want, sb) <= 1.0
    assert score[0].item() == 0 and score[8].item() == 0
    logz = z.crf_partition(*gpu(tr, st, en))
    bd = U.bounds(x, tr, st, en, lens, dtype)
    assert bool(((logz - score.detach()).double().cpu() >= -(bd['z'] + sb)).all()), 'logZ >= the score of any path'
    (score * w.to(DEV)).sum().backward()
    leaves64 = [t.double().clone().requires_grad_(True) for t in (x, tr, st, en)]
    (U.path_score64(leaves64[0], tags, *leaves64[1:], lens) * w.double()).sum().backward()
    leaves64a = [t.double().clone().requires_grad_(True) for t in (x, tr, st, en)]
    (U.path_score64(leaves64a[0], tags, *leaves64a[1:], lens) * w.double().abs()).sum().backward()
    got = [rewrap(z, leaves[0].grad).cat().data] + [l.grad for l in leaves[1:]]
    for g, l64, l64a in zip(got, leaves64, leaves64a):
        bound = (x.size(0) + 2) * u * l64a.grad.abs() + U.half_ulp(l64.grad, dtype)
        assert g.dtype == dtype and U.ratio(g, l64.grad, bound) <= 1.0
    none = z.crf_score(zt, tr.to(DEV))
    assert U.ratio(none, U.path_score64(x, tags, tr, None, None, lens), sb) <= 1.0


# ------------------------------------------------------------------ grid shapes
def test_more_sequences_than_waves():
    """B = 5 000 sequences of U(0, 12) tokens: more than the 1 024 parts of the backward and than the forward's grid, so
    the grid-stride loops and the finish launch run."""
    gen = torch.Generator().manual_seed(3)
    lens = tuple(torch.randint(0, 13, (5000,), generator=gen).tolist())
    x, tr, st, en, lt = U.case(5, F32, lens=lens, seed=13)
    w = U.draw((5000,), F32, 14).abs() + 0.5                    # (positive: the gradient is its own |g| form)
    bd = U.bounds(x, tr, st, en, lt, F32)
    want = want_abs = U.grads64(x, tr, st, en, lt, w)
    for kind in ('C', 'P'):
        got, _ = grads_gpu(kind, x, tr, st, en, lt, w)
        again, _ = grads_gpu(kind, x, tr, st, en, lt, w)
        z = build(kind, x.to(DEV), lt)
        logz = z.crf_partition(*gpu(tr, st, en))
        r = U.ratio(logz, want[0], bd['z'])
        U.note('logZ float32 B=5000', r)
        assert r <= 1.0
        p = want_abs[1] / torch.repeat_interleave(w.double().abs(), lt).unsqueeze(1)
        assert U.ratio(got[0], want[1], U.marginal_bound(p, bd, F32, lt, g=w)) <= 1.0
        for i in (1, 2, 3):
            assert same_bits(got[i], again[i])
            r = U.ratio(got[i], want[i + 1], U.param_bound(want[i + 1], want_abs[i + 1], bd, F32, x.size(0)))
            U.note('grad parameters float32 B=5000', r)
            assert r <= 1.0
        path = z.crf_decode(*gpu(tr, st, en))
        _, opt = U.viterbi64(x, tr, st, en, lt)
        assert U.ratio(path.score, opt, bd['z']) <= 1.0


def test_one_long_sequence_among_short_ones():
    lens = (3, 0, 7, 5000, 1, 2, 9, 4, 6, 5, 8)
    x, tr, st, en, lt = U.case(8, F32, lens=lens, seed=17)
    xg, trg, stg, eng = gpu(x, tr, st, en)
    bd = U.bounds(x, tr, st, en, lt, F32)
    ref = None
    for kind in ('C', 'L'):
        logz, marg, tags, score = run_all(build(kind, xg, lt), trg, stg, eng)
        r = U.ratio(logz, U.logz64(x, tr, st, en, lt), bd['z'])
        U.note('logZ float32 n=5000', r)
        assert r <= 1.0
        p = U.marginals64(x, tr, st, en, lt)
        r = U.ratio(marg, p, U.marginal_bound(p, bd, F32, lt))
        U.note('marginals float32 n=5000', r)
        assert r <= 1.0
        _, opt = U.viterbi64(x, tr, st, en, lt)
        assert U.ratio(score, opt, bd['z']) <= 1.0
        assert bool((opt - U.path_score64(x, tags.cpu(), tr, st, en, lt) <= 2 * bd['z']).all())
        if ref is not None:
            assert all(same_bits(a, b) for a, b in zip((logz, marg, tags, score), ref))
        ref = (logz, marg, tags, score)


def test_one_sequence_and_none():
    x, tr, st, en, lt = U.case(9, F32, lens=(17,), seed=19)
    xg, trg, stg, eng = gpu(x, tr, st, en)
    bd = U.bounds(x, tr, st, en, lt, F32)
    for kind in KINDS:
        logz, marg, tags, score = run_all(build(kind, xg, lt), trg, stg, eng)
        assert logz.shape == (1,) and U.ratio(logz, U.logz64(x, tr, st, en, lt), bd['z']) <= 1.0
        assert tags.shape == (17,)
    # B = 0: empty outputs, and nothing is launched (a null layout of no sequence would be refused by a launch)
    e0 = ta.C(torch.zeros(0, 9, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV))
    logz, marg, tags, score = run_all(e0, trg, stg, eng)
    assert logz.shape == (0,) and score.shape == (0,) and marg.shape == (0, 9) and tags.shape == (0,)
    t0 = ta.C(torch.zeros(0, dtype=torch.long, device=DEV), e0.token_sizes)
    assert e0.crf_score(t0, trg).shape == (0,)
    leaf = trg.clone().requires_grad_(True)
    e0.crf_partition(leaf, stg, eng).sum().backward()
    assert bool((leaf.grad == 0).all())
    # only empty sequences: logZ = 0 and zero gradients everywhere
    e1 = ta.C(torch.zeros(0, 9, device=DEV), torch.zeros(3, dtype=torch.long, device=DEV))
    leaf = trg.clone().requires_grad_(True)
    logz = e1.crf_partition(leaf, stg, eng)
    assert logz.tolist() == [0, 0, 0]
    logz.sum().backward()
    assert bool((leaf.grad == 0).all())
    assert e1.crf_decode(trg).score.tolist() == [0, 0, 0] and e1.crf_decode(trg).tags.data.shape == (0,)
