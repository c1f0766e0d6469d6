"""Yardsticks and bounds of the linear-chain CRF tests (tests/test_crf_surface.py on the CPU, tests/test_gpu_crf.py on the
GPU).  Every yardstick is float64 torch on the CPU on the inputs upcast exactly:

  forward_seq   the per-sequence forward recursion (alpha, logZ) — and, for the bounds only, the backward one (beta);
  batched64     the same two recursions for all sequences at once (the bounds, and batches of more than 64 sequences);
  viterbi64     Viterbi with the library's tie rule (the smallest index among the maxima, at every step and at the end);
  marginals64   the marginals by autograd of the float64 logZ (so not by the recursion the kernels use);
  brute         all K^n paths for K <= 3, n <= 5: logZ, the best path (ties: the smallest path read from its END, which
                is what "smallest backpointer" selects in exact arithmetic) and the marginals;
  path_score64  the score of a given path.

THE BOUND is derived from the evaluation order of csrc/rua_crf.hip, not from what the kernels give.  With u the unit
roundoff of the accumulator (2^-24; 2^-53 for float64) one step of the recursion for tag j is
    v_i = alpha[i] + transitions[i, j]           each off by the error d of alpha (inherited) + u |v_i|
    m = max_i v_i                                exact on the computed v
    e_i = exp(v_i - m)                           the difference: u |v_i - m|, the exp: 2 ulp = 4u; relative to s = sum e_i
                                                 a term weighs e_i / s <= e_i and (m - v_i) e^-(m - v_i) <= 1 / e, so the
                                                 differences cost at most 0.37 (K - 1) u of s, the exps 4u
    s = sum_i e_i  (ascending i)                 (K - 1) u
    log s                                        the relative error of s, + 2 ulp of |log s| <= log K: 4u log K
    m + log s,  x_t[j] + (...)                   u (|m| + log K),  u |alpha_t[j]|
logsumexp is 1-Lipschitz in the sup norm, so with A_t = max_j |alpha_t[j]| (the finite ones; an excluded -inf is
excluded in both computations), X = max |transitions| and c(K) = 1.37 (K - 1) + 4 + 5 log K:
    d_t <= d_{t-1} + u (2 (A_{t-1} + X) + A_t + c(K)),        d_0 = u A_0
    d_Z <= d_{n-1} + u (2 (A_{n-1} + E) + c(K))               E = max |end|
It grows with n and K and scales with 1 + |alpha|.  The float64 yardstick runs the same recursion sequentially and is off
by the same expression with u = 2^-53, which is added (invisible next to fp32, half of the bound for a float64 payload).
The backward recursion beta_{t-1}[i] = logsumexp_j(transitions[i, j] + (x_t[j] + beta_t[j])) has one more sum per step:
    d'_{t-1} <= d'_t + u (3 (B_t + X + |x_t|) + c(K)),        d'_{n-1} = 0
A marginal p = exp((alpha + beta) - logZ) has the exponent error D = d_t + d'_t + d_Z + u (A_t + B_t + min(|log p|, 110))
and then 2 ulp of the exp and one product with g:
    |p - want| <= 1.01 (D + 6u) want + 2^-126        (+ half an ulp of the output dtype for bf16 / f16: rounded once)
The parameter gradients are sums of |g_b| x pair marginals, each term with the relative error D_b + 16u at most (the pair
marginal reuses e_j and one more exp), added sequentially by a wave and then part by part: at most N + 1 024 additions,
    |grad - want| <= (1.01 (max_b D_b + 16u) + (N + 1 024) u) * G        G = the same gradient with |g_b| for g_b
(+ half an ulp of the output dtype).  The path scores of Viterbi follow the forward bound with c(K) = 0 (a max rounds
nothing); the tests use d_Z of the LOG recursion, which is larger."""
import itertools
import math

import torch

BF16, F16, F32, F64, I64 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64
NINF = -math.inf
REPORT = {}
BASE_LENS = (0, 1, 2, 5, 63, 64, 65, 130, 0, 3)
TAGS = (1, 2, 5, 8, 9, 33, 64)


def note(key, ratio):
    """Keep and print the worst achieved / bound ratio of `key` (the lines of profiles/crf_report.txt)."""
    REPORT[key] = max(REPORT.get(key, 0.0), float(ratio))
    print(f'crf report: {key} worst achieved/bound = {REPORT[key]:.4f}')


def bucket(K):
    return 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def name(dtype):
    return str(dtype).replace('torch.', '')


def draw(shape, dtype, seed, integers=False):
    """CPU inputs: standard normal rounded to `dtype`, or integers of [-3, 3] (exact sums in every dtype)."""
    gen = torch.Generator().manual_seed(seed)
    if integers:
        return torch.randint(-3, 4, shape, generator=gen).to(dtype)
    return torch.randn(shape, generator=gen, dtype=F64 if dtype == F64 else F32).to(dtype)


_cases = {}


def case(K, dtype, lens=BASE_LENS, seed=5, integers=False):
    """(x [N, K], transitions, start, end, lens) on the CPU; memoised, never modified."""
    key = (K, dtype, tuple(lens), seed, integers)
    if key not in _cases:
        n = sum(lens)
        _cases[key] = (draw((n, K), dtype, seed, integers), draw((K, K), dtype, seed + 1, integers),
                       draw((K,), dtype, seed + 2, integers), draw((K,), dtype, seed + 3, integers),
                       torch.tensor(lens, dtype=I64))
    return _cases[key]


def pieces(v, lens):
    return torch.split(v, [int(n) for n in lens], dim=0)


def lse(v, dim):
    """logsumexp that returns -inf (with zero gradients) where every term is -inf; NaN where one is NaN."""
    m = v.detach().amax(dim, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    s = torch.exp(v - m).sum(dim, keepdim=True)
    live = s > 0
    out = torch.where(live | torch.isnan(s), m + torch.log(torch.where(live, s, torch.ones_like(s))), torch.full_like(s, NINF))
    out = torch.where(torch.isnan(s), s, out)
    return out.squeeze(dim)


def _vec(v, like):
    return torch.zeros(like.size(-1), dtype=like.dtype) if v is None else v.to(like.dtype)


def forward_seq(x, trans, start, end, dtype=F64):
    """(alpha [n, K], logZ) of ONE sequence in `dtype` (float64: the yardstick; float32: the restatement)."""
    x, trans = x.to(dtype), trans.to(dtype)
    if x.size(0) == 0:
        return x, x.sum() * 0
    a = _vec(start, x) + x[0]
    rows = [a]
    for t in range(1, x.size(0)):
        a = x[t] + lse(a.unsqueeze(1) + trans, 0)
        rows.append(a)
    return torch.stack(rows), lse(a + _vec(end, x), 0)


def backward_seq(x, trans, end):
    """beta [n, K] of one sequence in float64 (for the bounds)."""
    x, trans = x.double(), trans.double()
    b = _vec(end, x)
    rows = [b]
    for t in range(x.size(0) - 1, 0, -1):
        b = lse(trans + (x[t] + b).unsqueeze(0), 1)
        rows.append(b)
    return torch.stack(rows[::-1]) if x.size(0) else x


def batched64(x, trans, start, end, lens):
    """(alpha [B, T, K], beta [B, T, K], logZ [B], the padded emissions [B, T, K], (b, t) of every token in cat order): the
    recursions of forward_seq / backward_seq for ALL sequences at once, float64 — T steps whatever B is.  A finished
    sequence keeps its alpha; positions past the end hold what the last step left (never read)."""
    x, trans = x.double(), trans.double()
    n = torch.as_tensor([int(v) for v in lens], dtype=I64)
    B, T, K = len(n), max(int(n.max()) if len(n) else 0, 1), x.size(1)
    ib = torch.repeat_interleave(torch.arange(B), n)
    it = torch.cat([torch.arange(int(v)) for v in n]) if len(n) else torch.zeros(0, dtype=I64)
    X = x.new_zeros(B, T, K).index_put((ib, it), x)
    st, en = _vec(start, x), _vec(end, x)
    a = st + X[:, 0]
    alphas = [a]
    for t in range(1, T):
        a = torch.where((n > t).unsqueeze(1), X[:, t] + lse(a.unsqueeze(2) + trans, 1), a)
        alphas.append(a)
    z = torch.where(n > 0, lse(a + en, 1), torch.zeros(B, dtype=F64))
    with torch.no_grad():
        b = en.expand(B, K)
        betas = [b]
        for t in range(T - 1, 0, -1):                      # beta_{t-1}, for the sequences with t <= n - 1
            b = torch.where((n - 1 >= t).unsqueeze(1), lse(trans + (X[:, t] + b).unsqueeze(1), 2), en.expand(B, K))
            betas.append(b)
    return torch.stack(alphas, 1), torch.stack(betas[::-1], 1), z, X, (ib, it)


def logz64(x, trans, start, end, lens):
    if len(lens) > 64:                                     # (the same recursion, all sequences at once)
        return batched64(x, trans, start, end, lens)[2]
    return torch.stack([forward_seq(p, trans, start, end)[1] for p in pieces(x, lens)]) if len(lens) else x.new_zeros(0).double()


def logz32(x, trans, start, end, lens):
    return torch.stack([forward_seq(p, trans, start, end, F32)[1] for p in pieces(x, lens)])


def grads64(x, trans, start, end, lens, w):
    """(logZ, d/dx, d/dtransitions, d/dstart, d/dend) of sum_b w_b logZ_b in float64 by autograd."""
    leaves = [t.double().clone().requires_grad_(True) for t in (x, trans, _vec(start, x.double()), _vec(end, x.double()))]
    z = logz64(leaves[0], leaves[1], leaves[2], leaves[3], lens)
    live = torch.isfinite(z)
    total = (torch.where(live, z, torch.zeros_like(z)) * w.double()).sum()
    g = torch.autograd.grad(total, leaves, allow_unused=True)
    return (z.detach(),) + tuple(torch.zeros_like(l) if gi is None else gi for gi, l in zip(g, leaves))


def marginals64(x, trans, start, end, lens):
    return grads64(x, trans, start, end, lens, torch.ones(len(lens), dtype=F64))[1]


def _first_max(v, dim):
    """(max, the SMALLEST index among the maxima) along `dim`."""
    m = v.amax(dim, keepdim=True)
    idx = torch.arange(v.size(dim)).reshape([-1 if d == dim else 1 for d in range(v.dim())]).expand_as(v)
    arg = torch.where(v == m, idx, torch.full_like(idx, v.size(dim))).amin(dim)
    return m.squeeze(dim), arg


def viterbi_seq(x, trans, start, end, dtype=F64):
    """(tags [n], score) of one sequence with the library's tie rule."""
    x, trans = x.to(dtype), trans.to(dtype)
    n = x.size(0)
    if n == 0:
        return torch.zeros(0, dtype=I64), x.sum() * 0
    a = _vec(start, x) + x[0]
    back = []
    for t in range(1, n):
        best, arg = _first_max(a.unsqueeze(1) + trans, 0)
        back.append(arg)
        a = x[t] + best
    score, tag = _first_max(a + _vec(end, x), 0)
    tags = [int(tag)]
    for arg in reversed(back):
        tags.append(int(arg[tags[-1]]))
    return torch.tensor(tags[::-1], dtype=I64), score


def viterbi64(x, trans, start, end, lens, dtype=F64):
    out = [viterbi_seq(p, trans, start, end, dtype) for p in pieces(x, lens)]
    return torch.cat([t for t, _ in out]), torch.stack([s for _, s in out])


def path_score_seq(x, tags, trans, start, end):
    x, trans = x.double(), trans.double()
    n = x.size(0)
    if n == 0:
        return x.sum() * 0
    s = x[torch.arange(n), tags].sum() + _vec(start, x)[tags[0]] + _vec(end, x)[tags[-1]]
    return s + trans[tags[:-1], tags[1:]].sum()


def path_score64(x, tags, trans, start, end, lens):
    return torch.stack([path_score_seq(p, q, trans, start, end) for p, q in zip(pieces(x, lens), pieces(tags, lens))])


def brute(x, trans, start, end):
    """(logZ, best path, marginals [n, K]) of one sequence by enumerating all K^n paths, float64."""
    x, trans = x.double(), trans.double()
    n, K = x.shape
    if n == 0:
        return x.sum() * 0, torch.zeros(0, dtype=I64), x
    paths = list(itertools.product(range(K), repeat=n))
    scores = torch.stack([path_score_seq(x, torch.tensor(p), trans, start, end) for p in paths])
    z = lse(scores, 0)
    top = scores.max()
    best = min((p for p, s in zip(paths, scores.tolist()) if s == top.item()), key=lambda p: p[::-1])
    marg = torch.zeros(n, K, dtype=F64)
    if torch.isfinite(z):
        for p, s in zip(paths, scores):
            marg[torch.arange(n), torch.tensor(p)] += torch.exp(s - z)
    return z, torch.tensor(best, dtype=I64), marg


# ------------------------------------------------------------------ the bound
def _amax(v):
    """max |finite entries| per row of [n, K]; 0 where there is none."""
    return torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v)).amax(-1) if v.numel() else v.new_zeros(v.shape[:-1])


def _fmax(v):
    return 0.0 if v is None or v.numel() == 0 else float(torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v)).max())


def c_of(K):
    return 1.37 * (K - 1) + 4 + 5 * math.log(K)


_bounds = {}


def bounds(x, trans, start, end, lens, dtype):
    """dict(z [B]: the bound of logZ; D [N]: the exponent error of the marginals of a token without its |log p| term;
    Dmax: the largest of them) for a kernel that accumulates in the accumulator of `dtype`, the float64 yardstick's own
    error included; see the module docstring.  Memoised on the identity of the (never modified) inputs."""
    key = (id(x), id(trans), id(start), id(end), tuple(int(n) for n in lens), dtype)
    if key in _bounds:
        return _bounds[key]
    u = (2.0 ** -53 if dtype == F64 else 2.0 ** -24) + 2.0 ** -53
    n = torch.as_tensor([int(v) for v in lens], dtype=I64)
    with torch.no_grad():
        alpha, beta, _, X, (ib, it) = batched64(x, trans, start, end, lens)
    B, T, K = alpha.shape
    pos = torch.arange(T).unsqueeze(0)
    A, Bt, xs = _amax(alpha) + 1, _amax(beta) + 1, _amax(X)
    Xm, E, c = _fmax(trans.double()), _fmax(end), c_of(K)
    # d_t = u A_0 + sum_{s = 1 .. t} u (2 (A_{s-1} + X) + A_s + c)
    inc = torch.zeros(B, T, dtype=F64)
    inc[:, 1:] = u * (2 * (A[:, :-1] + Xm) + A[:, 1:] + c)
    d = u * A[:, :1] + torch.cumsum(inc * (pos >= 1), 1)
    last = (n - 1).clamp_min(0).unsqueeze(1)
    dz = (d.gather(1, last) + u * (2 * (A.gather(1, last) + E) + c)).squeeze(1) * (n > 0)
    # d'_t = sum_{s = t + 1 .. n - 1} u (3 (B_s + X + |x_s|) + c)
    incb = u * (3 * (Bt + Xm + xs) + c) * ((pos >= 1) & (pos <= n.unsqueeze(1) - 1))
    db = incb.sum(1, keepdim=True) - torch.cumsum(incb, 1)
    D = (d + db + dz.unsqueeze(1) + u * (A + Bt))[ib, it]
    out = dict(z=dz, D=D, Dmax=float(D.max()) if D.numel() else 0.0, u=u,
               keep=(x, trans, start, end))            # (the ids of the key stay taken)
    _bounds[key] = out
    return out


def ulp_at(v64, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at the float64 values `v64`."""
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)
    _, e = torch.frexp(v64.abs().clamp_min(2.0 ** -140))
    return torch.ldexp(torch.ones_like(v64), (e - 1 - bits).clamp_min(lowest))


def half_ulp(want, dtype):
    return 0.5 * ulp_at(want, dtype) if dtype in (BF16, F16) else torch.zeros_like(want)


def marginal_bound(p, bd, dtype, lens, g=None):
    """The bound of the marginals [N, K] against the float64 marginals `p` — of g_b * p with a cotangent `g` [B]
    (grad_emissions)."""
    u = bd['u']
    logp = torch.where(p > 0, p.clamp_min(1e-300).log().abs().clamp_max(110.0), torch.full_like(p, 110.0))
    scale = torch.ones(p.size(0), 1, dtype=F64) if g is None else torch.repeat_interleave(g.double().abs(), lens).unsqueeze(1)
    bound = (1.01 * (bd['D'].unsqueeze(1) + u * logp + 6 * u) * p + 2.0 ** -126) * scale
    return bound + half_ulp(p * scale, dtype)


def param_bound(want, want_abs, bd, dtype, n_tokens):
    """The bound of a parameter gradient against the float64 `want`; `want_abs`: the same gradient with |g_b|."""
    u = bd['u']
    return (1.01 * (bd['Dmax'] + 116 * u + 16 * u) + (n_tokens + 1024) * u) * want_abs.abs() + 2.0 ** -126 + half_ulp(want, dtype)


def ratio(got, want, bound):
    """max |got - want| / bound over the finite wanted values; non-finite ones must match exactly."""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), 'NaN pattern'
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), 'infinities'
    if not fin.any():
        return 0.0
    bound = bound.expand_as(want) if isinstance(bound, torch.Tensor) else torch.full_like(want, bound)
    err = (got - want).abs()[fin]
    b = bound[fin]
    assert bool((err[b == 0] == 0).all()), 'a value that must be exact is not'
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
