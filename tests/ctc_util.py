"""Yardsticks and bounds of the CTC tests (tests/test_ctc_surface.py on the CPU, tests/test_gpu_ctc.py on the GPU).  Every
yardstick is float64 torch on the CPU on the inputs upcast exactly:

  forward_seq   the per-sequence DP over the extended target l' = (blank, y_0, blank, ..., blank) in the library's
                evaluation order — differentiable, so the gradient yardstick is AUTOGRAD of the float64 logZ, not the
                beta recursion the kernels use; with dtype=float32 it is the fp32 restatement;
  tables64      alpha, beta (without the emission at t) and logZ of one sequence, for the bounds only;
  viterbi_seq   the best alignment with the library's tie rule (ascending predecessor state s-2, s-1, s: the first of
                the maxima; at the end S'-2 before S'-1);
  brute         all V^T frame labellings of a tiny sequence, collapsed (repeats, then blanks) and compared with the target.

THE BOUND is derived from the evaluation order of csrc/rua_ctc.hip, not from what the kernels give.  With u the unit
roundoff of the accumulator (2^-24; 2^-53 for float64) one frame of the recursion for state s is
    v0, v1, v2 = alpha[s], alpha[s-1], alpha[s-2]     no arithmetic: off by the inherited error d alone
    m = max                                           exact on the computed v
    e_i = exp(v_i - m)                                the difference u |v_i - m|, the exp 2 ulp = 4u; relative to the sum a
                                                      term weighs (m - v_i) e^-(m - v_i) <= 1 / e: 0.37 * 2 u, and 4u
    s = e_0 + e_1 + e_2                               2u
    log s                                             the relative error of s, + 2 ulp of |log s| <= log 3: 4u log 3
    m + log s,  lp + (...)                            u (|m| + log 3),  u |alpha_t[s]|
logsumexp is 1-Lipschitz in the sup norm, so with A_t = 1 + max_s |alpha_t[s]| (the finite ones; an excluded -inf is
excluded in both computations) and c3 = 1.37 * 2 + 4 + 5 log 3 = 12.3 — crf_util's c(K) at K = 3, the PER-FRAME CONSTANT of
the three-term logsumexp —
    d_t <= d_{t-1} + u (A_{t-1} + A_t + c3),        d_0 = 0  (alpha_0 is a copy)
    d_Z <= d_{T-1} + u (A_{T-1} + c3)
accumulated along the path.  The float64 yardstick is off by the same expression with u = 2^-53, which is added.  The
loss is returned in the accumulator type, so nothing else is added to it.  The backward recursion adds the emission first
(u |u_s|) and bounds the new beta by B_t + X_t + log 3:
    d'_{t-1} <= d'_t + u (3 (B_t + X_t) + c3 + 2),   d'_{T-1} = 0,     X_t = max_s |lp_t[l'_s]|
A state posterior p = exp((alpha + beta) - logZ) has the exponent error D_t = d_t + d'_t + d_Z + u (A_t + B_t + |log p|) and
then 2 ulp of the exp; the class sum of n states adds (n + 8) u (sequential, or 64 parts and a butterfly of 6), the
product with g one more u:
    |grad - want| <= |g| (1.01 ((d_t + d'_t + d_Z + u (A_t + B_t) + (n_c + 16) u) P_c + u E_c) + 2^-126)
with P_c the float64 class posterior and E_c = sum_s p_s min(|log p_s|, 110), plus half an ulp of the output dtype for
bf16 / f16 (rounded once)."""
import itertools
import math

import torch

BF16, F16, F32, F64, I64 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64
NINF = -math.inf
REPORT = {}
C3 = 1.37 * 2 + 4 + 5 * math.log(3)


def note(key, ratio):
    """Keep and print the worst achieved / bound ratio of `key` (the lines of profiles/ctc_report.txt)."""
    REPORT[key] = max(REPORT.get(key, 0.0), float(ratio))
    print(f'ctc report: {key} worst achieved/bound = {REPORT[key]:.4f}')


def name(dtype):
    return str(dtype).replace('torch.', '')


def bucket(s_max):
    sp = 2 * s_max + 1
    return 'R1' if sp <= 64 else 'R2' if sp <= 128 else 'R4' if sp <= 256 else 'R8' if sp <= 512 else 'WG'


def draw_lp(n, V, dtype, seed, integers=False):
    """CPU log-probabilities [n, V]: a log_softmax of normals rounded to `dtype`, or integers of [-3, 0] (exact sums in
    every dtype, real ties)."""
    gen = torch.Generator().manual_seed(seed)
    if integers:
        return torch.randint(-3, 1, (n, V), generator=gen).to(dtype)
    x = torch.randn((n, V), generator=gen, dtype=F64)
    return x.log_softmax(-1).to(F64 if dtype == F64 else F32).to(dtype)


def draw_target(S, V, blank, seed, repeats=0, with_blank=False):
    """S labels != blank (unless with_blank), of which `repeats` equal their predecessor."""
    gen = torch.Generator().manual_seed(seed)
    classes = [c for c in range(V) if with_blank or c != blank]
    y = []
    for k in range(S):
        if k and k <= repeats:
            y.append(y[-1])
            continue
        pool = [c for c in classes if not y or c != y[-1]] or classes
        y.append(pool[int(torch.randint(0, len(pool), (1,), generator=gen))])
    return torch.tensor(y, dtype=I64)


def n_repeats(y):
    return int((y[1:] == y[:-1]).sum()) if y.numel() > 1 else 0


def pieces(v, lens):
    return torch.split(v, [int(n) for n in lens], dim=0)


# ------------------------------------------------------------------ the DP
def extended(y, blank):
    """(l' [S'], may the state take alpha[s-2]? [S'])"""
    S = int(y.numel())
    ext = torch.full((2 * S + 1,), blank, dtype=I64)
    ext[1::2] = y
    skip = torch.zeros(2 * S + 1, dtype=torch.bool)
    if S > 1:
        skip[3::2] = (y[1:] != blank) & (y[1:] != y[:-1])
    return ext, skip


def lse3(v0, v1, v2):
    """m + log(exp(v0 - m) + exp(v1 - m) + exp(v2 - m)) in that order; -inf (with zero gradients) where m == -inf; an
    absent term comes as -inf, which adds exp(-inf) = 0: the same bits."""
    m = torch.maximum(torch.maximum(v0, v1), v2).detach()
    nan = torch.isnan(v0) | torch.isnan(v1) | torch.isnan(v2)
    mm = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    s = torch.exp(v0 - mm) + torch.exp(v1 - mm) + torch.exp(v2 - mm)
    live = s > 0
    out = torch.where(live, mm + torch.log(torch.where(live, s, torch.ones_like(s))), torch.full_like(s, NINF))
    return torch.where(nan, torch.full_like(s, math.nan), out)


def _shift(a, k):
    return torch.cat([a.new_full((k,), NINF), a[:-k]]) if k < a.numel() else a.new_full(a.shape, NINF)


def forward_seq(lp, y, blank, dtype=F64):
    """logZ of ONE sequence (lp [T, V], y [S]) in `dtype`; T = 0: 0 for S = 0, else -inf."""
    lp = lp.to(dtype)
    T, S = lp.size(0), int(y.numel())
    if T == 0:
        return lp.sum() * 0 + (0.0 if S == 0 else NINF)
    ext, skip = extended(y, blank)
    x = lp[:, ext]
    start = torch.zeros(2 * S + 1, dtype=torch.bool)
    start[:2] = True
    a = torch.where(start, x[0], torch.full_like(x[0], NINF))
    for t in range(1, T):
        f = lse3(a, _shift(a, 1), torch.where(skip, _shift(a, 2), torch.full_like(a, NINF)))
        a = torch.where(f == NINF, torch.full_like(f, NINF), x[t] + f)
    va = a[-1:]
    vb = a[-2:-1] if S else va.new_full((1,), NINF)
    return lse3(va, vb, va.new_full((1,), NINF)).squeeze(0)


def loss64(lp, lens, y, ylens, blank, dtype=F64):
    """-logZ [B] of a batch given in cat order."""
    out = [-forward_seq(p, q, blank, dtype) for p, q in zip(pieces(lp, lens), pieces(y, ylens))]
    return torch.stack(out) if out else torch.zeros(0, dtype=dtype)


def grads64(lp, lens, y, ylens, blank, w):
    """(loss [B], d/dlp of sum_b w_b loss_b) in float64 by AUTOGRAD; a sequence without alignment contributes zeros."""
    leaf = lp.double().clone().requires_grad_(True)
    loss = loss64(leaf, lens, y, ylens, blank)
    live = torch.isfinite(loss)
    total = (torch.where(live, loss, torch.zeros_like(loss)) * w.double()).sum()
    g, = torch.autograd.grad(total, leaf, allow_unused=True)
    return loss.detach(), torch.zeros_like(leaf) if g is None else g


def tables64(lp, y, blank):
    """(alpha [T, S'], beta [T, S'], logZ) of one sequence, float64, no graph; beta excludes the emission at t."""
    with torch.no_grad():
        lp = lp.double()
        T, S = lp.size(0), int(y.numel())
        ext, skip = extended(y, blank)
        x = lp[:, ext]
        ninf = x.new_full((2 * S + 1,), NINF)
        if T == 0:
            return x, x, torch.tensor(0.0 if S == 0 else NINF, dtype=F64)
        start = torch.zeros(2 * S + 1, dtype=torch.bool)
        start[:2] = True
        a = torch.where(start, x[0], ninf)
        alphas = [a]
        for t in range(1, T):
            f = lse3(a, _shift(a, 1), torch.where(skip, _shift(a, 2), ninf))
            a = torch.where(f == NINF, ninf, x[t] + f)
            alphas.append(a)
        z = lse3(a[-1:], a[-2:-1] if S else a.new_full((1,), NINF), a.new_full((1,), NINF)).squeeze(0)
        b = ninf.clone()
        b[-2:] = 0.0
        betas = [b]
        up = lambda v, k: torch.cat([v[k:], v.new_full((k,), NINF)]) if k < v.numel() else v.new_full(v.shape, NINF)
        skip_up = torch.cat([skip[2:], torch.zeros(2, dtype=torch.bool)])[:2 * S + 1]
        for t in range(T - 1, 0, -1):
            u = torch.where(b == NINF, ninf, x[t] + b)
            b = lse3(u, up(u, 1), torch.where(skip_up, up(u, 2), ninf))
            betas.append(b)
        return torch.stack(alphas), torch.stack(betas[::-1]), z


def _first_max(cands):
    """(max, the index of the FIRST of the maxima) over dim 0 of [n, S']."""
    m = cands.amax(0)
    idx = torch.arange(cands.size(0)).unsqueeze(1).expand_as(cands)
    arg = torch.where(cands == m, idx, torch.full_like(idx, cands.size(0))).amin(0)
    return m, arg


def viterbi_seq(lp, y, blank):
    """(labels [T], positions [T], score) of one sequence, float64, with the library's tie rule; no alignment: all blank,
    -1 and -inf.  (NaN-free inputs.)"""
    lp = lp.double()
    T, S = lp.size(0), int(y.numel())
    if T == 0:
        return torch.zeros(0, dtype=I64), torch.zeros(0, dtype=I64), torch.tensor(0.0 if S == 0 else NINF, dtype=F64)
    ext, skip = extended(y, blank)
    x = lp[:, ext]
    ninf = x.new_full((2 * S + 1,), NINF)
    start = torch.zeros(2 * S + 1, dtype=torch.bool)
    start[:2] = True
    a = torch.where(start, x[0], ninf)
    codes = []
    for t in range(1, T):
        best, arg = _first_max(torch.stack([torch.where(skip, _shift(a, 2), ninf), _shift(a, 1), a]))
        codes.append(2 - arg)
        a = torch.where(best == NINF, ninf, x[t] + best)
    if S and a[-2] >= a[-1]:
        score, s = a[-2], 2 * S - 1
    else:
        score, s = a[-1], 2 * S
    if score == NINF:
        return torch.full((T,), blank, dtype=I64), torch.full((T,), -1, dtype=I64), score
    states = [s]
    for code in reversed(codes):
        s -= int(code[s])
        states.append(s)
    states = torch.tensor(states[::-1], dtype=I64)
    pos = torch.where(states % 2 == 1, states // 2, torch.full_like(states, -1))
    return ext[states], pos, score


def collapse(path, blank):
    out = [c for c, _ in itertools.groupby(path)]
    return [c for c in out if c != blank]


def brute(lp, y, blank):
    """logZ of one tiny sequence by enumerating all V^T frame labellings, float64."""
    lp = lp.double()
    T, V = lp.shape
    if T == 0:
        return torch.tensor(0.0 if y.numel() == 0 else NINF, dtype=F64)
    want = y.tolist()
    scores = [lp[torch.arange(T), torch.tensor(p)].sum() for p in itertools.product(range(V), repeat=T)
              if collapse(p, blank) == want]
    if not scores:
        return torch.tensor(NINF, dtype=F64)
    s = torch.stack(scores)
    m = s.max()
    return m if m == NINF else m + torch.log(torch.exp(s - m).sum())


# ------------------------------------------------------------------ the bound
def _amax(v):
    """1 + max |finite entries| per row of [T, n]."""
    return 1 + torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v)).amax(-1)


_bounds = {}


def bounds(lp, lens, y, ylens, blank, dtype):
    """dict(z [B]: the bound of the loss; g [N, V]: the bound of the gradient per unit |g_b|, without the rounding of the
    output) for kernels that accumulate in the accumulator of `dtype`, the float64 yardstick's own error included; see the
    module docstring.  Memoised on the identity of the (never modified) inputs."""
    key = (id(lp), id(y), tuple(int(n) for n in lens), tuple(int(n) for n in ylens), blank, dtype)
    if key in _bounds:
        return _bounds[key]
    u = (2.0 ** -53 if dtype == F64 else 2.0 ** -24) + 2.0 ** -53
    zs, gs = [], []
    for p, q in zip(pieces(lp, lens), pieces(y, ylens)):
        T, V = p.shape
        alpha, beta, z = tables64(p, q, blank)
        if T == 0:
            zs.append(0.0)
            continue
        ext, _ = extended(q, blank)
        A, Bt = _amax(alpha), _amax(beta)
        X = torch.where(torch.isfinite(p.double()[:, ext]), p.double()[:, ext].abs(), torch.zeros(T, ext.numel(), dtype=F64)).amax(-1)
        inc = torch.zeros(T, dtype=F64)
        inc[1:] = u * (A[:-1] + A[1:] + C3)
        d = torch.cumsum(inc, 0)
        dz = float(d[-1] + u * (A[-1] + C3))
        zs.append(dz)
        incb = torch.zeros(T, dtype=F64)
        incb[1:] = u * (3 * (Bt[1:] + X[1:]) + C3 + 2)
        db = incb.sum() - torch.cumsum(incb, 0)                  # d'_t = the increments of t + 1 .. T - 1
        if not torch.isfinite(z):
            gs.append(torch.zeros(T, V, dtype=F64))
            continue
        logp = (alpha + beta) - z
        post = torch.exp(logp)
        ent = post * torch.where(post > 0, logp.abs().clamp_max(110.0), torch.zeros_like(post))
        P = torch.zeros(T, V, dtype=F64).index_add_(1, ext, post)
        E = torch.zeros(T, V, dtype=F64).index_add_(1, ext, ent)
        n_c = torch.zeros(V, dtype=F64).index_add_(0, ext, torch.ones(ext.numel(), dtype=F64))
        D = (d + db + dz + u * (A + Bt)).unsqueeze(1) + (n_c + 16).unsqueeze(0) * u
        gs.append(1.01 * (D * P + u * E) + 2.0 ** -126)
    out = dict(z=torch.tensor(zs, dtype=F64), g=torch.cat(gs) if gs else torch.zeros(0, lp.size(1), dtype=F64), u=u,
               keep=(lp, y))
    _bounds[key] = out
    return out


def ulp_at(v64, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at the float64 values `v64`."""
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)
    _, e = torch.frexp(v64.abs().clamp_min(2.0 ** -140))
    return torch.ldexp(torch.ones_like(v64), (e - 1 - bits).clamp_min(lowest))


def half_ulp(want, dtype):
    return 0.5 * ulp_at(want, dtype) if dtype in (BF16, F16) else torch.zeros_like(want)


def grad_bound(want, bd, dtype, lens, g):
    """The bound of the gradient [N, V] against the float64 `want`, for the cotangent g [B]."""
    scale = torch.repeat_interleave(g.double().abs(), torch.as_tensor([int(n) for n in lens])).unsqueeze(1)
    return bd['g'] * scale + half_ulp(want, dtype)


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


# ------------------------------------------------------------------ the GPU tests' inputs (shared with the CPU tests)
_cases = {}


def edge_case(s_max, dtype, V=8, blank=0, seed=11):
    """(lp [N, V], lens, y [M], ylens) on the CPU, memoised, never modified: a batch of 6 whose longest target has
    `s_max` labels with two repeats (T = S + repeats + 3), next to S = 0, T = 0 and short sequences."""
    key = ('edge', s_max, dtype, V, blank, seed)
    if key not in _cases:
        ys = [draw_target(s_max, V, blank, seed, repeats=min(2, max(s_max - 1, 0))),
              draw_target(0, V, blank, seed), draw_target(min(3, s_max), V, blank, seed + 1),
              draw_target(0, V, blank, seed), draw_target(min(s_max, 5), V, blank, seed + 2, repeats=min(1, max(s_max - 1, 0))),
              draw_target(min(1, s_max), V, blank, seed + 3)]
        ts = [int(q.numel()) + n_repeats(q) + 3 for q in ys]
        ts[1], ts[3] = 4, 0                                   # S = 0 with frames; T = 0 and S = 0
        lens, ylens = torch.tensor(ts, dtype=I64), torch.tensor([int(q.numel()) for q in ys], dtype=I64)
        _cases[key] = (draw_lp(sum(ts), V, dtype, seed + 7), lens, torch.cat(ys), ylens)
    return _cases[key]
