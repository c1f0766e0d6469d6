"""The yardstick of the attention tests: a per-sequence, per-head float64 evaluation of the definition, from the already
rounded inputs, its gradients from float64 autograd, and the error bounds of DESIGN 3.2r next to them.

u is the half-ulp of the payload type, e = 2^-23 one fp32 step (a whole ulp: the matrix unit's adds are not promised
to round to nearest), A = sum_s p |v|.  An exponent argument of row t is off by at most d_t = (D + 2) e max_s sc |q|.|k|
+ 8 e (1 + max_s |s|), a weight therefore by the factor r_t = 2 d_t + (S + 8) e (its normaliser included), lse by d_t +
(S + 8) e + 2 e |lse|.  The forward: one rounding of P, one of the output, the weights, S adds and a rescale per block of
32 keys: (2 u + 1.01 (r_t + (S + 3 ceil(S / 32) + 8) e)) A.  The gradients repeat the pattern with the roundings the
backward performs — P~ in dV, dS once, the saved output inside delta (its own forward bound), the final one — see the
code, which is the derivation term by term.  f16 only: a weight or dS below 2^-14 is rounded to a subnormal, 2^-25
absolute each (of the weights only one with p < 2^-14 can be: the stored exp(s - running max) is never below the final
p), and the final rounding of every result is u max(|x|, 2^-14), 2^-14 the smallest normal.  The bf16 kernels carry P as
hi + lo into P V and P^T dO; the u of P stays in the bound, an over-estimate there."""
import math

import torch

BF16, F16, F64 = torch.bfloat16, torch.float16, torch.float64
U = {BF16: 2.0 ** -9, F16: 2.0 ** -11}
E = 2.0 ** -23
REPORT = {}


def note(key, ratio):
    """Keep and print the worst achieved / bound ratio of `key` (the lines of profiles/attention_report.txt)."""
    REPORT[key] = max(REPORT.get(key, 0.0), float(ratio))
    print(f'attention report: {key} worst achieved/bound = {REPORT[key]:.4f}')


def draw(lens, heads, D, dtype, seed):
    """CPU payloads [sum(lens), heads, D] of normals, rounded to `dtype`."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((int(sum(lens)), heads, D), generator=gen, dtype=torch.float32).to(dtype)


def one(q, k, v, g, causal, sc, dtype):
    """One sequence: q, g [T, H, D], k, v [S, H, D] float64.  (out, dq, dk, dv), (their bounds), A."""
    T, S, D, u = q.size(0), k.size(0), q.size(2), U[dtype]
    sub = 2.0 ** -25 if dtype == F16 else 0.0
    floor = 2.0 ** -14 if dtype == F16 else 2.0 ** -126        # the smallest normal: below it a rounding is absolute
    if S == 0 or T == 0:
        z = [torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)]
        return z, [torch.zeros_like(t) for t in z], torch.zeros_like(q)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    hide = torch.ones(T, S, dtype=torch.bool).triu(1) if causal else torch.zeros(T, S, dtype=torch.bool)
    s = (sc * torch.einsum('thd,shd->hts', q, k)).masked_fill(hide, -math.inf)
    p = s.softmax(-1)
    out = torch.einsum('hts,shd->thd', p, v)
    grads = torch.autograd.grad(out, (q, k, v), g)
    with torch.no_grad():
        qa, ka, va, ga = q.abs(), k.abs(), v.abs(), g.abs()
        sabs = sc * torch.einsum('thd,shd->hts', qa, ka).masked_fill(hide, 0)
        smax = s.masked_fill(hide, 0).abs().amax(-1)                             # [H, T]
        lse = s.logsumexp(-1)
        d_t = (D + 2) * E * sabs.amax(-1) + 8 * E * (1 + smax)
        r_t = 2 * d_t + (S + 8) * E
        A = torch.einsum('hts,shd->thd', p, va)
        tiny = sub * ((p < 2.0 ** -14) & ~hide).to(F64)          # a weight p >= 2^-14 is stored >= 2^-14: no subnormal
        b_out = (u * A.clamp_min(floor) + (u + 1.01 * (r_t + (S + 3 * math.ceil(S / 32) + 8) * E)).t().unsqueeze(-1) * A +
                 torch.einsum('hts,shd->thd', tiny, va))
        # the backward recomputes P from lse: the factor of a weight there
        rb = 1.01 * (2 * d_t + (S + 12 + 4 * (smax + lse.abs())) * E)            # [H, T]
        b_dv = torch.einsum('hts,thd->shd', p * (u + rb + (T + 8) * E).unsqueeze(-1), ga) + torch.einsum('hts,thd->shd', tiny, ga)
        b_dv = b_dv + u * (grads[2].abs() + b_dv).clamp_min(floor)
        delta = (g * out).sum(-1).t()                                            # [H, T]
        d_delta = ((ga * b_out).sum(-1) + (D + 1) * E * 1.01 * (ga * out.abs()).sum(-1)).t()
        dp = torch.einsum('thd,shd->hts', g, v)
        d_dp = (D + 8) * E * torch.einsum('thd,shd->hts', ga, va)
        ds = p * (dp - delta.unsqueeze(-1))
        e_ds = u * ds.abs() + sub + 1.01 * (rb.unsqueeze(-1) * ds.abs() + p * (d_dp + d_delta.unsqueeze(-1)) +
                                            2 * E * p * (dp.abs() + delta.abs().unsqueeze(-1)) + 2 * E * ds.abs())
        e_ds = e_ds.masked_fill(hide, 0)
        acc_q = sc * (torch.einsum('hts,shd->thd', e_ds, ka) + (S + 10) * E * torch.einsum('hts,shd->thd', ds.abs(), ka))
        acc_k = sc * (torch.einsum('hts,thd->shd', e_ds, qa) + (T + 10) * E * torch.einsum('hts,thd->shd', ds.abs(), qa))
        b_dq = acc_q + u * (grads[0].abs() + acc_q).clamp_min(floor)
        b_dk = acc_k + u * (grads[1].abs() + acc_k).clamp_min(floor)
    return [out.detach(), *grads], [b_out, b_dq, b_dk, b_dv], A


def reference(q, qlens, k, v, klens, g, causal, scale, dtype):
    """The batch, a plain loop over the sequences (cat form in, cat form out): (out, dq, dk, dv), bounds, A."""
    sc = q.size(-1) ** -0.5 if scale is None else scale
    parts = [one(a.to(F64), b.to(F64), c.to(F64), d.to(F64), causal, sc, dtype)
             for a, b, c, d in zip(q.split(qlens), k.split(klens), v.split(klens), g.split(qlens))]
    cat = lambda pick: [torch.cat([pick(p)[i] for p in parts]) for i in range(4)]           # noqa: E731
    return cat(lambda p: p[0]), cat(lambda p: p[1]), torch.cat([p[2] for p in parts])


def check(key, got, want, bound):
    """achieved <= bound element-wise (after noting the worst ratio); where the bound is 0 the result is exact."""
    err = (got.to(F64) - want).abs()
    note(key, (err / bound.clamp_min(1e-300)).max() if err.numel() else 0.0)
    assert bool((err <= bound).all()), key
