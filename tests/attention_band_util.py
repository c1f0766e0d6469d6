"""The yardstick of the band form of attention (grouped-query heads, windows, end-aligned masks): attention_util.one /
reference restated with the hide mask passed in — built from (left, right, align, T, S) — and the group factor G.  float64
from the rounded inputs; K / V are expanded over the group INSIDE autograd, so dk / dv come out summed; a row with no
visible key has p = 0 (not NaN), want = 0 and bound = 0.  The bounds are attention_util's derivation term by term with
`hide` general: S and T in the add-count terms stay the full lengths (the visible count is smaller), for dk / dv the
add count is G T, and the accumulation parts (acc_k, the pre-rounding part of b_dv) are summed over the group before the
single final rounding is applied."""
import math

import torch

from attention_util import BF16, E, F16, F64, REPORT, U, check, draw, note  # noqa: F401  (the tests take them from here)


def hide_of(T, S, align, left, right):
    """[T, S] bool: key s is hidden from query t unless -left <= s - (t + shift) <= right (None: unbounded)."""
    d = torch.arange(S)[None, :] - (torch.arange(T)[:, None] + (S - T if align == 'end' else 0))
    hide = torch.zeros(T, S, dtype=torch.bool)
    for bound, out in ((left, lambda w: d < -w), (right, lambda w: d > w)):
        hide = hide | out(bound) if bound is not None else hide
    return hide


def one(q, k, v, g, hide, G, sc, dtype):
    """One sequence: q, g [T, H, D], k, v [S, H / G, D] float64.  (out, dq, dk, dv), (their bounds), A."""
    T, S, D, u = q.size(0), k.size(0), q.size(2), U[dtype]
    sub = 2.0 ** -25 if dtype == F16 else 0.0
    floor = 2.0 ** -14 if dtype == F16 else 2.0 ** -126
    if S == 0 or T == 0:
        z = [torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)]
        return z, [torch.zeros_like(t) for t in z], torch.zeros_like(q)
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    ke, ve = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
    dead = hide.all(-1)                                                          # [T]: no visible key
    s = (sc * torch.einsum('thd,shd->hts', q, ke)).masked_fill(hide, -math.inf).masked_fill(dead[:, None], 0.0)
    p = s.softmax(-1) * (~dead)[:, None]
    out = torch.einsum('hts,shd->thd', p, ve)
    grads = torch.autograd.grad(out, (q, k, v), g)
    group = lambda x: x.reshape(S, -1, G, D).sum(2)                              # noqa: E731  [S, H, D] -> [S, H / G, D]
    with torch.no_grad():
        qa, ka, va, ga = q.abs(), ke.abs(), ve.abs(), g.abs()
        sabs = sc * torch.einsum('thd,shd->hts', qa, ka).masked_fill(hide, 0)
        smax = s.masked_fill(hide, 0).abs().amax(-1)                             # [H, T]
        lse = s.logsumexp(-1)
        d_t = (D + 2) * E * sabs.amax(-1) + 8 * E * (1 + smax)
        r_t = 2 * d_t + (S + 8) * E
        A = torch.einsum('hts,shd->thd', p, va)
        tiny = sub * ((p < 2.0 ** -14) & ~hide).to(F64)
        b_out = (u * A.clamp_min(floor) + (u + 1.01 * (r_t + (S + 3 * math.ceil(S / 32) + 8) * E)).t().unsqueeze(-1) * A +
                 torch.einsum('hts,shd->thd', tiny, va))
        rb = 1.01 * (2 * d_t + (S + 12 + 4 * (smax + lse.abs())) * E)            # [H, T]
        b_dv = group(torch.einsum('hts,thd->shd', p * (u + rb + (G * T + 8) * E).unsqueeze(-1), ga) +
                     torch.einsum('hts,thd->shd', tiny, ga))
        b_dv = b_dv + u * (grads[2].abs() + b_dv).clamp_min(floor)
        delta = (g * out).sum(-1).t()                                            # [H, T]
        d_delta = ((ga * b_out).sum(-1) + (D + 1) * E * 1.01 * (ga * out.abs()).sum(-1)).t()
        dp = torch.einsum('thd,shd->hts', g, ve)
        d_dp = (D + 8) * E * torch.einsum('thd,shd->hts', ga, va)
        ds = p * (dp - delta.unsqueeze(-1))
        e_ds = u * ds.abs() + sub + 1.01 * (rb.unsqueeze(-1) * ds.abs() + p * (d_dp + d_delta.unsqueeze(-1)) +
                                            2 * E * p * (dp.abs() + delta.abs().unsqueeze(-1)) + 2 * E * ds.abs())
        e_ds = e_ds.masked_fill(hide, 0)
        acc_q = sc * (torch.einsum('hts,shd->thd', e_ds, ka) + (S + 10) * E * torch.einsum('hts,shd->thd', ds.abs(), ka))
        acc_k = sc * group(torch.einsum('hts,thd->shd', e_ds, qa) + (G * T + 10) * E * torch.einsum('hts,thd->shd', ds.abs(), qa))
        alive = (~dead).to(F64)[:, None, None]                                   # no visible key: exact zeros
        b_out, b_dq = b_out * alive, (acc_q + u * (grads[0].abs() + acc_q).clamp_min(floor)) * alive
        b_dk = acc_k + u * (grads[1].abs() + acc_k).clamp_min(floor)
    return [out.detach(), *grads], [b_out, b_dq, b_dk, b_dv], A


def reference(q, qlens, k, v, klens, g, mask, scale, dtype):
    """The batch, a plain loop over the sequences (cat form in and out): (out, dq, dk, dv), bounds, A.  `mask` is
    (align, left, right); G follows from the head counts."""
    sc, G = (q.size(-1) ** -0.5 if scale is None else scale), q.size(1) // k.size(1)
    parts = [one(a.to(F64), b.to(F64), c.to(F64), d.to(F64), hide_of(a.size(0), b.size(0), *mask), G, sc, dtype)
             for a, b, c, d in zip(q.split(qlens), k.split(klens), v.split(klens), g.split(qlens))]
    cat = lambda pick: [torch.cat([pick(p)[i] for p in parts]) for i in range(4)]           # noqa: E731
    return cat(lambda p: p[0]), cat(lambda p: p[1]), torch.cat([p[2] for p in parts])
