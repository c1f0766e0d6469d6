"""The yardstick of attention_decode next to attention_band_util.reference (which gives `out`, its bound b_out and A): a
float64 logsumexp of the scaled visible scores from the rounded inputs, and the two terms the decode kernel adds.

MERGE TERM.  A result is merged from 4 + n_split partial softmax states (m_i, l_i, acc_i): the four waves of a
workgroup, then the splits.  Merging one partial costs, in fp32, an exp (the factor f_i = exp(m_i - m*)), a multiply
(f_i acc_i) and an add for the weights, and the same three for l — 6 operations of at most one step e = 2^-23 each,
relative to a sum of non-negative terms that never exceeds the final one (A for the weighted values, l for the
normaliser).  With the file's 1.01:  merge(n_split) = 1.01 * 6 * (4 + n_split) * e,  times A for `out`.  It is added to
b_out and replaces nothing in it (b_out keeps S adds and a rescale per 32 keys although a wave sees a quarter of them).

LSE.  attention_util: an exponent argument is off by d_t, the normaliser by the factor d_t + (S + 8) e; lse = m + log l
adds the rounding of log l and of the add, each at most 2 e (|m| + |log l|) <= 2 e (smax + |lse| + smax), bounded here as
4 e (smax + |lse|) with the 1.01:  b_lse = 1.01 (d_t + (S + 8) e + 4 e (smax + |lse|)) + merge(n_split).  A query with
no visible key has lse = -inf exactly (bound 0)."""
import math

import torch

from attention_band_util import E, F64, hide_of


def merge_term(n_split):
    return 1.01 * 6 * (4 + n_split) * E


def lse_reference(q, qlens, k, klens, mask, scale, n_split):
    """(lse, bound), each [sum(qlens), heads] float64; `mask` is (align, left, right)."""
    sc, G, D = (q.size(-1) ** -0.5 if scale is None else scale), q.size(1) // k.size(1), q.size(-1)
    lses, bounds = [], []
    for a, b in zip(q.to(F64).split(qlens), k.to(F64).split(klens)):
        T, S = a.size(0), b.size(0)
        if T == 0:
            continue
        if S == 0:
            lses.append(torch.full((T, a.size(1)), -math.inf, dtype=F64))
            bounds.append(torch.zeros(T, a.size(1), dtype=F64))
            continue
        hide, ke = hide_of(T, S, *mask), b.repeat_interleave(G, 1)
        dead = hide.all(-1)
        s = (sc * torch.einsum('thd,shd->hts', a, ke)).masked_fill(hide, -math.inf)
        lse = s.masked_fill(dead[:, None], 0.0).logsumexp(-1).masked_fill(dead, -math.inf)          # [H, T]
        sabs = sc * torch.einsum('thd,shd->hts', a.abs(), ke.abs()).masked_fill(hide, 0)
        smax = s.masked_fill(hide, 0).abs().amax(-1)
        d_t = (D + 2) * E * sabs.amax(-1) + 8 * E * (1 + smax)
        bound = 1.01 * (d_t + (S + 8) * E + 4 * E * (smax + lse.masked_fill(dead, 0.0).abs())) + merge_term(n_split)
        lses.append(lse.t())
        bounds.append(bound.masked_fill(dead, 0.0).t())
    return torch.cat(lses), torch.cat(bounds)
