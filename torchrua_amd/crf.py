"""Per-sequence linear-chain CRF over the tokens of any container (C / L / P / R) of emissions — an extension: the one
structured operator the reference's users build on these containers (sequence labelling, CTC-like alignment, torchlatent).
The stock spellings are `z.left()` plus a Python loop of T launches of torch.logsumexp over a [B, K, K] broadcast (padded,
hand-masked, wrong for an R without more care, nothing for a PackedSequence), or a tree of [N, K, K] matrices through
`segment_logsumexp` at K times the memory.  Here the log partition function, its gradients and Viterbi are fused HIP
kernels (csrc/rua_crf.hip), identical for the four layouts.

`e` is a container of emissions with exactly ONE hidden dimension, the K tags, 1 <= K <= 64: e.data is [N, K] for C / P
and [B, T_phys, K] for L / R.  `transitions` is [K, K]; transitions[i, j] scores tag i at t-1 followed by tag j at t.
`start` / `end` are [K] or None; None adds nothing, no zeros tensor is materialised, and the result equals the one with a
zeros tensor bit for bit.  All share the emissions' device and dtype: float32, float64, bfloat16 or float16;
accumulation is fp32 (fp64 for float64).

    crf_partition(e, transitions, start=None, end=None) -> Tensor [B]            also e.crf_partition(...)
        log Z of every sequence, in the batch order of `reduce_sum` (a P: the original order), in FLOAT32 (float64 for
        float64 emissions) — never rounded to bf16 / f16: the NLL `logZ - score` cancels, and eight bits of mantissa on
        a value of a few hundred would be useless.
            alpha_0[j] = start[j] + x_0[j]
            alpha_t[j] = x_t[j] + logsumexp_i(alpha_{t-1}[i] + transitions[i, j])
            logZ[b]    = logsumexp_j(alpha_{n-1}[j] + end[j])
    segment_crf_partition(tensor, transitions, sizes, start=None, end=None)     the `segment_*` argument style
    crf_marginals(e, transitions, start=None, end=None) -> container of e's type, shape and dtype
        P(tag_t = j) per token and tag, exp(alpha + beta - logZ), rounded once; padding rows are zeros.  The forward
        and the backward kernel with a cotangent of ones; no graph is built.
    crf_decode(e, transitions, start=None, end=None) -> SeqPath(tags, score)
        Viterbi.  `tags` is an int64 container of e's type and token layout ([N], or [B, T_phys] with zero padding) that
        reuses e's metadata objects; `score` [B] (float32 / float64) is the best path's score, evaluated in the
        recursion's own order.  Nothing is read back; neither output is differentiable.
    crf_score(e, tags, transitions, start=None, end=None) -> Tensor [B]
        The score of a given path, float32 / float64: a composition of the library's differentiable pieces (`cat`,
        `segment_sum`) and plain torch indexing — like `topk` it has no kernel of its own.  Differentiable in e,
        transitions, start and end, which makes `crf_partition(...) - crf_score(...)` a trainable loss.

SEMANTICS.  An empty sequence gives logZ = 0, score = 0, no tags and zero gradients everywhere.  -inf in `transitions`,
`start`, `end` or the emissions is a forbidden move (BIO constraints) and is first-class: an unreachable tag has
alpha = -inf, never NaN (a logsumexp whose max is -inf returns -inf); if EVERY path of a sequence is forbidden,
logZ = -inf and that sequence's gradients and marginals are exact zeros (a documented choice).  A NaN poisons only its
own sequence (and, through their sums, the parameter gradients).  +inf is out of scope: inf or NaN, in that sequence only.

ONE evaluation order per (sequence, tag, step): v_i = alpha[i] + transitions[i, j] for i = 0 .. K-1, m = max_i v_i,
s = sum_i exp(v_i - m) in ascending i, alpha_t[j] = x_t[j] + (m + log s) — so crf_partition, crf_marginals and crf_decode
give the same bits for e, e.cat(), e.pack(), e.left() and e.right(); for the container outputs this is the commutation
op(z).cat() == op(z.cat()) of the other operators.  VITERBI TIES: the backpointer at (t, j) is the SMALLEST i among the
maxima of alpha_{t-1}[i] + transitions[i, j], the last tag the smallest j among the maxima of alpha_{n-1}[j] + end[j] —
`argmax`'s rule (a NaN beats every number, the first NaN wins): every input has exactly one answer.

AUTOGRAD of crf_partition: gradients flow to the emissions, `transitions`, `start` and `end`.  It saves the [rows, K]
forward table alpha in the accumulator type, in the emissions' storage layout, plus logZ and the inputs;
grad_emissions[t, j] = g[b] * marginal, rounded once, exact zeros in padding rows.  The parameter gradients use no float
atomics (a part per wave, added in part order by a finish launch): bitwise reproducible from run to run for the same
container, not promised across layouts.  create_graph=True raises (second derivatives are out of scope).

REFUSALS, all before any launch, each a RuaError naming the argument: a CPU tensor; an integer payload; K > 64 or K == 0;
more than one hidden dimension, or none; a `transitions` that is not [K, K]; a `start` / `end` that is not [K]; a dtype or
device that differs from the emissions'; `tags` of another container type, raggedness or dtype in crf_score.
(Raggedness of `tags`: a P compares batch_sizes; C / L / R compare the lengths where the host knows both without a
read-back — CPU tensors, C.new / with_host_sizes containers — and otherwise only the number of sequences: crf_score does
not synchronise to refuse.)

LIMITS: one sequence is walked by ONE wave, so a single very long sequence is correct and slow (cutting it needs K x K
matrix products per block).  Out of scope: K > 64, batched or per-sequence transition matrices, extra hidden dimensions
(heads), second derivatives, a fused gold-score kernel, semi-Markov or higher-order chains, +inf scores, CTC loss.
"""
from typing import NamedTuple, Optional

import torch

from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import (P, T, Z, NAMES, cat_lay, cls_of, hidden_of, install, lay_hidden, lead_shape,
                                 require_container, rewrap)
from torchrua_amd._lib import RuaError
from torchrua_amd.reduce import segment_sum

__all__ = ['SeqPath', 'crf_partition', 'segment_crf_partition', 'crf_marginals', 'crf_decode', 'crf_score']


class SeqPath(NamedTuple):
    """What crf_decode returns: the best tags (a container of the input's type) and their score [B]."""
    tags: Z
    score: T


def crf_partition(sequence: Z, transitions: T, start: Optional[T] = None, end: Optional[T] = None) -> T:
    """log Z [B] of every sequence, float32 (float64 for float64 emissions: never rounded to bf16 / f16 — the NLL
    `logZ - score` cancels); differentiable in the emissions, `transitions`, `start` and `end`."""
    require_container(sequence, 'crf_partition')
    K = O.crf_args('crf_partition', sequence.data, hidden_of(sequence), transitions, start, end)
    lay, _ = lay_hidden(sequence)
    return O.crf_partition(sequence.data, transitions, start, end, lay, K)


def segment_crf_partition(tensor: T, transitions: T, segment_sizes: T, start: Optional[T] = None,
                          end: Optional[T] = None) -> T:
    """log Z of every run of `segment_sizes` rows of the emissions `tensor` [N, K]."""
    K = O.crf_args('segment_crf_partition', tensor, tuple(tensor.shape[1:]), transitions, start, end)
    return O.crf_partition(tensor, transitions, start, end, cat_lay(tensor, segment_sizes), K)


def crf_marginals(sequence: Z, transitions: T, start: Optional[T] = None, end: Optional[T] = None) -> Z:
    """P(tag_t = j) per token and tag, in e's container type, shape and dtype; zeros in padding rows; no graph."""
    require_container(sequence, 'crf_marginals')
    K = O.crf_args('crf_marginals', sequence.data, hidden_of(sequence), transitions, start, end)
    lay, _ = lay_hidden(sequence)
    data = sequence.data.detach().contiguous()
    logz, alpha, _, _ = O.launch_crf_forward(lay, data, transitions, start, end, K, want_alpha=True)
    ones = torch.ones(lay.B, dtype=logz.dtype, device=data.device)
    marginals, _, _, _ = O.launch_crf_backward(lay, ones, data, transitions, end, alpha, logz, K, True, False, False,
                                               False)
    return rewrap(sequence, marginals)


def crf_decode(sequence: Z, transitions: T, start: Optional[T] = None, end: Optional[T] = None) -> SeqPath:
    """SeqPath(tags, score): Viterbi with `argmax`'s tie rule (the smallest index among the maxima)."""
    require_container(sequence, 'crf_decode')
    K = O.crf_args('crf_decode', sequence.data, hidden_of(sequence), transitions, start, end)
    lay, _ = lay_hidden(sequence)
    data = sequence.data.detach()
    score, _, backptr, last = O.launch_crf_forward(lay, data, transitions, start, end, K, viterbi=True)
    tags = O.launch_crf_backtrace(lay, backptr, last, lead_shape(sequence), K)
    return SeqPath(rewrap(sequence, tags), score)


def _check_tags(sequence: Z, tags) -> None:
    cls = cls_of(sequence)
    if cls_of(tags) is not cls:
        raise RuaError(f'crf_score: `tags` is a {NAMES[cls]} like the emissions; got {type(tags).__name__}')
    if tags.data.dtype != torch.int64:
        raise RuaError(f'crf_score: `tags` has dtype {tags.data.dtype}; it must be torch.int64')
    if tuple(tags.data.shape) != lead_shape(sequence):
        raise RuaError(f'crf_score: `tags` has shape {tuple(tags.data.shape)}; the token dimensions of the emissions are '
                       f'{lead_shape(sequence)} (one tag per token)')
    if cls is P:
        same = torch.equal(tags.batch_sizes, sequence.batch_sizes)
    else:
        # the lengths themselves where the host knows both without a read-back; else only the number of sequences
        a, b = tags.token_sizes, sequence.token_sizes
        same = a is b or a.shape == b.shape
        if same and a is not b and M.host_known(a) and M.host_known(b):
            same = torch.equal(M.host_lens(a).to(torch.long), M.host_lens(b).to(torch.long))
    if not same:
        raise RuaError('crf_score: `tags` has another raggedness (sequence lengths) than the emissions')
    if tags.data.device != sequence.data.device:
        raise RuaError(f'crf_score: `tags` lives on {tags.data.device}, the emissions on {sequence.data.device}')


def crf_score(sequence: Z, tags: Z, transitions: T, start: Optional[T] = None, end: Optional[T] = None) -> T:
    """The score [B] of the path `tags` (float32 / float64): start[y_0] + sum_t x_t[y_t] + sum_t transitions[y_{t-1}, y_t]
    + end[y_{n-1}]; 0 for an empty sequence.  Differentiable in the emissions, `transitions`, `start` and `end`."""
    require_container(sequence, 'crf_score')
    O.crf_args('crf_score', sequence.data, hidden_of(sequence), transitions, start, end,
               before_device=lambda: _check_tags(sequence, tags))
    acc = torch.float64 if sequence.data.dtype == torch.float64 else torch.float32
    ec, tc = sequence.cat(), tags.cat()
    x, y, lens = ec.data, tc.data, ec.token_sizes.to(ec.data.device)
    n = int(x.size(0))
    if n == 0:
        return x.to(acc).sum() * 0 + torch.zeros(lens.numel(), dtype=acc, device=x.device)
    # the first and the last token of every sequence that has one (an empty one marks nothing)
    off = torch.cumsum(lens, 0) - lens
    live = (lens > 0).to(torch.int32)
    marks = torch.zeros(2, n, dtype=torch.int32, device=x.device)
    marks[0].index_add_(0, off.clamp(max=n - 1), live)
    marks[1].index_add_(0, (off + lens - 1).clamp(0, n - 1), live)
    first, final = marks[0] > 0, marks[1] > 0
    prev = torch.cat([y.new_zeros(1), y[:-1]])
    term = x.gather(1, y.unsqueeze(1)).squeeze(1).to(acc)
    zero = term.new_zeros(())
    head = zero if start is None else start.to(acc)[y]
    term = term + torch.where(first, head, transitions.to(acc)[prev, y])
    if end is not None:
        term = term + torch.where(final, end.to(acc)[y], zero)
    return segment_sum(term, lens)


install(crf_partition=crf_partition, crf_marginals=crf_marginals, crf_decode=crf_decode, crf_score=crf_score)
