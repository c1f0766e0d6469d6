"""Per-sequence CTC over the frames of any container (C / L / P / R) of log-probabilities and the labels of ANOTHER ragged
container — an extension: the loss the ragged speech / sequence-labelling pipeline ends in (`unique_consecutive` and
`compress` are the CTC collapse and greedy decoding, `repeat_interleave` and `window_pool` the length regulator and the
frame subsampler).  The stock spelling is `left()` on both containers, a transpose to [T, B, V] and `F.ctc_loss` — the
padded [B, T_max, V] tensor the containers exist to avoid, and nothing at all for a PackedSequence.  Here the loss, its
TRUE gradient and the forced alignment are fused HIP kernels (csrc/rua_ctc.hip), identical for all 4 x 4
pairs of layouts.

`log_probs` is a container with exactly ONE hidden dimension, the V classes: data is [N, V] for C / P and [B, T_phys, V]
for L / R; float32, float64, bfloat16 or float16; accumulation is fp32 (fp64 for float64).  `targets` is an int64
container WITHOUT hidden dimensions and with the same number of sequences; it may be any of the four types,
independently of `log_probs`.  Sequence b is the same sequence in both (a P: the original batch order).

    ctc_loss(log_probs, targets, blank=0, zero_infinity=False) -> Tensor [B]     also log_probs.ctc_loss(targets, ...)
        The negative log-likelihood of every sequence, in the batch order of `reduce_sum`, in FLOAT32 (float64 for
        float64 input) — never rounded to bf16 / f16, for the same reason as the CRF's logZ.  There is no `reduction`
        argument: torch's 'sum' is `.sum()`, torch's 'mean' is `(loss / target_lengths.clamp(min=1)).mean()` — it
        divides every loss by its TARGET length first.
    segment_ctc_loss(tensor, sizes, targets, target_sizes, blank=0, zero_infinity=False)      the `segment_*` style
    ctc_align(log_probs, targets, blank=0) -> SeqAlign(labels, positions, score)  also log_probs.ctc_align(...)
        The best alignment (the max semiring).  `labels` is an int64 container of log_probs' type and token layout that
        reuses its metadata objects: one class per frame, zeros in padding rows.  `positions`, same layout: the index
        into the sequence's own target for a non-blank frame, -1 for a blank frame (durations are `unique_consecutive` /
        `seg` away).  `score` [B] is the best path's log-probability.  Nothing is differentiable.

SEMANTICS.  The extended target is l' = (blank, y_0, blank, ..., blank), S' = 2 S + 1 states.  ONE evaluation order per
(sequence, frame, state), whatever the layouts, the bucket or the kernel form: v0 = alpha[s], v1 = alpha[s-1],
v2 = alpha[s-2] (only if l'_s != blank and l'_s != l'_{s-2}); terms that do not exist are absent; m = max; m == -inf gives
-inf; otherwise lp_t[l'_s] + (m + log(exp(v0-m) + exp(v1-m) [+ exp(v2-m)])).  alpha_0[0] = lp_0[blank],
alpha_0[1] = lp_0[y_0]; logZ folds alpha_{T-1}[S'-1] and then alpha_{T-1}[S'-2]; the loss is -logZ.
T = 0 and S = 0 give 0; S = 0 gives -sum_t lp_t[blank]; a target with no valid alignment (T < S + repeats, or every path
through -inf) gives +inf, or 0 under zero_infinity, and exact zero gradients in both cases (the CRF's documented choice).
-inf log-probabilities are first-class and never give NaN; a NaN stays in its own sequence.  A label equal to `blank`
is an ordinary class under the rule above.  A label outside [0, V) is never dereferenced: that sequence's loss is NaN,
its gradient zeros, its alignment all `blank` with score NaN.

GRADIENT — the TRUE one: grad[t, c] = -g[b] * sum_{s : l'_s = c} exp((alpha_t[s] + beta_t[s]) - logZ[b]), beta without the
emission at t, each value rounded once; exact zeros in padding rows.  This DEVIATES from `F.ctc_loss`, whose `grad` is
exp(lp) - posterior: that is not the gradient of its own value and is only right directly behind a class log_softmax.
Both coincide behind `data.log_softmax(-1)` (torch's, over the V classes); the library's own `z.log_softmax()` is over
TIME, not over classes.  No float atomics: the sum over the states of a class has one fixed order, so the
gradient is bitwise reproducible from run to run and identical for all 4 x 4 pairs of layouts and for every state
bucket.  create_graph=True raises.

ALIGNMENT TIES follow `argmax`: among the maxima the smallest predecessor state wins, at the end the smaller of S'-2 and
S'-1; a NaN beats every number and the first NaN wins.  No alignment: all-`blank` labels, -1 positions, score -inf.
T = 0: no tokens, score 0 (-inf if S > 0).

TARGET LENGTHS.  The state bucket goes by the longest target of the batch, so the host must know the target lengths:
with host lengths (C.new, with_host_sizes, a P, an earlier read-back) nothing is read back; otherwise there is ONE
blocking copy of [B] int64, attached to the container.  The longest target allowed is 1 023 labels (S' <= 2 047).  The
frame lengths are not needed on the host (an R sized by device-only lengths is described as every operator describes it).

REFUSALS, all before any launch, each a RuaError naming the argument: a CPU tensor; an integer `log_probs`; no hidden
dimension, or more than one; `targets` that is not int64 or has hidden dimensions; another number of sequences or
another device; `blank` outside [0, V); a target that is too long.

LIMITS: one long target sends the whole batch to the workgroup form; one wave (one workgroup) walks all the frames of a
sequence; the saved table costs N x (2 S_max + 1) accumulators.
"""
from typing import NamedTuple

import torch

from torchrua_amd import _meta as M
from torchrua_amd import _ops as O
from torchrua_amd.layout import (P, T, Z, cat_lay, cls_of, hidden_of, install, lay_hidden, lead_shape, lens_of, n_seq,
                                 require_container, rewrap)
from torchrua_amd._lib import RuaError

__all__ = ['SeqAlign', 'ctc_loss', 'segment_ctc_loss', 'ctc_align']


class SeqAlign(NamedTuple):
    """What ctc_align returns: the class and the target position of every frame (containers of the input's type) and the
    best path's log-probability [B]."""
    labels: Z
    positions: Z
    score: T


def _known_bound(targets: Z):
    """The longest target if the host can tell without a device (None: it cannot)."""
    if isinstance(targets, P):
        return int(targets.batch_sizes.numel())
    return M.known_max_len(targets.token_sizes) if targets.token_sizes.numel() else 0


def _plan(what: str, log_probs: Z, targets: Z, blank) -> O.CtcPlan:
    require_container(log_probs, what)
    if cls_of(targets) is None:
        raise RuaError(f'{what}: `targets` is a container (C / L / P / R) of int64 labels; got {type(targets).__name__}')
    known = _known_bound(targets)
    V = O.ctc_args(what, log_probs.data, hidden_of(log_probs), n_seq(log_probs), targets.data, hidden_of(targets),
                   n_seq(targets), blank,
                   before_device=None if known is None else (lambda: O.ctc_target_bound(what, known)))
    s_max = known if known is not None else O.ctc_target_bound(what, M.max_len(lens_of(targets)))
    return O.CtcPlan(lay_hidden(log_probs)[0], lay_hidden(targets)[0], V, s_max, blank)


def ctc_loss(log_probs: Z, targets: Z, blank: int = 0, zero_infinity: bool = False) -> T:
    """The negative log-likelihood [B] of every sequence, float32 (float64 for float64 input: never rounded to bf16 /
    f16); differentiable in the log-probabilities, with the TRUE gradient -posterior (F.ctc_loss returns
    exp(lp) - posterior; both coincide behind `data.log_softmax(-1)`).  No `reduction`: torch's 'mean' is
    `(loss / target_lengths.clamp(min=1)).mean()`."""
    plan = _plan('ctc_loss', log_probs, targets, blank)
    return O.ctc_loss(log_probs.data, targets.data, plan, zero_infinity)


def segment_ctc_loss(tensor: T, segment_sizes: T, targets: T, target_sizes: T, blank: int = 0,
                     zero_infinity: bool = False) -> T:
    """The loss of every run of `segment_sizes` rows of `tensor` [N, V] against the run of `target_sizes` labels of
    `targets` [M]."""
    what = 'segment_ctc_loss'
    for name, t in (('tensor', tensor), ('segment_sizes', segment_sizes), ('targets', targets),
                    ('target_sizes', target_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuaError(f'{what}: `{name}` is a tensor; got {type(t).__name__}')
    known = M.known_max_len(target_sizes) if target_sizes.numel() else 0
    V = O.ctc_args(what, tensor, tuple(tensor.shape[1:]), int(segment_sizes.numel()), targets, tuple(targets.shape[1:]),
                   int(target_sizes.numel()), blank,
                   before_device=None if known is None else (lambda: O.ctc_target_bound(what, known)))
    s_max = known if known is not None else O.ctc_target_bound(what, M.max_len(target_sizes))
    plan = O.CtcPlan(cat_lay(tensor, segment_sizes), cat_lay(targets, target_sizes), V, s_max, blank)
    return O.ctc_loss(tensor, targets, plan, zero_infinity)


def ctc_align(log_probs: Z, targets: Z, blank: int = 0) -> SeqAlign:
    """SeqAlign(labels, positions, score): the best alignment, with `argmax`'s tie rule."""
    plan = _plan('ctc_align', log_probs, targets, blank)
    data = log_probs.data.detach()
    score, _, _, codes, last = O.launch_ctc_forward(plan, data, targets.data, viterbi=True)
    labels, positions = O.launch_ctc_backtrace(plan, targets.data, codes, last, lead_shape(log_probs))
    return SeqAlign(rewrap(log_probs, labels), rewrap(log_probs, positions), score)


install(ctc_loss=ctc_loss, ctc_align=ctc_align)
