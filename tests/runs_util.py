"""The yardstick of `unique_consecutive` in plain torch on the CPU: split a batch into its sequences,
`torch.unique_consecutive(seq, dim=0, return_inverse=True, return_counts=True)` each, rebuild.  Nothing here touches the
library; tests/test_unique_surface.py checks it against a written-out loop.  Floats are compared through an integer
view (`same_bits` of tests/compress_util.py), so NaN payloads and the sign of a zero compare."""
import torch

from compress_util import cat, padded, same_bits, split  # noqa: F401  (re-exported for the tests)


def runs(seq):
    """(values, inverse, counts) of one sequence [n, *hidden]: stock torch, the definition."""
    if seq.shape[0] == 0:
        return seq[:0], torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    return torch.unique_consecutive(seq, dim=0, return_inverse=True, return_counts=True)


def runs_by_loop(seq):
    """The same, written out: a token starts a run when it is the first or any element differs (`==` of the dtype) from
    its predecessor's; the values are the run's FIRST token."""
    n = seq.shape[0]
    if n == 0:
        return seq[:0], torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    width = max(seq[0].numel(), 1)
    same = (seq[1:] == seq[:-1]).reshape(n - 1, width).all(dim=1)
    head = torch.cat([torch.ones(1, dtype=torch.bool), ~same])
    inverse = torch.cumsum(head.long(), 0) - 1
    starts = head.nonzero().reshape(-1)
    counts = torch.diff(torch.cat([starts, torch.tensor([n])]))
    return seq[starts], inverse, counts


def runs_cat(data, lens, fn=runs):
    """The yardstick in cat form: (values [N', *hidden], new lengths int64 [B], inverse [N], counts [N'], per-sequence
    lists of the three) of C(data, lens).unique_consecutive(True, True)."""
    parts = [fn(s) for s in split(data, lens)]
    values, new_lens = cat([p[0] for p in parts], data)
    inverse = torch.cat([p[1] for p in parts]) if parts else torch.zeros(0, dtype=torch.long)
    counts = torch.cat([p[2] for p in parts]) if parts else torch.zeros(0, dtype=torch.long)
    return values, new_lens, inverse, counts, parts


def runs_padded(data, lens, right=False):
    """The padded form for L / R: (values [B, T', *hidden], inverse [B, T], counts [B, T']) with zero padding; T the
    longest old sequence, T' the longest new one."""
    parts = runs_cat(data, lens)[4]
    like_i = torch.zeros(0, dtype=torch.long)
    return (padded([p[0] for p in parts], data, right=right), padded([p[1] for p in parts], like_i, right=right),
            padded([p[2] for p in parts], like_i, right=right))
