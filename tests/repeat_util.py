"""The yardstick of `repeat_interleave` in plain torch on the CPU: split a batch into its sequences, stock
`torch.repeat_interleave(seq, counts, dim=0)` each, rebuild.  Nothing here touches the library;
tests/test_repeat_surface.py checks it against a Python loop over the tokens.  Floats are compared through an integer
view (`bits` of tests/compress_util.py), so NaN payloads compare."""
import torch

from compress_util import bits, cat, padded, same_bits, split  # noqa: F401  (re-exported for the tests)


def repeat(seqs, counts):
    """The definition: every sequence repeats token t counts[t] times, in order."""
    return [torch.repeat_interleave(s, c, dim=0) for s, c in zip(seqs, counts)]


def repeat_by_loop(seqs, counts):
    """The same, copy by copy."""
    out = []
    for s, c in zip(seqs, counts):
        rows = [s[t] for t in range(s.shape[0]) for _ in range(int(c[t]))]
        out.append(torch.stack(rows) if rows else s[:0])
    return out


def repeat_cat(data, counts, lens):
    """The yardstick in cat form: (data', lengths') of C(data, lens).repeat_interleave(counts)."""
    return cat(repeat(split(data, lens), split(counts, lens)), data)


def repeat_grad_cat(counts, w, lens, like, dtype=torch.float64):
    """The gradient of (repeat_interleave(z).data * w).sum() w.r.t. the cat-form payload, accumulated in `dtype` on the
    CPU: autograd through the yardstick (the backward of repeat_interleave adds the cotangents of a token's copies)."""
    leaf = torch.zeros_like(like, dtype=dtype).requires_grad_(True)
    out, _ = repeat_cat(leaf, counts, lens)
    (out * w.to(dtype)).sum().backward()
    return leaf.grad
