"""The yardstick of `compress` in plain torch on the CPU: split a batch into its sequences, `seq[m]` each, rebuild.
Nothing here touches the library; tests/test_compress_surface.py checks it against a Python loop over the tokens.
Floats are compared through an integer view (`bits`), so NaN payloads compare."""
import torch

INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """`t` as integers of its element size (bool as uint8): equality of these is equality of the bits."""
    t = t.detach().cpu().contiguous()
    return t.view(INT_VIEW[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def split(data, lens):
    """The sequences of a cat-form payload [N, *hidden] (or mask [N]) with lengths `lens`."""
    return list(torch.split(data, [int(n) for n in lens]))


def keep(seqs, masks):
    """The definition: every sequence keeps the tokens where its mask is true, in order."""
    return [s[m] for s, m in zip(seqs, masks)]


def keep_by_loop(seqs, masks):
    """The same, token by token."""
    out = []
    for s, m in zip(seqs, masks):
        rows = [s[t] for t in range(s.shape[0]) if bool(m[t])]
        out.append(torch.stack(rows) if rows else s[:0])
    return out


def cat(seqs, like):
    """(data [N', *hidden], lengths int64) of a list of sequences; `like` gives dtype and hidden shape when empty."""
    lens = torch.tensor([s.shape[0] for s in seqs], dtype=torch.long)
    data = torch.cat(seqs) if seqs else like[:0]
    return data, lens


def compress_cat(data, mask, lens):
    """The yardstick in cat form: (data', lengths') of C(data, lens).compress(mask)."""
    return cat(keep(split(data, lens), split(mask, lens)), data)


def padded(seqs, like, right=False, T=None):
    """[B, T, *hidden] with zero padding; T defaults to the longest sequence (what C.left() / C.right() give)."""
    longest = max([s.shape[0] for s in seqs], default=0)
    T = longest if T is None else T
    out = torch.zeros((len(seqs), T) + tuple(like.shape[1:]), dtype=like.dtype)
    for b, s in enumerate(seqs):
        n = s.shape[0]
        if right:
            out[b, longest - n:longest] = s
        else:
            out[b, :n] = s
    return out


def compress_grad_cat(mask, w_kept, lens, like):
    """The gradient of (compress(z).data * w).sum() w.r.t. the cat-form payload: w at the kept tokens in their order,
    exact zeros elsewhere — autograd through the yardstick (indexing moves values, so it is exact in any dtype)."""
    leaf = torch.zeros_like(like, dtype=torch.float64).requires_grad_(True)
    out, _ = compress_cat(leaf, mask, lens)
    (out * w_kept.to(torch.float64)).sum().backward()
    return leaf.grad.to(like.dtype)
