"""The yardstick of `join` / `unjoin` in plain torch on the CPU: split every part into its sequences, `torch.cat` per
sequence, rebuild cat or padded storage.  Nothing here touches the library; tests/test_join_surface.py checks it against
a Python loop over the tokens.  Floats are compared through an integer view (`bits`), so NaN payloads compare."""
import torch

INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def bits(t):
    """`t` as integers of its element size (bool as uint8): equality of these is equality of the bits."""
    t = t.detach().cpu().contiguous()
    return t.view(INT_VIEW[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def split(data, lens):
    """The sequences of a cat-form payload [N, *hidden] with lengths `lens`."""
    return list(torch.split(data, [int(n) for n in lens]))


def as_seqs(part, lens=None):
    """A part as its list of sequences: (data, lens) in cat form, or a tensor [B, *hidden] — one token per sequence."""
    if lens is None:
        return [row[None] for row in part]
    return split(part, lens)


def join_seqs(parts):
    """The definition: sequence b of the result is sequence b of every part in list order.  `parts` is a list of lists
    of sequences."""
    return [torch.cat([p[b] for p in parts]) for b in range(len(parts[0]))]


def join_by_loop(parts):
    """The same, token by token."""
    out = []
    for b in range(len(parts[0])):
        rows = [p[b][t] for p in parts for t in range(p[b].shape[0])]
        out.append(torch.stack(rows) if rows else parts[0][b][:0])
    return out


def unjoin_seqs(seqs, sizes):
    """The inverse: part j holds the tokens [pre_j, pre_j + s_j) of every sequence, clamped to its end; `sizes` is a
    list of per-sequence lists (or ints).  Returns a list of lists of sequences."""
    out = [[] for _ in sizes]
    for b, s in enumerate(seqs):
        pre = 0
        for j, size in enumerate(sizes):
            n = int(size if isinstance(size, int) else size[b])
            n = max(0, min(n, s.shape[0] - pre))
            out[j].append(s[pre:pre + n])
            pre += n
    return out


def cat(seqs, like):
    """(data [N, *hidden], lengths int64) of a list of sequences; `like` gives dtype and hidden shape when empty."""
    lens = torch.tensor([s.shape[0] for s in seqs], dtype=torch.long)
    data = torch.cat(seqs) if seqs else like[:0]
    return data, lens


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
