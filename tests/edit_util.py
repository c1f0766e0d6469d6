"""The yardstick of the edit-distance operators (torchrua_amd/edit.py): the plain triple-loop Python DP with the documented
backtrace rule, a numpy row-wise version of the same for the larger cases, and the input generators of the tests.

    D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j-1] + (hyp[i-1] != ref[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)

The backtrace starts at (T, S) and takes the diagonal if it attains D[i][j], else up (an insertion: hyp token i - 1 has no
partner, position -1), else left (a deletion); at i == 0 only left exists, at j == 0 only up.  Everything is integer: the
GPU tests compare with torch.equal.
"""
from typing import List, NamedTuple, Sequence

import numpy as np
import torch

I64 = torch.int64


class Edit(NamedTuple):
    positions: List[int]      # per hyp token: the ref index it is paired with, -1 for an insertion
    distance: int
    substitutions: int
    insertions: int
    deletions: int


def _backtrace(D, hyp, ref) -> Edit:
    """The documented walk over a full table D[T + 1][S + 1] (lists or an array)."""
    i, j = len(hyp), len(ref)
    pos = [-1] * i
    sub = ins = dele = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]) == D[i][j]:
            pos[i - 1] = j - 1
            sub += int(hyp[i - 1] != ref[j - 1])
            i, j = i - 1, j - 1
        elif i > 0 and (j == 0 or D[i - 1][j] + 1 == D[i][j]):
            ins += 1
            i -= 1
        else:
            dele += 1
            j -= 1
    return Edit(pos, int(D[len(hyp)][len(ref)]), sub, ins, dele)


def table_loop(hyp: Sequence[int], ref: Sequence[int]) -> List[List[int]]:
    """The plain DP, cell by cell."""
    T, S = len(hyp), len(ref)
    D = [[0] * (S + 1) for _ in range(T + 1)]
    for j in range(S + 1):
        D[0][j] = j
    for i in range(1, T + 1):
        D[i][0] = i
        for j in range(1, S + 1):
            D[i][j] = min(D[i - 1][j - 1] + (hyp[i - 1] != ref[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    return D


def edit_loop(hyp: Sequence[int], ref: Sequence[int]) -> Edit:
    """THE yardstick: the triple loop and the documented backtrace."""
    hyp, ref = [int(v) for v in hyp], [int(v) for v in ref]
    return _backtrace(table_loop(hyp, ref), hyp, ref)


def table_numpy(hyp: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """The same table, a row at a time: D[i][j] = min(t[j], D[i][j-1] + 1) unrolled is j + the running minimum of
    t[k] - k (checked against the triple loop in tests/test_edit_surface.py)."""
    T, S = len(hyp), len(ref)
    D = np.empty((T + 1, S + 1), dtype=np.int64)
    cols = np.arange(S + 1, dtype=np.int64)
    D[0] = cols
    t = np.empty(S + 1, dtype=np.int64)
    for i in range(1, T + 1):
        prev = D[i - 1]
        t[0] = i
        np.minimum(prev[:-1] + (ref != hyp[i - 1]), prev[1:] + 1, out=t[1:])
        D[i] = np.minimum.accumulate(t - cols) + cols
    return D


def edit_numpy(hyp, ref) -> Edit:
    hyp, ref = np.asarray(hyp, dtype=np.int64).reshape(-1), np.asarray(ref, dtype=np.int64).reshape(-1)
    return _backtrace(table_numpy(hyp, ref), hyp, ref)


def alignment_cost(e: Edit, hyp: Sequence[int], ref: Sequence[int]) -> int:
    """The cost of the alignment `positions` describes, recounted from the tokens alone."""
    named = [p for p in e.positions if p >= 0]
    subs = sum(int(hyp[t] != ref[p]) for t, p in enumerate(e.positions) if p >= 0)
    return subs + (len(hyp) - len(named)) + (len(ref) - len(named))


# ------------------------------------------------------------------ batches
class Want(NamedTuple):
    positions: torch.Tensor   # cat form
    distance: torch.Tensor
    substitutions: torch.Tensor
    insertions: torch.Tensor
    deletions: torch.Tensor


def want_of(hyps: Sequence[torch.Tensor], refs: Sequence[torch.Tensor]) -> Want:
    es = [edit_numpy(h.numpy(), r.numpy()) for h, r in zip(hyps, refs)]
    pos = [torch.tensor(e.positions, dtype=I64) for e in es]
    return Want(torch.cat(pos) if pos else torch.zeros(0, dtype=I64),
                *(torch.tensor([getattr(e, f) for e in es], dtype=I64)
                  for f in ('distance', 'substitutions', 'insertions', 'deletions')))


def lens_of(seqs: Sequence[torch.Tensor]) -> torch.Tensor:
    return torch.tensor([int(s.numel()) for s in seqs], dtype=I64)


def cat_of(seqs: Sequence[torch.Tensor]) -> torch.Tensor:
    return torch.cat(list(seqs)) if len(seqs) else torch.zeros(0, dtype=I64)


def draw(n: int, alphabet: int, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, alphabet, (n,), generator=gen, dtype=I64)


def noisy(ref: torch.Tensor, n: int, alphabet: int, seed: int) -> torch.Tensor:
    """A hyp of n tokens that resembles `ref`: a resampling of it with some tokens redrawn (n == 0: empty)."""
    if n == 0 or ref.numel() == 0:
        return draw(n, alphabet, seed)
    gen = torch.Generator().manual_seed(seed)
    idx = torch.sort(torch.randint(0, ref.numel(), (n,), generator=gen))[0]
    out = ref[idx].clone()
    flip = torch.rand(n, generator=gen) < 0.3
    out[flip] = torch.randint(0, alphabet, (int(flip.sum()),), generator=gen, dtype=I64)
    return out


HYP_LENS = (0, 1, 2, 63, 64, 65, 150)          # both sides of the 64-token fetch


def edge_case(s_max: int, alphabet: int = 5):
    """(hyps, refs): 7 pairs, the last ref of exactly s_max tokens and the rest shorter (as far as s_max leaves room);
    hyp lengths HYP_LENS."""
    ref_lens = [s_max // 2, min(3, s_max), s_max // 3, max(s_max - 1, 0), 0, min(70, s_max), s_max]     # the longest hyp: s_max
    refs = [draw(n, alphabet, 1000 + 7 * s_max + k) for k, n in enumerate(ref_lens)]
    hyps = [noisy(r, n, alphabet, 2000 + 7 * s_max + k) for k, (r, n) in enumerate(zip(refs, HYP_LENS))]
    return hyps, refs


def bucket(s_max: int) -> str:
    return 'R1' if s_max <= 64 else 'R2' if s_max <= 128 else 'R4' if s_max <= 256 else 'R8' if s_max <= 512 else 'WG'
