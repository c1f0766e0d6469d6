"""Per-sequence sliding-window pooling: the float64 yardstick and the bounds shared by tests/test_window_surface.py and
tests/test_gpu_window.py.

The reference library has no such operator.  The yardstick is the definition, as a plain loop on the CPU: for every
sequence on its own and every window u < n_out(n), the tokens seq[u*S : min(u*S + K, n)] in float64, with

    n <= 0: 0;   floor: (n - K) // S + 1 if n >= K else 0;   ceil: m = ceil(max(n - K, 0) / S) + 1, m - 1 if (m - 1) S >= n

`max` yields the winner by the total order on (value, position) — a NaN beats every number, the first NaN or the first
maximal position wins, -0.0 == +0.0 — as an offset into the window (`arg`) and as the winner's BITS in the payload's own
dtype; the spread is the stated adjoint.  For bf16 / f16 the wanted value is computed from the ROUNDED inputs the kernel
actually receives.

The bounds are derived the way tests/conv_util.py derives its own; none comes from what the kernels give.  u = 2^-24 is
the rounding of the fp32 accumulator (2^-53 for float64 payloads), r |y| half a unit in the last place of the output
dtype at the wanted value (conv_util.half_ulp):

    sum:            |err| <= cnt u sum |x_i| + r |y|           cnt - 1 additions of partial sums bounded by sum |x_i|
    mean:           |err| <= (cnt + 1) u sum |x_i| / cnt + r |y|       ... and one division
    max, take:      bits
    spread, token t in the windows W(t):
      sum:          |err| <= |W| u sum_W |g_u| + r |grad|
      mean:         |err| <= (|W| + 1) u sum_W |g_u| / cnt_u + r |grad|        every term is divided (one rounding) first
      max / take:   |err| <= |W| u sum_{W, arg_u = t - uS} |g_u| + r |grad|
    a token in no window, and every padding row: exactly 0 (the bound is 0: conv_util.ratio then demands equality).
Integer payloads are exact.
"""
import numpy as np
import torch

from conv_util import acc_u, half_ulp

F32, BF16, F16, F64, I64 = torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int64
KS = [(1, 1), (2, 2), (3, 1), (3, 2), (2, 5), (1, 3), (64, 64), (64, 1), (7, 2 ** 31 - 1)]
MODES = ('max', 'mean', 'sum')


def n_out(n: int, K: int, S: int, ceil_mode: bool) -> int:
    if n <= 0:
        return 0
    if not ceil_mode:
        return (n - K) // S + 1 if n >= K else 0
    m = -(-max(n - K, 0) // S) + 1
    return m - 1 if (m - 1) * S >= n else m


def out_lens(lens, K: int, S: int, ceil_mode: bool) -> torch.Tensor:
    return torch.tensor([n_out(int(n), K, S, ceil_mode) for n in lens], dtype=torch.long)


def _winner(win: torch.Tensor) -> torch.Tensor:
    """argmax over dim 0 by (value, position): the first NaN, else the first maximum.  win: [cnt, H]."""
    nan = torch.isnan(win) if win.is_floating_point() else torch.zeros_like(win, dtype=torch.bool)
    first_nan = torch.argmax(nan.to(torch.uint8), dim=0)
    safe = torch.where(nan, torch.full_like(win, float('-inf')), win) if win.is_floating_point() else win
    return torch.where(nan.any(0), first_nan, torch.argmax(safe, dim=0))


class Pooled:
    """What the yardstick gives for one (payload, lengths, K, S, mode, ceil_mode): `want` (float64, or int64 for an int64
    payload; [N', H]), `bits` (max: the winners in the payload's dtype), `arg` ([N', H] int64), `lens` (new lengths),
    `bound` ([N', H] float64) and, for the spread, `windows`: (row of the pooled side, first row, last row + 1 of the big
    side in cat form) per window."""


def pool64(x: torch.Tensor, lens, K: int, S: int, mode: str, ceil_mode: bool) -> Pooled:
    N = x.shape[0]
    H = int(np.prod(x.shape[1:], dtype=np.int64))
    x2 = x.reshape(N, H)
    exact = not x.is_floating_point()
    xd = x2 if exact else x2.double()
    rows, bits, args, bounds, windows = [], [], [], [], []
    off = 0
    u_acc = acc_u(x.dtype)
    for n in [int(v) for v in lens]:
        for u in range(n_out(n, K, S, ceil_mode)):
            a, e = off + u * S, off + min(u * S + K, n)
            win = xd[a:e]
            cnt = e - a
            windows.append((len(rows), a, e))
            if mode == 'max':
                w = _winner(win)
                args.append(w)
                rows.append(win.gather(0, w[None])[0])
                bits.append(x2[a:e].gather(0, w[None])[0])
                bounds.append(torch.zeros(H, dtype=F64))
            else:
                s = win.sum(0)
                rows.append(s if mode == 'sum' or exact else s / cnt)
                scale = win.abs().sum(0).double()
                bounds.append(cnt * u_acc * scale if mode == 'sum' else (cnt + 1) * u_acc * scale / cnt)
                args.append(torch.zeros(H, dtype=torch.long))
        off += n
    p = Pooled()
    hidden = tuple(x.shape[1:])
    stack = lambda seq, dtype: (torch.stack(seq) if seq else torch.zeros((0, H), dtype=dtype)).reshape((-1,) + hidden)
    p.want = stack(rows, xd.dtype)
    p.bits = stack(bits, x.dtype) if mode == 'max' else None
    p.arg = stack(args, torch.long)
    p.lens = out_lens(lens, K, S, ceil_mode)
    p.bound = stack(bounds, F64)
    if not exact and mode != 'max':
        p.bound = p.bound + half_ulp(torch.nan_to_num(p.want, nan=0.0, posinf=0.0, neginf=0.0), x.dtype)
    p.windows, p.mode, p.n_rows, p.hidden, p.dtype = windows, mode, N, hidden, x.dtype
    return p


def spread64(p: Pooled, g: torch.Tensor):
    """(grad [N, *hidden] float64, bound) of the cotangent g [N', *hidden] by the stated rule."""
    H = int(np.prod(p.hidden, dtype=np.int64))
    g2 = g.double().reshape(g.shape[0], H)
    grad, scale, count = torch.zeros((p.n_rows, H), dtype=F64), torch.zeros((p.n_rows, H), dtype=F64), torch.zeros(p.n_rows, dtype=F64)
    arg = p.arg.reshape(-1, H)
    for row, a, e in p.windows:
        cnt = e - a
        count[a:e] += 1
        if p.mode == 'max':
            hit = torch.arange(cnt)[:, None] == arg[row][None]
            grad[a:e] += torch.where(hit, g2[row][None], torch.zeros((), dtype=F64))
            scale[a:e] += torch.where(hit, g2[row].abs()[None], torch.zeros((), dtype=F64))
        else:
            term = g2[row] if p.mode == 'sum' else g2[row] / cnt
            grad[a:e] += term[None]
            scale[a:e] += term.abs()[None]
    extra = 1 if p.mode == 'mean' else 0
    bound = (count + extra)[:, None] * acc_u(p.dtype) * scale
    bound = torch.where(count[:, None] > 0, bound + half_ulp(grad, p.dtype), torch.zeros((), dtype=F64))
    shape = (p.n_rows,) + p.hidden
    return grad.reshape(shape), bound.reshape(shape)


def ratio_nan(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor) -> float:
    """conv_util.ratio for payloads that may hold NaN / inf: those must sit at the same places (inf with its sign);
    everywhere else the worst error over its bound, exact where the bound is 0."""
    if got.numel() == 0:
        return 0.0
    got = got.detach().cpu().double().reshape(want64.shape)
    want64 = want64.double()
    special = ~torch.isfinite(want64)
    if not torch.equal(torch.isnan(got), torch.isnan(want64)):
        return float('inf')
    inf = special & ~torch.isnan(want64)
    if not torch.equal(got[inf], want64[inf]):
        return float('inf')
    err = torch.where(special, torch.zeros((), dtype=F64), (got - want64).abs())
    bound = torch.where(torch.isfinite(bound), bound, torch.zeros((), dtype=F64))
    if bool(((bound == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / bound.clamp_min(1e-300)).max())


def draw(shape, dtype, seed: int) -> torch.Tensor:
    """randn rounded to `dtype` (CPU); int64: values whose window sums wrap."""
    g = torch.Generator().manual_seed(seed)
    if dtype == I64:
        return torch.randint(-2 ** 62, 2 ** 62, tuple(shape), generator=g)
    return torch.randn(tuple(shape), generator=g, dtype=F64 if dtype == F64 else F32).to(dtype)


def host_formula(n: np.ndarray, K: int, S: int, ceil_mode: bool) -> np.ndarray:
    from torchrua_amd.window import window_out_lens
    return window_out_lens(n, K, S, ceil_mode)
