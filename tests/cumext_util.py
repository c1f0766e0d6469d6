"""Yardsticks and bounds of the cummax / cummin / logcumsumexp tests (tests/test_cumext_surface.py on the CPU,
tests/test_gpu_cumext.py on the GPU).

Yardsticks: stock torch on the CPU, per sequence via torch.split —
  torch.cummax / torch.cummin in the payload's own dtype: exact (bf16 / f16 comparisons do not round), both outputs;
  torch.logcumsumexp in float64.

The bound of logcumsumexp is DERIVED from the fold order (csrc/rua_cumext.hip: groups of 8 by three doubling steps,
tiles of 4 groups, blocks of 64 tiles, block bases in block order), not from what the kernels give.  With u the unit
roundoff of the accumulator (2^-24; 2^-53 for float64), a token at scan position p has passed through at most
    n(p) = 3 (doubling steps) + 3 (groups of its tile) + (p % 2048) // 32 (tile carries, up to 63) + p // 2048 (blocks) + 2
combines (the last two: base with carry, and the prefix with the token's own group).  Every combine forms
s = s_a * exp(m_a - M) + s_b * exp(m_b - M) where one factor is exactly 1: one exp (1 ulp = 2u), one product (u) and
one sum (u) of positive terms, so the relative error of s grows by at most 4u per combine.  y = m + log s adds the
error of the log (1 ulp of |log s| <= log(p + 1)) and of the last sum (u |y|):
    |y - want| <= 4u n(p) + 2u log(p + 1) + u |y|        (+ half an ulp of the output dtype for bf16 / f16)
The float64 yardstick is a sequential log-add-exp (max + log1p(exp(min - max)) per step): after p steps it is itself off
by up to (p + 1) * 2^-53 * (3 + |y|) (an exp, a log1p of at most log 2 and a sum per step), which is added to the bound —
invisible next to an fp32 accumulator, the larger part for a float64 payload.
`lse_bound` returns it together with the project's float bar 1e-5 * (1 + |y|); callers assert bound <= bar on their own
inputs (fp32 / fp64) and hold the kernels to the BOUND.

The gradient's yardstick is its definition, grad_in[s] = sum_{t >= s} g_t exp(x_s - y_t) (0 where x_s = -inf), in
float64 on the forward's own output y, and the bar is 1e-5 * sum_{t >= s} |g_t| exp(x_s - y_t)."""
import math

import torch

BAR = 1e-5
BF16, F16, F32, F64, I64 = torch.bfloat16, torch.float16, torch.float32, torch.float64, torch.int64
REPORT = {}


def note(key, ratio):
    """Keep and print the worst achieved / bound ratio of `key` (the lines of profiles/cumext_report.txt)."""
    REPORT[key] = max(REPORT.get(key, 0.0), float(ratio))
    print(f'cumext report: {key} worst achieved/bound = {REPORT[key]:.4f}')


def pieces(v, lens):
    return torch.split(v, lens.tolist(), dim=0)


def seg_cumextreme(v, lens, largest, reverse):
    """(values, indices) of torch.cummax / torch.cummin per sequence of the cat-form CPU payload `v`, in its own dtype;
    `reverse`: the scan of the mirrored sequence, reported in un-mirrored positions."""
    fn = torch.cummax if largest else torch.cummin
    vals, idxs = [], []
    for p in pieces(v, lens):
        if p.size(0) == 0:
            continue
        if reverse:
            a, i = fn(p.flip(0), dim=0)
            a, i = a.flip(0), p.size(0) - 1 - i.flip(0)
        else:
            a, i = fn(p, dim=0)
        vals.append(a)
        idxs.append(i)
    if not vals:
        return v.clone(), torch.zeros(v.shape, dtype=I64)
    return torch.cat(vals), torch.cat(idxs)


def seg_run_sum(g, idx, lens, reverse):
    """The adjoint of the gather by `idx` per sequence, in the dtype of `g` (float64 for a yardstick): index_add."""
    out = []
    for gp, ip in zip(pieces(g, lens), pieces(idx, lens)):
        out.append(torch.zeros_like(gp).scatter_add_(0, ip, gp))
    return torch.cat(out) if out else g.clone()


def seg_lse64(v, lens, reverse):
    """torch.logcumsumexp per sequence in float64."""
    out = []
    for p in pieces(v.double(), lens):
        out.append(torch.logcumsumexp(p.flip(0), 0).flip(0) if reverse else torch.logcumsumexp(p, 0))
    return torch.cat(out) if out else v.double()


def scan_position(lens, reverse):
    """The position along the scan of every token of a cat-form payload."""
    out = []
    for n in lens.tolist():
        p = torch.arange(n, dtype=torch.int64)
        out.append(p.flip(0) if reverse else p)
    return torch.cat(out) if out else torch.zeros(0, dtype=I64)


def chain(p):
    """n(p) of the module docstring."""
    return 3 + 3 + (p % 2048) // 32 + p // 2048 + 2


def ulp_at(v64, dtype):
    """One unit in the last place of `dtype` (bf16 / f16) at the float64 values `v64`."""
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)
    _, e = torch.frexp(v64.abs().clamp_min(2.0 ** -140))
    return torch.ldexp(torch.ones_like(v64), (e - 1 - bits).clamp_min(lowest))


def lse_bound(want64, lens, reverse, dtype):
    """(bound, bar) per element of the cat-form float64 result `want64`; see the module docstring."""
    u = 2.0 ** -53 if dtype == F64 else 2.0 ** -24
    p = scan_position(lens, reverse).double()
    p = p.reshape(p.shape + (1,) * (want64.dim() - 1))
    w = torch.where(torch.isfinite(want64), want64, torch.zeros_like(want64)).abs()
    bound = 4 * u * chain(p.long()).double() + 2 * u * torch.log(p + 1) + u * w
    bound = bound + (p + 1) * 2.0 ** -53 * (3 + w)                 # the yardstick's own error
    bound = bound.expand_as(want64).clone()
    if dtype in (BF16, F16):
        bound = bound + 0.5 * ulp_at(want64, dtype)
    return bound, BAR * (1 + w)


def check_lse(got, x, lens, reverse, what, key, bar_holds=True):
    """`got` (cat form, any device) against float64 torch.logcumsumexp of `x`, at the derived bound.  Non-finite wanted
    values must be matched exactly."""
    got, x, lens = got.cpu(), x.cpu(), lens.cpu()
    want = seg_lse64(x, lens, reverse)
    assert got.shape == want.shape and got.dtype == x.dtype, what
    if got.numel() == 0:
        return
    bound, bar = lse_bound(want, lens, reverse, x.dtype)
    if x.dtype in (F32, F64) and bar_holds:
        assert bool((bound <= bar).all()), f'{what}: the derived bound exceeds the float bar 1e-5 * (1 + |y|)'
    fin = torch.isfinite(want)
    g64 = got.double()
    assert torch.equal(torch.isnan(g64), torch.isnan(want)), f'{what}: NaN pattern'
    inf = torch.isinf(want)
    assert torch.equal(g64[inf], want[inf]), f'{what}: infinities'
    if fin.any():
        ratio = ((g64 - want).abs()[fin] / bound[fin]).max().item()
        note(f'{key} {str(x.dtype).replace("torch.", "")} fwd', ratio)
        assert ratio <= 1.0, f'{what}: {ratio:.3f} x the derived bound'


def lse_grad64(x, y, g, lens, reverse, absolute=False):
    """sum_{t >= s (scan order)} g_t exp(x_s - y_t) per sequence in float64 (|g_t| with `absolute`); 0 where
    x_s = -inf."""
    out = []
    for xp, yp, gp in zip(pieces(x.double(), lens), pieces(y.double(), lens), pieces(g.double(), lens)):
        if xp.size(0) == 0:
            continue
        if not reverse:                      # tokens t >= s are the LATER ones: a suffix sum
            xp, yp, gp = xp.flip(0), yp.flip(0), gp.flip(0)
        if absolute:
            gp = gp.abs()
        fin = torch.isfinite(yp)
        c = torch.where(fin, yp, torch.full_like(yp, -math.inf)).amax(0, keepdim=True)
        c = torch.where(torch.isfinite(c), c, torch.zeros_like(c))
        # after the flip (or with `reverse`) the terms of token s are those at and BEFORE it in this order
        acc = torch.cumsum(gp * torch.exp(c - yp), 0) * torch.exp(xp - c)
        acc = torch.where(xp == -math.inf, torch.zeros_like(acc), acc)
        out.append(acc if reverse else acc.flip(0))
    return torch.cat(out) if out else x.double()


def check_lse_grad(got, x, y, g, lens, reverse, what, key):
    got, x, y, g, lens = got.cpu(), x.cpu(), y.cpu(), g.cpu(), lens.cpu()
    if got.numel() == 0:
        return
    want = lse_grad64(x, y, g, lens, reverse)
    bound = BAR * lse_grad64(x, y, g, lens, reverse, absolute=True)
    if x.dtype in (BF16, F16):
        bound = bound + 0.5 * ulp_at(want, x.dtype)
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got.double()), fin), f'{what}: non-finite pattern of the gradient'
    err = (got.double() - want).abs()[fin]
    assert bool((err[bound[fin] == 0] == 0).all()), f'{what}: a gradient that must be exactly 0 is not'
    nz = bound[fin] > 0
    if nz.any():
        ratio = (err[nz] / bound[fin][nz]).max().item()
        note(f'{key} {str(x.dtype).replace("torch.", "")} grad', ratio)
        assert ratio <= 1.0, f'{what}: {ratio:.3f} x the bar'


def draw(shape, dtype, seed):
    """The payloads of the GPU tests (CPU tensors): standard normal, rounded to `dtype`; int64 from 4 000 values."""
    gen = torch.Generator().manual_seed(seed)
    if dtype == I64:
        return torch.randint(-2000, 2000, shape, generator=gen, dtype=I64)
    return torch.randn(shape, generator=gen, dtype=F64 if dtype == F64 else F32).to(dtype)


# the lengths of the GPU tests (tests/test_gpu_cumsum.py: the smallest shapes that reach every form)
RAGGED = torch.tensor((0, 1, 31, 32, 33, 129, 2100, 64), dtype=torch.long)
CROSSING = torch.tensor((0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 5, 0, 4100), dtype=torch.long)
CUT = torch.tensor((8197, 8192 + 2048), dtype=torch.long)
