"""What the var_mean / standardize tests and scripts/gen_golden_standardize.py share (no GPU needed): the fixture cases of
tests/golden/r11_standardize.npz, a float64 per-sequence reference and the error bounds.

Bounds — none comes from the code under test.  u = 2^-24 for fp32 accumulation (2^-53 for float64), BAR = 1e-5 (1e-12);
mu, sigma, var, y are the float64 values:
  y      |d| <= (BAR + 4 u rho) (1 + |y|),   rho = |mu| / sqrt(var0 + eps), var0 the correction-0 variance
  var    |d| <= (BAR + 4 u rho) var,         rho = |mu| / sigma;  exactly 0 where var == 0
  mean   |d| <= BAR max(|mu|, sigma)
  bf16 / f16 outputs: plus one ulp of the payload dtype at the expected value (2^-7 |w|, 2^-10 |w|) plus the smallest
  subnormal — check_grad's form in the softmax tests, because y crosses zero.
Why 4 u rho: the mean carries at least one rounding of relative size u, so the deviation x - mean inherits u |mu|
absolutely, i.e. u rho relative to sigma.
  rstd   |d| <= (BAR + 4 u rho) rstd, rho as for y: rstd = (var + eps)^-1/2 carries half the relative error of
         var + eps, which is at most var's; the other half covers the roundings of the division and the square root
  standardize gradient   BAR norm against the float64 evaluation of the backward formula on the y and rstd the forward
                         produced; (BAR + 4 u rho) norm against an independent gradient (the fixtures' reference);
                         norm = rstd (|g| + mean_t |g| + |y| sum_t |g y| / (n - c)).
                         A bf16 / f16 backward consumes the y it saved, ROUNDED to the payload dtype: dy <= h |y| with
                         h = 2^-8 (bf16: 8 significant bits, half an ulp at the bottom of a binade) or 2^-11 (f16).  In
                         rstd (g - mean g - y S), S = sum_t(g y) / (n - c), that moves y by h |y| and S by h sum|g y| /
                         (n - c): against an independent gradient a 16-bit payload gets 2 h rstd |y| sum_t|g y| / (n - c)
                         more (std_grad_rounded_y).
  var_mean gradient      BAR (|g_var| 2 (|x - mu| + u |mu|) / (n - c) + |g_mean| / n) against the float64 evaluation of the
                         backward formula on the mean the forward produced.  Against an INDEPENDENT gradient (the fixtures'
                         reference, float64 autograd) the two means differ by their own roundings, up to 4 u |mu| as in
                         the forward's budget, and x - mu may be arbitrarily small next to that; there the deviation's
                         term is |g_var| 2 (BAR |x - mu| + 4 u |mu|) / (n - c): vm_grad_bound(independent=True).
"""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r11_standardize.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
COMBOS = {'00': (0, 1e-5), '01': (0, 0.0), '10': (1, 1e-5), '11': (1, 0.0)}      # key -> (correction, eps)
GRAD_COMBOS = ('00', '11')                                                        # the y gradients that are stored
STORE_INPUT_MAX = 1024


def bar_u(dtype):
    return (1e-12, 2.0 ** -53) if dtype == torch.float64 else (1e-5, 2.0 ** -24)


def ulp_term(w, dtype):
    if dtype == torch.bfloat16:
        return 2.0 ** -7 * w.abs() + 2.0 ** -133
    if dtype == torch.float16:
        return 2.0 ** -10 * w.abs() + 2.0 ** -24
    return torch.zeros_like(w)


def draw(seed, lens, H, dtype_name, offset, scale):
    """(x, cot_y, cot_var, cot_mean) of a fixture case: the ONE definition (the generator imports it from here)."""
    g = torch.Generator().manual_seed(int(seed))
    n, B = int(lens.sum()), int(lens.numel())
    hid = () if H == 0 else (H,)
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    dt = DTYPES[dtype_name]
    x = (offset + scale * torch.randn((n,) + hid, generator=g, dtype=work)).to(dt).to(work)
    cot = torch.randn((n,) + hid, generator=g, dtype=work).to(dt).to(work)
    cv = torch.randn((B,) + hid, generator=g, dtype=work).to(dt).to(work)
    cm = torch.randn((B,) + hid, generator=g, dtype=work).to(dt).to(work)
    return x, cot, cv, cm


# ------------------------------------------------------------------ float64, per sequence, any device
def seg_ids(lens, device):
    lens = lens.to(device)
    return torch.repeat_interleave(torch.arange(lens.numel(), device=device), lens)


def seg_sum(v, ids, B):
    """[N, *H] -> [B, *H] per-sequence sums (float64 index_add)."""
    return torch.zeros((B,) + tuple(v.shape[1:]), dtype=v.dtype, device=v.device).index_add_(0, ids, v)


class Exact:
    """float64 two-pass statistics of a cat-form payload: n, mean, M2 [B, *H] (mean NaN for an empty sequence)."""

    def __init__(self, x, lens):
        self.x = x.double()
        self.B = int(lens.numel())
        self.ids = seg_ids(lens, x.device)
        shape = (self.B,) + (1,) * (x.dim() - 1)
        self.n = lens.to(x.device).double().reshape(shape)
        self.mean = seg_sum(self.x, self.ids, self.B) / self.n
        self.dev = self.x - self.mean[self.ids]
        self.m2 = seg_sum(self.dev * self.dev, self.ids, self.B)

    def var(self, c):
        dof = self.n - c
        return torch.where(dof > 0, self.m2 / dof.clamp_min(1), torch.full_like(self.m2, float('nan')))

    def rstd(self, c, eps):
        return 1.0 / torch.sqrt(self.var(c) + eps)

    def y(self, c, eps):
        return self.dev * self.rstd(c, eps)[self.ids]

    # ---- bounds
    def y_bound(self, c, eps, dtype):
        bar, u = bar_u(dtype)
        rho = self.mean.abs() / torch.sqrt(self.var(0) + eps)
        y = self.y(c, eps)
        return (bar + 4 * u * rho)[self.ids] * (1 + y.abs()) + ulp_term(y, dtype)

    def var_bound(self, c, dtype):
        bar, u = bar_u(dtype)
        var = self.var(c)
        rho = self.mean.abs() / torch.sqrt(var)
        b = (bar + 4 * u * rho) * var + ulp_term(var, dtype)
        return torch.where(var == 0, torch.zeros_like(b), b)

    def rstd_bound(self, c, eps, dtype):
        """rstd is kept in the accumulator type: no payload ulp."""
        bar, u = bar_u(dtype)
        rho = self.mean.abs() / torch.sqrt(self.var(0) + eps)
        return (bar + 4 * u * rho) * self.rstd(c, eps)

    def mean_bound(self, dtype):
        bar, _ = bar_u(dtype)
        return bar * torch.maximum(self.mean.abs(), torch.sqrt(self.var(0))) + ulp_term(self.mean, dtype)


def std_grad(y, rstd, g, lens, c):
    """(float64 backward formula of standardize on the given y [N, *H], rstd [B, *H] and cotangent, its norm)."""
    y, rstd, g = y.double(), rstd.double(), g.double()
    ids, B = seg_ids(lens, y.device), int(lens.numel())
    n = lens.to(y.device).double().reshape((B,) + (1,) * (y.dim() - 1))
    dof = torch.where(n - c > 0, n - c, torch.full_like(n, float('nan')))
    s1, s2 = seg_sum(g, ids, B) / n, seg_sum(g * y, ids, B) / dof
    want = rstd[ids] * (g - s1[ids] - y * s2[ids])
    norm = rstd[ids] * (g.abs() + (seg_sum(g.abs(), ids, B) / n)[ids] + y.abs() * (seg_sum((g * y).abs(), ids, B) / dof)[ids])
    return want, norm


def std_grad_rounded_y(y, rstd, g, lens, c, dtype):
    """What the rounding of the saved y to a bf16 / f16 payload can move the gradient by (0 for fp32 / fp64)."""
    if dtype not in (torch.bfloat16, torch.float16):
        return torch.zeros_like(y.double())
    h = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    y, rstd, g = y.double(), rstd.double(), g.double()
    ids, B = seg_ids(lens, y.device), int(lens.numel())
    n = lens.to(y.device).double().reshape((B,) + (1,) * (y.dim() - 1))
    dof = torch.where(n - c > 0, n - c, torch.full_like(n, float('nan')))
    return 2 * h * rstd[ids] * y.abs() * (seg_sum((g * y).abs(), ids, B) / dof)[ids]


def std_grad_bound(want, norm, dtype, rho=None):
    bar, u = bar_u(dtype)
    return (bar + (4 * u * rho if rho is not None else 0.0)) * norm + ulp_term(want, dtype)


def vm_grad(x, mean, gvar, gmean, lens, c):
    """(float64 backward formula of var_mean on the given mean [B, *H], |x - mean| and the two per-row factors)."""
    x, mean = x.double(), mean.double()
    ids, B = seg_ids(lens, x.device), int(lens.numel())
    n = lens.to(x.device).double().reshape((B,) + (1,) * (x.dim() - 1))
    dof = torch.where(n - c > 0, n - c, torch.full_like(n, float('nan')))
    kv = (2 * gvar.double() / dof)[ids]
    km = (gmean.double() / n)[ids]
    dev = x - mean[ids]
    return kv * dev + km, dev.abs(), kv.abs(), km.abs()


def vm_grad_bound(want, absdev, kv, km, mu, dtype, independent=False):
    """mu: |mean| spread over the rows.  See the module docstring for the two forms."""
    bar, u = bar_u(dtype)
    if independent:
        return kv * (bar * absdev + 4 * u * mu) + bar * km + ulp_term(want, dtype)
    return bar * (kv * (absdev + u * mu) + km) + ulp_term(want, dtype)


# ------------------------------------------------------------------ the fixture file
def load_cases():
    z = np.load(GOLDEN)
    names = sorted(set(k.split('/')[0] for k in z.files))
    out = {}
    for name in names:
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['H'], c['seed'], c['dtype'] = int(c['H']), int(c['seed']), str(c['dtype'])
        c['offset'], c['scale'] = float(c['offset']), float(c['scale'])
        c['lens'] = torch.from_numpy(c['lens'].astype(np.int64))
        x, cot, cv, cm = draw(c['seed'], c['lens'], c['H'], c['dtype'], c['offset'], c['scale'])
        if 'x' in c:
            assert np.array_equal(c['x'], x.numpy()) and np.array_equal(c['cot'], cot.numpy()), \
                f'{name}: the generator of this torch build does not reproduce the stored inputs'
        c['x'], c['cot'], c['cv'], c['cm'] = x, cot, cv, cm
        for k in list(c):
            if isinstance(c[k], np.ndarray) and k not in ('lens',):
                c[k] = torch.from_numpy(c[k])
        out[name] = c
    return out
