"""What the softmax_pool tests and scripts/gen_golden_pool.py share (plain torch, no GPU): the ONE definition of a fixture
case's inputs, the float64 per-sequence evaluation, and the error bounds.

Bounds (the project's bound for sums; none of them comes from what the kernels give), with p = softmax of a sequence's
scores, g the cotangent row of the sequence and a_t = sum over the columns h of a score column of |v[t,h] * g[h]|:
    forward      |d| <= 1e-5 * sum_t p_t |v[t,h]|
    grad_values  |d| <= 1e-5 * p_t |g[h]|
    grad_scores  |d| <= 1e-5 * p_t (a_t + sum_t' p_t' a_t')
bf16 / f16 results add one unit in the last place of the payload dtype at the wanted value."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r10_softmax_pool.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
BAR = 1e-5
STORE_INPUT_MAX = 1024


def prod(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


def draw(seed, lens, hidden, shidden, dtype_name, scale):
    """(values [N, *hidden], scores [N, *shidden], cot [B, *hidden]) of a case, exactly representable in its dtype."""
    g = torch.Generator().manual_seed(int(seed))
    n, B = int(lens.sum()), int(lens.numel())
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    dt = DTYPES[dtype_name]
    v = torch.randn((n,) + tuple(hidden), generator=g, dtype=work).to(dt).to(work)
    s = (torch.randn((n,) + tuple(shidden), generator=g, dtype=work) * scale).to(dt).to(work)
    cot = torch.randn((B,) + tuple(hidden), generator=g, dtype=work).to(dt).to(work)
    return v, s, cot


def exact(v, s, cot, lens, want_grad=True):
    """float64: (torch.softmax(s_seq, 0)[..., None] * v_seq).sum(0) of every sequence, its gradients under `cot`, and the
    three bounds WITHOUT their 1e-5 factor.  Cat form; returns a dict of tensors shaped like out / v / s."""
    lens = lens.cpu()
    B, n = int(lens.numel()), int(v.shape[0])
    hidden, shidden = tuple(v.shape[1:]), tuple(s.shape[1:])
    H, G = prod(hidden), prod(shidden)
    D = H // G if G else 1
    v64 = v.detach().double().cpu().reshape(n, G, D).clone().requires_grad_(want_grad)
    s64 = s.detach().double().cpu().reshape(n, G).clone().requires_grad_(want_grad)
    outs, ps = [], []
    for vp, sp in zip(torch.split(v64, lens.tolist()), torch.split(s64, lens.tolist())):
        p = torch.softmax(sp, dim=0)
        ps.append(p)
        outs.append((p[..., None] * vp).sum(0))
    out = torch.stack(outs) if outs else v64.new_zeros((0, G, D))
    res = {'out': out.detach().reshape((B,) + hidden)}
    p = torch.cat(ps).detach() if ps else s64.detach()
    seq = torch.repeat_interleave(torch.arange(B), lens)

    def seg(x):                                    # per-sequence sum of [n, ...] rows -> [B, ...]
        return torch.zeros((B,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, seq, x)
    va = v64.detach().abs()
    res['b_out'] = seg(p[..., None] * va).reshape((B,) + hidden)
    if cot is not None:
        c64 = cot.detach().double().cpu().reshape(B, G, D)
        if want_grad and n:
            gv, gs = torch.autograd.grad((out * c64).sum(), [v64, s64])
        else:
            gv, gs = torch.zeros_like(v64), torch.zeros_like(s64)
        res['gv'], res['gs'] = gv.reshape((n,) + hidden), gs.reshape((n,) + shidden)
        crow = c64[seq]                            # [n, G, D]
        res['b_gv'] = (p[..., None] * crow.abs()).reshape((n,) + hidden)
        a = (va * crow.abs()).sum(-1)              # [n, G]
        res['b_gs'] = (p * (a + seg(p * a)[seq])).reshape((n,) + shidden)
    return res


def ulp(want, dtype):
    """One unit in the last place of `dtype` at `want` (0 for fp32 / fp64: their bound is the 1e-5 one alone)."""
    if dtype in (torch.float32, torch.float64):
        return torch.zeros_like(want)
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    w = torch.nan_to_num(want.abs(), nan=1.0, posinf=1.0)
    e = torch.floor(torch.log2(w.clamp_min(2.0 ** emin)))
    return torch.pow(torch.full_like(e, 2.0), e - mant)


def ratio(got, want, bound, dtype=torch.float32):
    """The worst |got - want| / (1e-5 * bound [+ 1 ulp]); elements with a zero bound must be exact."""
    got, want, bound = got.detach().double().cpu(), want.double().cpu(), bound.double().cpu()
    if got.numel() == 0:
        return 0.0
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), 'NaN positions differ'
    ok = torch.isfinite(want)
    lim = BAR * bound + ulp(want, dtype)
    d = (got - want).abs()
    zero = ok & (lim == 0)
    assert bool((d[zero] == 0).all()), 'an element with a zero bound is not exact'
    live = ok & (lim > 0)
    return float((d[live] / lim[live]).max()) if bool(live.any()) else 0.0


def load_cases():
    z = np.load(GOLDEN)
    out = {}
    for name in sorted(set(k.split('/')[0] for k in z.files)):
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['H'], c['D'], c['seed'], c['scale'], c['dtype'] = int(c['H']), int(c['D']), int(c['seed']), float(c['scale']), str(c['dtype'])
        c['hidden'] = tuple(int(d) for d in c['hidden'])
        c['shidden'] = tuple(int(d) for d in c['shidden'])
        assert prod(c['hidden']) == c['H'] and prod(c['shidden']) * c['D'] == c['H'], name
        c['lens'] = torch.from_numpy(c['lens'].astype(np.int64))
        v, s, cot = draw(c['seed'], c['lens'], c['hidden'], c['shidden'], c['dtype'], c['scale'])
        if 'v' in c:
            assert np.array_equal(c['v'], v.numpy()) and np.array_equal(c['s'], s.numpy()) and \
                np.array_equal(c['cot'], cot.numpy()), f'{name}: this torch build does not reproduce the stored inputs'
        c['v'], c['s'], c['cot'] = v, s, cot
        for k in ('out', 'gv', 'gs'):
            c[k] = torch.from_numpy(c[k])
        out[name] = c
    return out
