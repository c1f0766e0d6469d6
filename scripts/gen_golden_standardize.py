"""Generate tests/golden/r11_standardize.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported
read-only, CPU autograd).  The reference has no per-sequence variance or standardize; what its users write is

    mean = torchrua.segment_mean(x, sizes)
    dev  = x - torch.repeat_interleave(mean, sizes, dim=0)
    var0 = torchrua.segment_mean(dev * dev, sizes)                  # correction 1: var0 * n / (n - 1)
    y    = dev * torch.repeat_interleave((var + eps).rsqrt(), sizes, dim=0)

and that composition, with its gradients under stored cotangents, is what is recorded — for correction in {0, 1} and eps
in {1e-5, 0}.  Only inputs and the reference's outputs are stored — data, never reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_standardize.py PATH_OF_THE_REFERENCE_CHECKOUT

Payloads are `offset + scale * randn` with |offset| / scale <= 10, finite.  bf16 / f16 cases draw the payload and the
cotangents in that dtype and the reference works on their fp32 upcast.  Large inputs are regenerated from the stored
seed (`x` / `cot` are stored only when small; tests/norm_util.py:draw), results are always stored.

A case is kept only if the reference is within HALF of each bound of tests/norm_util.py of a float64 per-sequence
torch.var_mean / standardize (the kernels have the other half); a dropped case is printed, and at most 10 % may be
dropped.  The generator also checks, with the reference's own casts, that the L / P / R forms of every case are the same
cast of the cat result (the casts only move rows), which is why only the cat form is stored.

Per case `<name>/...`:
    lens, H (0 = a 1-D payload), dtype, seed, offset, scale
    x, cot                              only when N * max(H, 1) <= 1024
    mean, var0, var1                    [B, *H]; empty sequences: NaN (the reference's segment_mean gives 0 there: patched
                                        to torch's NaN); singletons: var1 is NaN — only that mask is meaningful
    y00, y01, y10, y11                  y<correction><eps: 0 = 1e-5, 1 = 0>, cat form; NaN where n - c <= 0 or var + eps == 0
    gy00, gy11                          d sum(y * cot) / dx for (correction 0, eps 1e-5) and (correction 1, eps 0)
    gvm0, gvm1                          d (sum(var_c * cv) + sum(mean * cm)) / dx
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
if len(sys.argv) < 2:
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

import torchrua as ref  # noqa: E402
from torchrua import C  # noqa: E402

import norm_util as U  # noqa: E402

store = {}
dropped = []
total = 0


def worst(err, bound):
    """max of err / (bound / 2) over the elements where the float64 value is finite (NaN masks must agree)."""
    fin = torch.isfinite(bound)
    assert torch.equal(torch.isnan(err) | ~fin, ~fin), 'the reference is not finite where float64 is'
    if not bool(fin.any()):
        return 0.0
    e, b = err[fin], bound[fin] / 2
    if bool(((b == 0) & (e != 0)).any()):
        return float('inf')
    return float((e / b.clamp_min(1e-300)).max())


def case(name, lens, H, dtype_name, offset, scale, seed):
    global total
    total += 1
    assert abs(offset) <= 10 * scale
    lens = torch.as_tensor(lens, dtype=torch.long)
    n = int(lens.sum())
    dt = U.DTYPES[dtype_name]
    x, cot, cv, cm = U.draw(seed, lens, H, dtype_name, offset, scale)
    shape1 = (lens.numel(),) + (1,) * (x.dim() - 1)
    nn = lens.to(x.dtype).reshape(shape1)
    nan = torch.full_like(cv, float('nan'))

    # ---- the reference
    xr = x.clone().requires_grad_(True)
    mean = ref.segment_mean(xr, lens)
    dev = xr - torch.repeat_interleave(mean, lens, dim=0)
    var = {0: ref.segment_mean(dev * dev, lens)}
    var[1] = var[0] * (nn / (nn - 1))
    res, ys = {}, {}
    for key, (c, eps) in U.COMBOS.items():
        ys[key] = dev * torch.repeat_interleave((var[c] + eps).rsqrt(), lens, dim=0)
        res['y' + key] = ys[key].detach()
    for key in U.GRAD_COMBOS:
        res['gy' + key], = torch.autograd.grad((ys[key] * cot).sum(), xr, retain_graph=True)
    live = (lens > 0).reshape(shape1)
    for c in (0, 1):
        # (a NaN variance — singletons at correction 1 — must poison its own sequence only: it leaves the sum)
        obj = (torch.nan_to_num(var[c], nan=0.0) * cv).sum() + (mean * cm).sum()
        res[f'gvm{c}'], = torch.autograd.grad(obj, xr, retain_graph=True)
    single = torch.repeat_interleave(lens == 1, lens)
    res['gvm1'][single] = float('nan')                       # singletons, correction 1: only the NaN mask is stored
    res['mean'] = torch.where(live, mean.detach(), nan)
    res['var0'] = torch.where(live, var[0].detach(), nan)
    res['var1'] = torch.where(live, var[1].detach(), nan)

    # ---- is the reference itself inside half of every bound?
    if n:
        ex = U.Exact(x, lens)
        w = {'mean': worst((res['mean'].double() - ex.mean).abs(), ex.mean_bound(dt))}
        for c in (0, 1):
            w[f'var{c}'] = worst((res[f'var{c}'].double() - ex.var(c)).abs(), ex.var_bound(c, dt))
        for key, (c, eps) in U.COMBOS.items():
            w['y' + key] = worst((res['y' + key].double() - ex.y(c, eps)).abs(), ex.y_bound(c, eps, dt))
        for key in U.GRAD_COMBOS:
            c, eps = U.COMBOS[key]
            want, norm = U.std_grad(ex.y(c, eps), ex.rstd(c, eps), cot, lens, c)
            rho = (ex.mean.abs() / torch.sqrt(ex.var(0) + eps))[ex.ids]
            w['gy' + key] = worst((res['gy' + key].double() - want).abs(), U.std_grad_bound(want, norm, dt, rho))
        for c in (0, 1):
            want, absdev, kv, km = U.vm_grad(x, ex.mean, cv, cm, lens, c)
            bound = U.vm_grad_bound(want, absdev, kv, km, ex.mean.abs()[ex.ids], dt, independent=True)
            w[f'gvm{c}'] = worst((res[f'gvm{c}'].double() - want).abs(), bound)
        bad = {k: v for k, v in w.items() if v > 1.0}
        if bad:
            print(f'DROPPED {name}: reference beyond half a bound: ' + ', '.join(f'{k} {v:.2f}x' for k, v in bad.items()))
            dropped.append(name)
            return
        print(f'{name}: worst reference error / half bound ' + ', '.join(f'{k} {v:.2f}' for k, v in w.items()))

    # ---- the other layouts are the same cast of the cat result (the reference's own casts)
    if n and lens.min() > 0:
        y = res['y00']
        cx, cy = C(data=x, token_sizes=lens), C(data=y, token_sizes=lens)
        for cast in (lambda z: z.left(0), lambda z: z.right(0), lambda z: z.pack()):
            assert torch.equal(cast(cy).cat().data, y) and torch.equal(cast(cx).cat().data, x), name

    def put(key, value):
        store[f'{name}/{key}'] = value.detach().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)

    for k, v in (('lens', lens), ('H', H), ('dtype', dtype_name), ('seed', seed), ('offset', float(offset)),
                 ('scale', float(scale))):
        put(k, v)
    if n * max(H, 1) <= U.STORE_INPUT_MAX:
        put('x', x)
        put('cot', cot)
    for k, v in res.items():
        put(k, v)


def main():
    rng = np.random.RandomState(11)
    seed = 11000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    short = lambda b: rng.randint(1, 65, b)          # noqa: E731  U(1, 64)
    # every width at short lengths, fp32, with offsets
    case('short.h0.fp32', short(20), 0, 'fp32', 0.0, 1.0, nxt())
    case('short.h3.fp32', short(10), 3, 'fp32', 5.0, 1.0, nxt())
    case('short.h8.fp32', short(6), 8, 'fp32', -20.0, 2.0, nxt())
    case('short.h64.fp32', rng.randint(2, 17, 3), 64, 'fp32', 1.0, 0.5, nxt())
    case('short.h250.fp32', [3, 4], 250, 'fp32', 3.0, 1.0, nxt())
    case('short.h512.fp32', [2, 3], 512, 'fp32', -1.0, 0.1, nxt())
    # the other dtypes
    for dt in ('fp64', 'bf16', 'fp16'):
        case(f'short.h0.{dt}', short(14), 0, dt, 2.0, 1.0, nxt())
        case(f'short.h8.{dt}', rng.randint(1, 33, 4), 8, dt, -10.0, 1.0, nxt())
        case(f'short.h64.{dt}', rng.randint(2, 9, 2), 64, dt, 0.5, 3.0, nxt())
    # longer sequences, small H
    case('mid.h0.fp32', rng.randint(8, 513, 4), 0, 'fp32', 10.0, 1.0, nxt())
    case('mid.h3.fp32', rng.randint(8, 513, 2), 3, 'fp32', 0.0, 3.0, nxt())
    case('mid.h8.bf16', [130], 8, 'bf16', 1.0, 1.0, nxt())
    case('long.h0.fp32', [1024, 700, 33], 0, 'fp32', 1.0, 1.0, nxt())
    case('long.h0.fp64', [1024, 17], 0, 'fp64', 10.0, 1.0, nxt())
    # empty sequences (first, last, adjacent), singletons
    case('empty.h0.fp32', [0, 5, 0, 0, 9, 1, 0], 0, 'fp32', 1.0, 1.0, nxt())
    case('empty.h8.fp32', [0, 0, 33, 2, 0, 17, 0], 8, 'fp32', -3.0, 1.0, nxt())
    case('empty.h64.bf16', [3, 0, 0, 5, 0], 64, 'bf16', 0.0, 1.0, nxt())
    case('singletons.h0.fp32', [1] * 9, 0, 'fp32', 3.0, 1.0, nxt())
    case('singletons.h3.fp32', [1, 1, 4, 1, 1], 3, 'fp32', 1.0, 1.0, nxt())
    assert len(dropped) * 10 <= total, f'{len(dropped)} of {total} cases dropped: more than 10 %'
    np.savez_compressed(U.GOLDEN, **store)
    names = sorted(set(k.split('/')[0] for k in store))
    print(f'{len(names)} of {total} cases -> {U.GOLDEN} ({os.path.getsize(U.GOLDEN)} bytes); dropped: {dropped or "none"}')


if __name__ == '__main__':
    main()
