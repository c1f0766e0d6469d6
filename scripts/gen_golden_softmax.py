"""Generate tests/golden/r7_softmax.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported read-only,
CPU autograd).  The reference has no per-sequence softmax; what its users write is

    lse = torchrua.segment_logsumexp(x, sizes)
    y   = (x - torch.repeat_interleave(lse, sizes, dim=0)).exp()        # log variant: without .exp()

and that composition, with its gradient under a stored cotangent, is what is recorded.  Only inputs and the reference's
outputs are stored — data, never reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_softmax.py PATH_OF_THE_REFERENCE_CHECKOUT

Finite inputs only (the reference's segment_logsumexp poisons the whole tensor on one NaN; this operator does not).
Payloads are `scale * randn`, scale <= 3.  bf16 / f16 cases draw the payload and the cotangent in that dtype and the
reference works on their fp32 upcast.  Large inputs are regenerated from the stored seed (`x` / `cot` are stored only
when small), results are always stored.

Per stored case the generator asserts that the reference is within 5e-6 of a float64 per-sequence torch.softmax /
torch.log_softmax — half of the 1e-5 bar the kernels are held to — forward (relative; log: 1e-5-style `max(1, |y|)` floor)
and gradient (normalised by y * (|g| + sum|g y|), log: |g| + exp(y) * sum|g|); a case that is not is dropped.  It also
checks, with the reference's own casts, that the L / P / R forms of every case are the same cast of the cat result (the
casts only move rows), which is why only the cat form is stored: the tests cast it.

Per case `<name>/...`:
    lens, H (0 = a 1-D payload), dtype, seed, scale
    x, cot                        only when N * max(H, 1) <= 1024; otherwise draw(seed) below reproduces them
    y, ylog, gx, gxlog            the reference's results (fp32; fp64 for fp64 cases), cat form
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

import torchrua as ref  # noqa: E402
from torchrua import C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'r7_softmax.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
STORE_INPUT_MAX = 1024
HALF_BAR = 5e-6
store = {}
worst = {'fwd': 0.0, 'grad': 0.0}


def draw(seed, n, H, dtype_name, scale):
    """(x, cot) of a case: the ONE definition the tests repeat (tests/test_gpu_softmax.py, test_softmax_surface.py)."""
    g = torch.Generator().manual_seed(int(seed))
    shape = (n,) if H == 0 else (n, H)
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    x = (torch.randn(shape, generator=g, dtype=work) * scale).to(DTYPES[dtype_name]).to(work)
    cot = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    return x, cot


def exact(x, cot, lens):
    """float64 per-sequence torch.softmax / log_softmax and their gradients."""
    x64 = x.double().clone().requires_grad_(True)
    c64 = cot.double()
    ys, yl = [], []
    for piece in torch.split(x64, lens.tolist(), dim=0):
        ys.append(torch.softmax(piece, dim=0))
        yl.append(torch.log_softmax(piece, dim=0))
    y, ylog = torch.cat(ys), torch.cat(yl)
    gx, = torch.autograd.grad((y * c64).sum(), x64, retain_graph=True)
    gxl, = torch.autograd.grad((ylog * c64).sum(), x64)
    return y.detach(), ylog.detach(), gx, gxl


def seg_abs_sum(v, lens):
    return torch.repeat_interleave(torch.stack([p.sum(dim=0) for p in torch.split(v, lens.tolist(), dim=0)]), lens, dim=0)


def case(name, lens, H, dtype_name, scale, seed):
    lens = torch.as_tensor(lens, dtype=torch.long)
    n = int(lens.sum())
    x, cot = draw(seed, n, H, dtype_name, scale)

    # ---- the reference
    xr = x.clone().requires_grad_(True)
    lse = ref.segment_logsumexp(xr, lens)
    ylog = xr - torch.repeat_interleave(lse, lens, dim=0)
    y = ylog.exp()
    gx, = torch.autograd.grad((y * cot).sum(), xr, retain_graph=True)
    gxl, = torch.autograd.grad((ylog * cot).sum(), xr)
    y, ylog = y.detach(), ylog.detach()

    # ---- is the reference itself inside half the bar?
    if n:
        ey, eyl, egx, egxl = exact(x, cot, lens)
        live = torch.repeat_interleave(lens, lens) > 0            # (every stored row belongs to a non-empty sequence)
        assert bool(live.all())
        f1 = ((y.double() - ey).abs() / ey).max().item()
        f2 = ((ylog.double() - eyl).abs() / eyl.abs().clamp_min(1.0)).max().item()
        n1 = ey * (cot.double().abs() + seg_abs_sum((cot.double() * ey).abs(), lens))
        n2 = cot.double().abs() + eyl.exp() * seg_abs_sum(cot.double().abs(), lens)
        g1 = ((gx.double() - egx).abs() / n1).max().item()
        g2 = ((gxl.double() - egxl).abs() / n2).max().item()
        if max(f1, f2, g1, g2) > HALF_BAR:
            print(f'DROPPED {name}: reference off float64 by fwd {max(f1, f2):.2e} grad {max(g1, g2):.2e}')
            return
        worst['fwd'] = max(worst['fwd'], f1, f2)
        worst['grad'] = max(worst['grad'], g1, g2)

    # ---- the other layouts are the same cast of the cat result (the reference's own casts)
    if n and lens.min() > 0:
        cx, cy = C(data=x, token_sizes=lens), C(data=y, token_sizes=lens)
        for cast in (lambda z: z.left(0), lambda z: z.right(0), lambda z: z.pack()):
            assert torch.equal(cast(cy).cat().data, y) and torch.equal(cast(cx).cat().data, x), name

    def put(key, value):
        store[f'{name}/{key}'] = value.detach().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)

    put('lens', lens)
    put('H', H)
    put('dtype', dtype_name)
    put('seed', seed)
    put('scale', float(scale))
    if n * max(H, 1) <= STORE_INPUT_MAX:
        put('x', x)
        put('cot', cot)
    put('y', y)
    put('ylog', ylog)
    put('gx', gx)
    put('gxlog', gxl)


def main():
    rng = np.random.RandomState(7)
    seed = 7000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    short = lambda b: rng.randint(1, 65, b)          # noqa: E731  U(1, 64)
    mid = lambda b: rng.randint(8, 513, b)           # noqa: E731  U(8, 512)
    long_ = lambda b: rng.randint(16, 1025, b)       # noqa: E731  U(16, 1024)
    # every width at short lengths, fp32
    for H, b in ((0, 24), (3, 16), (8, 12), (64, 3), (250, 2), (512, 2)):
        case(f'short.h{H}.fp32', short(b) if H < 250 else rng.randint(1, 9, b), H, 'fp32', 1.0, nxt())
    # the other dtypes
    for dt in ('fp64', 'bf16', 'fp16'):
        case(f'short.h0.{dt}', short(16), 0, dt, 1.0, nxt())
        case(f'short.h8.{dt}', short(5), 8, dt, 3.0, nxt())
        case(f'short.h64.{dt}', rng.randint(1, 17, 3), 64, dt, 1.0, nxt())
    # longer sequences, small H
    case('mid.h0.fp32', mid(8), 0, 'fp32', 3.0, nxt())
    case('mid.h3.fp32', mid(5), 3, 'fp32', 1.0, nxt())
    case('mid.h8.bf16', mid(2), 8, 'bf16', 1.0, nxt())
    case('mid.h8.fp32', mid(2), 8, 'fp32', 3.0, nxt())
    case('long.h0.fp32', long_(6), 0, 'fp32', 1.0, nxt())
    case('long.h3.fp32', long_(3), 3, 'fp32', 3.0, nxt())
    case('long.h8.fp32', long_(2), 8, 'fp32', 1.0, nxt())
    case('long.h0.fp64', long_(4), 0, 'fp64', 3.0, nxt())
    # empty sequences (first, last, adjacent), singletons
    case('empty.h0.fp32', [0, 5, 0, 0, 9, 1, 0], 0, 'fp32', 1.0, nxt())
    case('empty.h8.fp32', [0, 0, 33, 2, 0, 70, 0], 8, 'fp32', 3.0, nxt())
    case('empty.h64.bf16', [3, 0, 0, 12, 0], 64, 'bf16', 1.0, nxt())
    case('singletons.h0.fp32', [1] * 9, 0, 'fp32', 3.0, nxt())
    case('singletons.h3.fp32', [1, 1, 4, 1, 1], 3, 'fp32', 1.0, nxt())
    np.savez_compressed(OUT, **store)
    names = sorted(set(k.split('/')[0] for k in store))
    print(f'{len(names)} cases -> {OUT} ({os.path.getsize(OUT)} bytes); worst kept reference error vs float64: '
          f'forward {worst["fwd"]:.2e}, gradient {worst["grad"]:.2e}')


if __name__ == '__main__':
    main()
