"""Generate tests/golden/r8_cumsum.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported read-only,
CPU autograd).  The reference has no per-sequence cumsum; what its users write is

    z = C.new(sequences)
    l = z.left()
    y = l._replace(data=torch.cumsum(l.data, dim=1)).cat()

and, for the suffix sums, the same between two `.rev()`.  That composition, with its gradient under a cotangent drawn
from the stored seed, is what is recorded.  Only lengths, seeds and the reference's outputs are stored — data, never
reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_cumsum.py PATH_OF_THE_REFERENCE_CHECKOUT

Float payloads are `randn`; bf16 / f16 cases draw the payload and the cotangent in that dtype and the reference works on
their fp32 upcast.  int64 payloads are integers in [-1000, 1000] and carry no gradient.  Inputs are never stored:
draw(seed) below reproduces them.

Per stored float result the generator asserts that the reference is within 5e-6 * sum_{s<=t} |x_s| (suffix sums for the
reverse direction; sums of |cot| for the gradients) of a float64 per-sequence torch.cumsum — half of the 1e-5 bar the
kernels are held to.  int64 results are asserted equal.

Per case `<name>/...`:
    lens, H (0 = a 1-D payload), dtype, seed
    y, yrev                       the reference's prefix / suffix sums (fp32; fp64 and int64 for those cases), cat form
    gx, gxrev                     their gradients under the cotangent (float cases only)
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

from torchrua import C  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'r8_cumsum.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16,
          'int64': torch.int64}
HALF_BAR = 5e-6
store = {}
worst = {'fwd': 0.0, 'grad': 0.0}


def draw(seed, n, H, dtype_name):
    """(x, cot) of a case: the ONE definition the tests repeat (tests/test_cumsum_surface.py)."""
    g = torch.Generator().manual_seed(int(seed))
    shape = (n,) if H == 0 else (n, H)
    if dtype_name == 'int64':
        return torch.randint(-1000, 1001, shape, generator=g, dtype=torch.int64), None
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    x = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    cot = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    return x, cot


def seg_cumsum(v, lens, reverse):
    """per-sequence torch.cumsum of a cat-form payload (in the dtype of `v`)."""
    out = []
    for piece in torch.split(v, lens.tolist(), dim=0):
        out.append(piece.flip(0).cumsum(0).flip(0) if reverse else piece.cumsum(0))
    return torch.cat(out) if out else v.clone()


def reference(x, lens, reverse):
    """the reference's spelling: C.new -> (rev) -> left -> torch.cumsum(dim=1) -> cat -> (rev)"""
    z = C.new(list(torch.split(x, lens.tolist(), dim=0)))
    if reverse:
        z = z.rev()
    pad = z.left()
    y = pad._replace(data=torch.cumsum(pad.data, dim=1)).cat()
    if reverse:
        y = y.rev()
    return y.data


def case(name, lens, H, dtype_name, seed):
    lens = torch.as_tensor(lens, dtype=torch.long)
    n = int(lens.sum())
    x, cot = draw(seed, n, H, dtype_name)

    def put(key, value):
        store[f'{name}/{key}'] = value.detach().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)

    put('lens', lens)
    put('H', H)
    put('dtype', dtype_name)
    put('seed', seed)
    for reverse, ykey, gkey in ((False, 'y', 'gx'), (True, 'yrev', 'gxrev')):
        if dtype_name == 'int64':
            y = reference(x, lens, reverse)
            assert torch.equal(y, seg_cumsum(x, lens, reverse)), name
            put(ykey, y)
            continue
        xr = x.clone().requires_grad_(True)
        y = reference(xr, lens, reverse)
        gx, = torch.autograd.grad((y * cot).sum(), xr)
        y = y.detach()
        # ---- is the reference itself inside half the bar?
        f = ((y.double() - seg_cumsum(x.double(), lens, reverse)).abs()
             / seg_cumsum(x.double().abs(), lens, reverse).clamp_min(1e-300)).max().item()
        g = ((gx.double() - seg_cumsum(cot.double(), lens, not reverse)).abs()
             / seg_cumsum(cot.double().abs(), lens, not reverse).clamp_min(1e-300)).max().item()
        assert f <= HALF_BAR and g <= HALF_BAR, f'{name}: reference off float64 by fwd {f:.2e} grad {g:.2e}'
        worst['fwd'], worst['grad'] = max(worst['fwd'], f), max(worst['grad'], g)
        put(ykey, y)
        put(gkey, gx)


def main():
    seed = 8000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    # every length the kernels change their step at, 1-D payloads of every dtype split between them
    edges = [0, 1, 31, 32, 33, 63, 64, 65, 255, 257, 2047, 2048, 2049]
    case('edges.h0.fp32', edges, 0, 'fp32', nxt())
    case('edges.h1.fp32', [33, 0, 64, 1, 65, 257], 1, 'fp32', nxt())
    for dt in ('fp64', 'bf16', 'fp16', 'int64'):
        case(f'short.h0.{dt}', [0, 1, 31, 32, 33, 63, 64, 65, 0, 255, 257], 0, dt, nxt())
    # every width
    case('short.h3.fp32', [31, 0, 33, 1, 64], 3, 'fp32', nxt())
    case('short.h8.fp32', [65, 32, 0, 63], 8, 'fp32', nxt())
    case('short.h64.fp32', [33, 1, 0, 31], 64, 'fp32', nxt())
    case('short.h250.fp32', [1, 9, 0, 2], 250, 'fp32', nxt())
    case('short.h512.fp32', [3, 0, 5], 512, 'fp32', nxt())
    # the other dtypes at a narrow, a one-vector and a wide row
    for dt in ('fp64', 'bf16', 'fp16', 'int64'):
        case(f'short.h3.{dt}', [5, 0, 33, 1], 3, dt, nxt())
        case(f'short.h8.{dt}', [33, 0, 64, 2], 8, dt, nxt())
        case(f'short.h64.{dt}', [9, 0, 5], 64, dt, nxt())
    case('mid.h250.bf16', [12, 3], 250, 'bf16', nxt())
    # two sequences of more than four blocks of 2 048 tokens
    case('long.h1.fp32', [8200, 8193], 1, 'fp32', nxt())
    np.savez_compressed(OUT, **store)
    names = sorted(set(k.split('/')[0] for k in store))
    size = os.path.getsize(OUT)
    assert size < 1_000_000, size
    print(f'{len(names)} cases -> {OUT} ({size} bytes); worst reference error vs float64 over prefix sum |x|: '
          f'forward {worst["fwd"]:.2e}, gradient {worst["grad"]:.2e}')


if __name__ == '__main__':
    main()
