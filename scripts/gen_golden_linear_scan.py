"""Generate tests/golden/r9_linear_scan.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported
read-only, CPU autograd).  The reference has no per-sequence recurrence; what its users write is

    z, g = C.new(sequences), C.new(gates)
    l, a = z.left(), g.left()
    h = [l.data[:, 0]]
    for t in range(1, T):
        h.append(a.data[:, t] * h[-1] + l.data[:, t])
    y = l._replace(data=torch.stack(h, dim=1)).cat()                 # and back to the container they came from

and, for the return recursion (reverse=True), the same between two `.rev()`.  That composition, with its gradients for
the payload and the gate under a cotangent drawn from the stored seed, is what is recorded.  Only lengths, seeds and the
reference's outputs are stored — data, never reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_linear_scan.py PATH_OF_THE_REFERENCE_CHECKOUT

Payload and cotangent are `randn`.  Gates are +-exp(0.02 * randn) with about a quarter negative: running products stay
bounded over 8 000 tokens and nothing decays, so a lost or misplaced block carry shows at full size.  bf16 / f16 cases
draw all three in that dtype and the reference works on their fp32 upcast.  Scalar-gate cases store `gamma` (a constant
discount, representable in the payload dtype) and no gate gradient.  Inputs are never stored: draw(seed) reproduces them.

Per stored result the generator asserts that the reference is within HALF the bar the kernels are held to
(tests/test_linear_scan_surface.py: BAR * M_t, M the same recurrence in float64 on (|a|, |x|)) of an independent float64
per-sequence loop.

Per case `<name>/...`:
    lens, H (0 = a 1-D payload), dtype, seed, gamma (NaN: a tensor gate)
    y, yrev                       the reference's forward / reverse recurrences (fp32; fp64 for those cases), cat form
    gx, gxrev, ga, garev          their gradients under the cotangent (ga / garev: tensor gates only)
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
if len(sys.argv) < 2:
    sys.exit(__doc__)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# the float64 loop, the bound scales and draw(): ONE definition, the tests'
from test_linear_scan_surface import BAR, DTYPES, draw, grads64, scales64, scan64  # noqa: E402

for _name in [m for m in sys.modules if m == 'torchrua' or m.startswith('torchrua.')]:
    del sys.modules[_name]
sys.path.insert(0, sys.argv[1])
torch.set_num_threads(1)

from torchrua import C  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'r9_linear_scan.npz')
store = {}
worst = {'fwd': 0.0, 'gx': 0.0, 'ga': 0.0}


def reference(x, a, lens, reverse):
    """the reference's spelling: C.new -> (rev) -> left -> a loop over the time steps -> cat -> (rev)"""
    sizes = lens.tolist()
    z = C.new(list(torch.split(x, sizes, dim=0)))
    g = C.new(list(torch.split(a, sizes, dim=0))) if isinstance(a, torch.Tensor) else None
    if reverse:
        z, g = z.rev(), (g.rev() if g is not None else None)
    pad = z.left()
    gate = g.left().data if g is not None else None
    T = pad.data.size(1)
    h = [pad.data[:, 0]] if T else []
    for t in range(1, T):
        h.append((gate[:, t] if gate is not None else a) * h[-1] + pad.data[:, t])
    y = pad._replace(data=torch.stack(h, dim=1) if T else pad.data).cat()
    if reverse:
        y = y.rev()
    return y.data


def case(name, lens, H, dtype_name, seed, gamma=None):
    lens = torch.as_tensor(lens, dtype=torch.long)
    n = int(lens.sum())
    x, a, cot = draw(seed, n, H, dtype_name)

    def put(key, value):
        store[f'{name}/{key}'] = value.detach().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)

    put('lens', lens)
    put('H', H)
    put('dtype', dtype_name)
    put('seed', seed)
    put('gamma', float('nan') if gamma is None else float(gamma))
    x64, c64 = x.double().numpy(), cot.double().numpy()
    a64 = a.double().numpy() if gamma is None else float(gamma)
    for reverse, ykey, gxkey, gakey in ((False, 'y', 'gx', 'ga'), (True, 'yrev', 'gxrev', 'garev')):
        xr = x.clone().requires_grad_(True)
        ar = a.clone().requires_grad_(True) if gamma is None else float(gamma)
        y = reference(xr, ar, lens, reverse)
        if n:
            grads = torch.autograd.grad((y * cot).sum(), (xr, ar) if gamma is None else (xr,), allow_unused=True)
            grads = [torch.zeros_like(xr) if g is None else g for g in grads]
        else:
            grads = [torch.zeros_like(xr)] * 2
        y = y.detach()
        put(ykey, y)
        put(gxkey, grads[0])
        if gamma is None:
            put(gakey, grads[1])
        if not n:
            continue
        # ---- is the reference itself inside half the bar?
        want_y = scan64(x64, a64, lens, reverse)
        want_gx, want_ga = grads64(a64, c64, want_y, lens, reverse)
        M, Mdx, Mda = scales64(x64, a64, c64, lens, reverse)
        f = (np.abs(y.double().numpy() - want_y) / np.maximum(BAR * M, 1e-300)).max()
        gx = (np.abs(grads[0].double().numpy() - want_gx) / np.maximum(BAR * Mdx, 1e-300)).max()
        assert f <= 0.5 and gx <= 0.5, f'{name}: reference off float64 by fwd {f:.3f} gx {gx:.3f} of the bar'
        worst['fwd'], worst['gx'] = max(worst['fwd'], f), max(worst['gx'], gx)
        if gamma is None:
            ga = (np.abs(grads[1].double().numpy() - want_ga) / np.maximum(2 * BAR * Mda, 1e-300)).max()
            assert ga <= 0.5, f'{name}: reference off float64 by ga {ga:.3f} of the bar'
            worst['ga'] = max(worst['ga'], ga)


def main():
    seed = 9000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    # every length the kernels change their step at, 1-D payloads
    edges = [0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049]
    case('edges.h0.fp32', edges, 0, 'fp32', nxt())
    case('edges.h1.fp32', [33, 0, 257, 1, 65, 129], 1, 'fp32', nxt())
    for dt in ('fp64', 'bf16', 'fp16'):
        case(f'short.h0.{dt}', [0, 1, 7, 8, 9, 31, 32, 33, 0, 127, 129], 0, dt, nxt())
    # every width
    case('short.h3.fp32', [31, 0, 33, 1, 64], 3, 'fp32', nxt())
    case('short.h8.fp32', [65, 32, 0, 63], 8, 'fp32', nxt())
    case('short.h64.fp32', [33, 1, 0, 31], 64, 'fp32', nxt())
    case('short.h250.fp32', [1, 9, 0, 2], 250, 'fp32', nxt())
    # the other dtypes at a narrow, a one-vector and a wide row
    for dt in ('fp64', 'bf16', 'fp16'):
        case(f'short.h3.{dt}', [5, 0, 33, 1], 3, dt, nxt())
        case(f'short.h8.{dt}', [33, 0, 64, 2], 8, dt, nxt())
        case(f'short.h64.{dt}', [9, 0, 5], 64, dt, nxt())
    case('mid.h250.bf16', [12, 3], 250, 'bf16', nxt())
    # more than four blocks of 2 048 tokens
    case('long.h1.fp32', [8200, 257], 1, 'fp32', nxt())
    # scalar gates: constant discounts representable in every payload dtype
    case('scalar.h0.fp32', [0, 1, 9, 33, 129, 2049], 0, 'fp32', nxt(), gamma=0.96875)
    case('scalar.h8.bf16', [33, 0, 64, 2], 8, 'bf16', nxt(), gamma=0.5)
    case('scalar.h64.fp32', [33, 1, 0, 31], 64, 'fp32', nxt(), gamma=0.96875)
    case('scalar.h3.fp64', [5, 0, 33, 1], 3, 'fp64', nxt(), gamma=-0.96875)
    np.savez_compressed(OUT, **store)
    names = sorted(set(k.split('/')[0] for k in store))
    size = os.path.getsize(OUT)
    assert size < 1_000_000, size
    print(f'{len(names)} cases -> {OUT} ({size} bytes); worst reference error vs float64, as a fraction of the bar: '
          f'forward {worst["fwd"]:.3f}, grad_x {worst["gx"]:.3f}, grad_gate {worst["ga"]:.3f}')


if __name__ == '__main__':
    main()
