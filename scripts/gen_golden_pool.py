"""Generate tests/golden/r10_softmax_pool.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported
read-only, CPU autograd).  The reference has no attention pooling; what its users write is

    lse = torchrua.segment_logsumexp(s, sizes)
    w   = (s - torch.repeat_interleave(lse, sizes, dim=0)).exp()            # [N, *prefix]
    out = torchrua.segment_sum(w[..., None] * v, sizes)                     # w broadcast over the rest of hidden

and that composition, with its gradients to v and s under a stored cotangent, is what is recorded.  Only inputs and the
reference's outputs are stored — data, never reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_pool.py PATH_OF_THE_REFERENCE_CHECKOUT

Finite inputs only.  Values and cotangent are randn, scores `scale * randn` with scale <= 3.  bf16 / f16 cases draw all
three in that dtype and the reference works on their fp32 upcast.  Large inputs are regenerated from the stored seed by
tests/pool_util.py:draw (the one definition, imported here); `v`, `s`, `cot` are stored only when small; results always.

A case whose reference result is not within HALF the bar of the tests (0.5 x the bounds of tests/pool_util.py) of the
float64 per-sequence evaluation is dropped; the worst kept ratio is printed.

Per case `<name>/...`:
    lens, hidden, shidden, H, D, dtype, seed, scale
    v, s, cot                     only when N * H <= 1024
    out, gv, gs                   the reference's results (fp32; fp64 for fp64 cases), cat form
"""
import os
import sys

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True
if len(sys.argv) < 2:
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

import torchrua as ref  # noqa: E402

from pool_util import GOLDEN, STORE_INPUT_MAX, draw, exact, prod, ratio  # noqa: E402

store = {}
worst = {'out': 0.0, 'gv': 0.0, 'gs': 0.0}


def case(name, lens, hidden, shidden, dtype_name, scale, seed):
    lens = torch.as_tensor(np.asarray(lens), dtype=torch.long)
    n = int(lens.sum())
    H, G = prod(hidden), prod(shidden)
    D = H // G
    v, s, cot = draw(seed, lens, hidden, shidden, dtype_name, scale)

    # ---- the reference
    vr, sr = v.clone().requires_grad_(True), s.clone().requires_grad_(True)
    lse = ref.segment_logsumexp(sr, lens)
    w = (sr - torch.repeat_interleave(lse, lens, dim=0)).exp()
    weighted = (w.reshape(n, G, 1) * vr.reshape(n, G, D)).reshape((n,) + tuple(hidden))
    out = ref.segment_sum(weighted, lens)
    gv, gs = torch.autograd.grad((out * cot).sum(), [vr, sr])
    out = out.detach()

    # ---- is the reference itself inside half the bar?
    e = exact(v, s, cot, lens)
    r = {'out': ratio(out, e['out'], e['b_out']), 'gv': ratio(gv, e['gv'], e['b_gv']), 'gs': ratio(gs, e['gs'], e['b_gs'])}
    if max(r.values()) > 0.5:
        print(f'DROPPED {name}: reference at {r} of the bar')
        return
    for k in worst:
        worst[k] = max(worst[k], r[k])

    def put(key, value):
        store[f'{name}/{key}'] = value.detach().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)

    put('lens', lens)
    put('hidden', np.asarray(hidden, dtype=np.int64))
    put('shidden', np.asarray(shidden, dtype=np.int64))
    put('H', H)
    put('D', D)
    put('dtype', dtype_name)
    put('seed', seed)
    put('scale', float(scale))
    if n * H <= STORE_INPUT_MAX:
        put('v', v)
        put('s', s)
        put('cot', cot)
    put('out', out)
    put('gv', gv)
    put('gs', gs)


def main():
    rng = np.random.RandomState(10)
    seed = 10000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    short = lambda b: rng.randint(1, 65, b)          # noqa: E731  U(1, 64)
    mid = lambda b: rng.randint(8, 513, b)           # noqa: E731  U(8, 512)
    long_ = lambda b: rng.randint(16, 1025, b)       # noqa: E731  U(16, 1024)
    shapes = (((), ()), ((3,), ()), ((8,), ()), ((64,), ()), ((4, 16), (4,)), ((3, 5), (3,)), ((64,), (64,)),
              ((250,), ()), ((512,), ()))

    def tag(hidden, shidden):
        return 'h' + 'x'.join(map(str, hidden)) + '.s' + 'x'.join(map(str, shidden))

    # every shape at short lengths, fp32
    for hidden, shidden in shapes:
        H = prod(hidden)
        lens = short(12) if H <= 8 else (short(3) if H <= 64 else rng.randint(1, 9, 2))
        case(f'short.{tag(hidden, shidden)}.fp32', lens, hidden, shidden, 'fp32', 1.0, nxt())
    # the other dtypes
    for dt in ('fp64', 'bf16', 'fp16'):
        case(f'short.h.s.{dt}', short(16), (), (), dt, 1.0, nxt())
        case(f'short.h8.s.{dt}', short(5), (8,), (), dt, 3.0, nxt())
        case(f'short.h4x16.s4.{dt}', rng.randint(1, 17, 3), (4, 16), (4,), dt, 1.0, nxt())
        case(f'short.h3x5.s3.{dt}', short(4), (3, 5), (3,), dt, 2.0, nxt())
        case(f'short.h64.s64.{dt}', rng.randint(1, 17, 3), (64,), (64,), dt, 1.0, nxt())
    # longer sequences, small H
    case('mid.h.s.fp32', mid(8), (), (), 'fp32', 3.0, nxt())
    case('mid.h3.s.fp32', mid(5), (3,), (), 'fp32', 1.0, nxt())
    case('mid.h8.s.bf16', mid(2), (8,), (), 'bf16', 1.0, nxt())
    case('mid.h8.s.fp32', mid(2), (8,), (), 'fp32', 3.0, nxt())
    case('mid.h3x5.s3.fp32', mid(2), (3, 5), (3,), 'fp32', 2.0, nxt())
    case('long.h.s.fp32', long_(6), (), (), 'fp32', 1.0, nxt())
    case('long.h3.s.fp32', long_(3), (3,), (), 'fp32', 3.0, nxt())
    case('long.h8.s.fp32', long_(2), (8,), (), 'fp32', 1.0, nxt())
    case('long.h.s.fp64', long_(4), (), (), 'fp64', 3.0, nxt())
    # empty sequences (first, last, adjacent), singletons
    case('empty.h.s.fp32', [0, 5, 0, 0, 9, 1, 0], (), (), 'fp32', 1.0, nxt())
    case('empty.h8.s.fp32', [0, 0, 33, 2, 0, 70, 0], (8,), (), 'fp32', 3.0, nxt())
    case('empty.h4x16.s4.bf16', [3, 0, 0, 12, 0], (4, 16), (4,), 'bf16', 1.0, nxt())
    case('singletons.h.s.fp32', [1] * 9, (), (), 'fp32', 3.0, nxt())
    case('singletons.h3x5.s3.fp32', [1, 1, 4, 1, 1], (3, 5), (3,), 'fp32', 1.0, nxt())
    np.savez_compressed(GOLDEN, **store)
    names = sorted(set(k.split('/')[0] for k in store))
    print(f'{len(names)} cases -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes); worst kept reference error / bar: '
          f'out {worst["out"]:.3f}, grad_values {worst["gv"]:.3f}, grad_scores {worst["gs"]:.3f}')


if __name__ == '__main__':
    main()
