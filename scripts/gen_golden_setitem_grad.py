"""Generate tests/golden/r6_setitem_grad.npz by running the REFERENCE itself (speedcell4/torchrua 0.5.1, imported
read-only, CPU autograd): `z[batch_ptr, token_ptr] = v`, `z[Z] = v`, `z[tensor] = v` and `tensor[Z] = v` for the four
layouts, with the written storage and the gradients w.r.t. the base and the value under one fixed cotangent.  Only inputs
and the reference's outputs are stored — data, never reference source.

    PYTHONDONTWRITEBYTECODE=1 python scripts/gen_golden_setitem_grad.py PATH_OF_THE_REFERENCE_CHECKOUT

Every value and cotangent is an INTEGER-VALUED float, small enough that every sum stays exactly representable in the
case's dtype (bf16 included): the row sum of a broadcast value is then exact in any order and the tests compare bit for
bit.  Per case `<name>/...`:
    kind, dtype, form, unique     the layout, the payload dtype, the key form, 1 when no storage row is named twice
    lens (+ batch_sizes, sorted_indices, unsorted_indices for P)
    base                          s, the leaf: the written container is Z(s * 2.0, ...)
    bp, tp | idx (+ key_lens)     the key
    flat                          the non-negative flat storage rows the key names (the reference's own getitem on an iota)
    value, cot                    the value as given (its own shape) and the cotangent of the written storage
    out, grad_base, grad_value    the reference's results
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

import torchrua as ref  # noqa: E402,F401  (the reference; importing it patches Tensor.__getitem__ / __setitem__)
from torchrua import C, L, P, R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'r6_setitem_grad.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
store = {}


def npy(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy().view(np.uint16)
    return t.numpy()


def put(case, name, value):
    store[f'{case}/{name}'] = npy(value) if isinstance(value, torch.Tensor) else np.asarray(value)


def ints(g, shape, lo, hi, dtype):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype)


def build(kind, data, lens):
    """The container of `kind` over the tokens of C(data, lens), made by the reference's own casts."""
    c = C(data=data, token_sizes=lens)
    return {'C': lambda: c, 'L': lambda: c.left(0), 'P': c.pack, 'R': lambda: c.right(0)}[kind]()


def rewrap(z, data):
    return z._replace(data=data)


def case(name, kind, lens, H, dtype_name, form, vshape, unique, seed, m=None):
    g = torch.Generator().manual_seed(seed)
    dtype = DTYPES[dtype_name]
    lens = torch.as_tensor(lens, dtype=torch.long)
    N, B = int(lens.sum()), lens.numel()
    hidden = () if H == 0 else (H,)
    shell = build(kind, ints(g, (N,) + hidden, -4, 4, dtype), lens)
    base = shell.data.detach().clone()
    lead_dims = 2 if kind in 'LR' else 1
    n_rows = int(np.prod(base.shape[:lead_dims]))
    put(name, 'kind', kind)
    put(name, 'dtype', dtype_name)
    put(name, 'form', form)
    put(name, 'unique', int(unique))
    put(name, 'lens', lens)
    put(name, 'base', base)
    if kind == 'P':
        put(name, 'batch_sizes', shell.batch_sizes)
        put(name, 'sorted_indices', shell.sorted_indices)
        put(name, 'unsorted_indices', shell.unsorted_indices)

    # ---- the key
    iota = rewrap(shell, torch.arange(n_rows).reshape(base.shape[:lead_dims]))
    if form in ('pair', 'pair2d'):
        bp_all = torch.repeat_interleave(torch.arange(B), lens)
        tp_all = torch.cat([torch.arange(int(k)) for k in lens]) if N else torch.zeros(0, dtype=torch.long)
        if unique:
            pick = torch.randperm(N, generator=g)[:N if m is None else m]
        else:
            pick = torch.randint(0, N, (N + 3 if m is None else m,), generator=g)
        if form == 'pair2d':
            pick = pick[:pick.numel() // 2 * 2].reshape(2, -1)
        bp, tp = bp_all[pick], tp_all[pick]
        put(name, 'bp', bp)
        put(name, 'tp', tp)
        key = (bp, tp)
        flat = iota[bp, tp]
        lead = tuple(bp.shape)
    else:
        if form == 'mask':
            idx = torch.rand(n_rows, generator=g) < 0.4
            flat = torch.nonzero(idx).reshape(-1)
        else:
            count = (n_rows * 2 // 3) if m is None else m
            if unique:
                idx = torch.randperm(n_rows, generator=g)[:count]
            else:
                idx = torch.randint(0, n_rows, (count + 2,), generator=g)
            if form in ('flat', 'zkeyL'):                       # negative rows wrap, as in torch's own indexing
                neg = torch.rand(idx.shape, generator=g) < 0.4
                idx = torch.where(neg, idx - n_rows, idx)
            if form == 'int32':
                idx = idx.to(torch.int32)
            flat = torch.where(idx < 0, idx + n_rows, idx).long()
        lead = tuple(flat.shape)
        put(name, 'idx', idx)
        key = idx
        if form in ('zkey', 'tensorZ'):
            half = idx.numel() // 2
            key_lens = torch.tensor([half, idx.numel() - half])
            put(name, 'key_lens', key_lens)
            key = C(data=idx, token_sizes=key_lens)
        elif form == 'zkeyL':                                    # a padded container of row indices: a 2-D index
            cols = 3
            idx = idx[:idx.numel() // cols * cols].reshape(-1, cols)
            flat = torch.where(idx < 0, idx + n_rows, idx)
            lead = tuple(idx.shape)
            key_lens = torch.full((idx.size(0),), cols, dtype=torch.long)
            put(name, 'idx', idx)
            put(name, 'key_lens', key_lens)
            key = L(data=idx, token_sizes=key_lens)
    put(name, 'flat', flat)
    if unique:
        assert flat.reshape(-1).unique().numel() == flat.numel(), name

    # ---- value and cotangent: small integers, every partial sum exact in the dtype
    full = lead + hidden
    vs = {'full': full, 'H': hidden, 'M1': lead + (1,) * len(hidden), '0d': ()}[vshape]
    value = ints(g, vs, -9, 9, dtype)
    cot = ints(g, base.shape, -2, 2, dtype)
    if dtype_name == 'bf16':
        bound = 2 * {'full': 1, 'H': int(np.prod(lead)), 'M1': H or 1, '0d': int(np.prod(full))}[vshape]
        assert bound < 256, (name, bound)
    put(name, 'value', value)
    put(name, 'cot', cot)

    # ---- the reference
    s = base.clone().requires_grad_(True)
    v = value.clone().requires_grad_(True)
    z = rewrap(shell, s * 2.0)
    if form == 'tensorZ':
        t = z.raw() if kind in 'LR' else z.data
        t[key] = v                                               # Tensor.__setitem__ as the reference patches it
    else:
        z[key] = v
    out = z.data
    (out * cot).sum().backward()
    assert out.dtype == dtype and s.grad is not None and v.grad is not None, name
    put(name, 'out', out)
    put(name, 'grad_base', s.grad)
    put(name, 'grad_value', v.grad)


def main():
    rng = np.random.RandomState(6)
    seed = 6000
    # (form, value shape, H, dtype, unique): rows of 4 (1-D fp32), 4, 8, 20, 24, 500 and 1 024 bytes
    combos = [
        ('pair', 'full', 5, 'fp32', True), ('pair', 'full', 5, 'fp32', False), ('pair', 'H', 5, 'fp32', False),
        ('pair', 'M1', 6, 'fp32', False), ('pair', '0d', 2, 'fp32', False), ('pair', 'full', 0, 'fp32', True),
        ('pair', 'H', 0, 'fp32', False), ('pair2d', 'full', 3, 'fp64', True), ('pair2d', 'H', 3, 'fp64', False),
        ('pair', 'full', 125, 'fp32', True), ('pair', 'full', 512, 'bf16', True), ('pair', 'H', 12, 'bf16', False),
        ('pair', '0d', 4, 'bf16', False), ('pair', 'M1', 2, 'fp16', False), ('pair', 'full', 2, 'bf16', False),
        ('zkey', 'full', 5, 'fp32', True), ('zkey', 'H', 2, 'fp32', False), ('zkeyL', 'full', 3, 'fp32', False),
        ('flat', 'full', 6, 'fp32', True), ('flat', '0d', 3, 'fp16', False), ('int32', 'full', 5, 'fp32', True),
        ('int32', 'M1', 12, 'bf16', False), ('mask', 'full', 5, 'fp32', True), ('mask', 'H', 4, 'fp64', True),
        ('tensorZ', 'full', 5, 'fp32', True), ('tensorZ', 'H', 125, 'fp32', False),
    ]
    for kind in 'CLPR':
        for form, vshape, H, dtype, unique in combos:
            seed += 1
            lens = rng.randint(1, 7, 6)
            m = None
            if dtype == 'bf16':          # keep every sum below 256
                m = 20 if vshape != '0d' else 12
            case(f'{kind}.{form}.{vshape}.h{H}.{dtype}.{"u" if unique else "r"}', kind, lens, H, dtype, form, vshape,
                 unique, seed, m=m)
    # one batch with an empty sequence, every layout; one key that is empty
    for kind in 'CLPR':
        seed += 1
        case(f'{kind}.empty_seq', kind, [3, 0, 4, 1, 0, 2], 5, 'fp32', 'pair', 'full', True, seed)
        seed += 1
        case(f'{kind}.empty_seq.H', kind, [0, 2, 5, 0, 1], 3, 'fp32', 'pair', 'H', False, seed)
    np.savez_compressed(OUT, **store)
    print(f'{len(set(k.split("/")[0] for k in store))} cases -> {OUT} ({os.path.getsize(OUT)} bytes)')


if __name__ == '__main__':
    main()
