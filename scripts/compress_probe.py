"""Per-sequence compress (rua_segment_compress_plan + rua_segment_compress_move): interleaved legs in ONE process on the
same tensors.  No speed threshold is set anywhere: this reports.

    python scripts/compress_probe.py [--reps 7] [--window 0.2] [--small]  > profiles/compress_probe.txt

    fwd        c.compress(mask), the public call: the plan (mask read once, 4 bytes written per row), the ONE read-back
               of the new lengths, their offset scan, the move (kept rows read once, written once)
    fwd+bwd    the same with a payload that requires grad, then backward of a cotangent (the expand: reads the kept rows,
               writes every row of the input's storage); float payloads only
    plan/move  the two launches alone on preallocated tensors (no read-back, no allocation)
    stock      the spelling that was available before, for a C: data[mask] (ATen nonzero + index) plus
               segment_sum(mask.float(), sizes).long() for the new lengths (the library's segment_sum takes the float
               types); stock+bwd: its backward (index_put of the cotangent)
    copy       out[:N'].copy_(data[:N']): the streaming copy of the kept bytes — the floor of the move

Keep-rate 0.5 (Bernoulli, seeded), for a CattedSequence and a PackedSequence (the stock spelling exists for a C only), at
the north-star shape, the same lengths with 1-D int64 payloads, and few but long sequences (the cut geometry).  Every leg
is timed over a window of about --window seconds of work, the legs interleaved inside every repetition: only the ratios
inside one run mean something.  Printed per case: ms per call (median, min .. max over the repetitions) and TB/s of
2 * N' * H * e (kept bytes read + written) for the move.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name)"""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('1-D int64: 65536 x U(8,512)', 65536 // s, 8, 512, (), 'int64'),
        ('cut: 8 x U(100000,200000), H=64 bf16', 8, 100000 // s, 200000 // s, (64,), 'bfloat16'),
    ]


def payload(n, hidden, dtype, dev, seed):
    """[n, *hidden] values of `dtype`, drawn on the device in pieces (no fp32 copy of the whole)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n,) + hidden, dtype=dtype, device=dev)
    step = 1 << 22
    for a in range(0, n, step):
        m = min(n, a + step) - a
        if dtype.is_floating_point:
            out[a:a + step] = torch.randn((m,) + hidden, generator=g, device=dev)
        else:
            out[a:a + step] = torch.randint(0, 50000, (m,) + hidden, generator=g, device=dev)
    return out


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call; every window repeats its callable for about `window` seconds, the
    callables interleaved inside every repetition.  None for a leg that is None or fails."""
    import torch

    def once(f, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n

    counts = []
    for f in fns:
        if f is None:
            counts.append(0)
            continue
        try:
            f()                                               # warm-up
            torch.cuda.synchronize()
            counts.append(max(1, min(1000, math.ceil(window * 1e3 / max(once(f, 1), 1e-3)))))
        except Exception as e:
            print(f'#   a leg failed: {type(e).__name__}: {str(e)[:120]}', flush=True)
            counts.append(0)
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            if counts[i]:
                ms[i].append(once(f, counts[i]))
    return [(statistics.median(m), min(m), max(m)) if m else None for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.2, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; keep-rate 0.5; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of 2*N\'*H*e')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, lo, hi, hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden, dtype=np.int64))
        x = payload(n, hidden, dtype, dev, 0)
        mask_c = torch.rand(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1)) < 0.5
        c = ta.with_host_sizes(x, lens)
        n_kept = int(mask_c.sum())
        algo = 2 * n_kept * h * x.element_size()
        print(f'# {name}: N = {n}, N\' = {n_kept}, 2*N\'*H*e = {algo / 1e9:.3f} GB', flush=True)
        is_float = dtype.is_floating_point
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            mask = ta.C(mask_c, c.token_sizes).pack().data if cont == 'P' else mask_c
            big = M.lay_pack(z) if cont == 'P' else describe(z)
            first = z.compress(mask)                              # the result once: its layout for the bare launches
            small = M.lay_pack(first) if cont == 'P' else describe(first)
            rank, _ = O.launch_compress_plan(big, mask)
            out = torch.empty_like(first.data)
            g = payload(n_kept, hidden, dtype, dev, 3) if is_float else None
            leaf = z.data.detach().clone().requires_grad_(True) if is_float else None
            zl = (ta.P(leaf, z.batch_sizes, z.sorted_indices, z.unsorted_indices) if cont == 'P' else
                  ta.C(leaf, z.token_sizes)) if is_float else None

            def fwd():
                return z.compress(mask)

            def fwd_bwd():
                leaf.grad = None
                zl.compress(mask).data.backward(g)

            def plan():
                O.launch_compress_plan(big, mask)

            def move():
                O.launch_compress_move(small, big, rank, z.data, hidden, out.shape, False, out=out)

            def stock():
                return x[mask_c], ta.segment_sum(mask_c.float(), c.token_sizes).long()

            def stock_bwd():
                leaf.grad = None
                leaf[mask_c].backward(g)
                return ta.segment_sum(mask_c.float(), c.token_sizes).long()

            def copy():
                out.copy_(x[:n_kept])

            legs = [fwd, fwd_bwd if is_float else None, plan, move, stock if cont == 'C' else None,
                    stock_bwd if cont == 'C' and is_float else None, copy]
            f_, fb, pl, mv, st, sb, cp = timed(legs, args.reps, args.window)
            print(f'  {cont}  fwd {fmt(f_)} | fwd+bwd {fmt(fb)} | plan {fmt(pl)} | move {fmt(mv)} '
                  f'{algo / mv[0] / 1e9:6.3f} TB/s | stock {fmt(st)} | stock+bwd {fmt(sb)} | copy {fmt(cp)}', flush=True)
            print(f'      fwd/copy {over(f_, cp)}  move/copy {over(mv, cp)}  plan/copy {over(pl, cp)}  fwd/stock {over(f_, st)}  '
                  f'(fwd+bwd)/copy {over(fb, cp)}  (fwd+bwd)/(stock+bwd) {over(fb, sb)}', flush=True)
            if cont == 'C':
                same = torch.equal(first.data.view(torch.uint8), x[mask_c].contiguous().view(torch.uint8))
                print(f'      fused == data[mask] bit for bit: {same}', flush=True)
            del z, mask, big, small, rank, out, g, leaf, zl, first
        del x, c, mask_c
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
