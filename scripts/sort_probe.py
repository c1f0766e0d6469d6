"""Per-sequence stable sort (rua_segment_sort) and reorder (rua_segment_reorder): interleaved legs in ONE process on the
same tensors.  No speed threshold is set anywhere: this reports.

    python scripts/sort_probe.py [--reps 7] [--window 0.2] [--small]  > profiles/sort_probe.txt

    sort       z.sort(), the public call: values and indices
    argsort    z.argsort(): the indices alone
    reorder    z.reorder(indices), the gather through the indices the sort produced (per row for a 1-D payload, per
               element otherwise)
    padded     the stock spelling for a C: z.left(fill_value=inf) + torch.sort(dim=1, stable=True) — a padded copy and a
               sort of B x T elements; the cast back is NOT timed (it flatters the stock spelling); wrong when the payload
               holds inf or NaN
    two-sorts  the other stock spelling, 1-D payloads only: a global stable sort by value, then a global stable sort of
               the sequence ids gathered through it, then the positions rebuilt from the offsets
    copy       out.copy_(x): a streaming copy of the payload's bytes

A CattedSequence with host lengths and a PackedSequence (the stock spellings exist for a C only), at: 262 144 ranking
lists of U(5, 60) items, 1-D f32; the north-star raggedness (65 536 x U(8, 512)) with H = 1 and H = 8, f32; few but
long sequences (the cut geometry of the other probes); and one SKEWED case: 4 096 short sequences and one of 1 000 000
tokens.  Every leg is timed over a window of about --window seconds of work, the legs interleaved inside every
repetition: only the ratios inside one run mean something.  Printed per case: ms per call (median, min .. max).
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, shortest, longest, hidden, one giant sequence of this many tokens or 0)"""
    s = 16 if small else 1
    return [
        ('ranking lists: 262144 x U(5,60), 1-D f32', 262144 // s, 5, 60, (), 0),
        ('north star raggedness: 65536 x U(8,512), H=1 f32', 65536 // s, 8, 512, (1,), 0),
        ('north star raggedness: 65536 x U(8,512), H=8 f32', 65536 // s, 8, 512, (8,), 0),
        ('cut: 8 x U(100000,200000), 1-D f32', 8, 100000 // s, 200000 // s, (), 0),
        ('skew: 4096 x U(8,512) and ONE sequence of 1000000, 1-D f32', 4096 // s, 8, 512, (), 1000000 // s),
    ]


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call; every window repeats its callable for about `window` seconds, the
    callables interleaved inside every repetition.  None for a leg that is None."""
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
        f()                                                   # warm-up; a leg that raises ends the run: nothing more is
        torch.cuda.synchronize()                              # launched on a card after an error
        counts.append(max(1, min(1000, math.ceil(window * 1e3 / max(once(f, 1), 1e-3)))))
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
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, lo, hi, hidden, giant in shapes(args.small):
        rs = np.random.RandomState(0)
        lens_np = rs.randint(lo, hi + 1, B).astype(np.int64)
        if giant:
            lens_np[B // 2] = giant
        lens = torch.from_numpy(lens_np)
        n = int(lens.sum())
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((n,) + hidden, generator=g, device=dev)
        c = ta.with_host_sizes(x, lens)
        print(f'# {name}: N = {n}, payload {x.numel() * 4 / 1e9:.4f} GB, longest {int(lens.max())}', flush=True)
        out = torch.empty_like(x)
        ids = torch.repeat_interleave(torch.arange(B, device=dev), c.token_sizes)
        offsets = torch.cumsum(c.token_sizes, 0) - c.token_sizes
        padded_cells = B * int(lens.max())
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            indices = z.argsort()

            def sort():
                return z.sort()

            def argsort():
                return z.argsort()

            def reorder():
                return z.reorder(indices)

            def padded():
                return torch.sort(c.left(fill_value=float('inf')).data, dim=1, stable=True)

            def two_sorts():
                by_value = torch.sort(x, stable=True)[1]
                by_seq = torch.sort(ids[by_value], stable=True)[1]
                order = by_value[by_seq]
                return x[order], order - offsets[ids]

            def copy():
                out.copy_(x)

            stock_ok = cont == 'C' and padded_cells * max(1, x.numel() // max(n, 1)) <= 2 ** 31
            legs = [sort, argsort, reorder, padded if stock_ok else None,
                    two_sorts if cont == 'C' and not hidden else None, copy]
            so, ar, ro, pa, tw, cp = timed(legs, args.reps, args.window)
            print(f'  {cont}  sort {fmt(so)} | argsort {fmt(ar)} | reorder {fmt(ro)} | padded {fmt(pa)} | two-sorts {fmt(tw)} '
                  f'| copy {fmt(cp)}', flush=True)
            print(f'      sort/copy {over(so, cp)}  sort/padded {over(so, pa)}  sort/two-sorts {over(so, tw)}  '
                  f'argsort/sort {over(ar, so)}  reorder/copy {over(ro, cp)}', flush=True)
            if cont == 'C' and not hidden:
                v, order = two_sorts()
                got = z.sort()
                print(f'      fused == two stable sorts, values and indices: '
                      f'{torch.equal(got.values.data, v) and torch.equal(got.indices.data, order)}', flush=True)
            del z, indices
        del x, c, out, ids, offsets
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
