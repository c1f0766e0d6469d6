"""Per-sequence unique_consecutive (rua_segment_runs_heads + the compress plan and move + rua_segment_runs_inverse /
rua_segment_runs_counts): interleaved legs in ONE process on the same tensors.  No speed threshold is set anywhere: this
reports.

    python scripts/unique_probe.py [--reps 7] [--window 0.2] [--small]  > profiles/unique_probe.txt

    values     c.unique_consecutive(), the public call: the heads (the payload read, a byte written per row), the plan over
               them, the ONE read-back of the new lengths, their offset scan, the move of the run heads
    all        the same with return_inverse=True, return_counts=True (one more scan, two small launches)
    heads      the compare launch alone on preallocated tensors
    stock      the spelling that was available before, for a C: torch.unique_consecutive over the concatenated data
               (dim=0 for rows), a border fix — every sequence start is a head whatever its predecessor holds, so the heads
               are rebuilt as a mask with the starts set — data[heads], and segment_sum of the heads for the new lengths
    copy       out.copy_(data): the streaming copy of the whole payload — what reading every row once costs

For a CattedSequence and a PackedSequence (the stock spelling exists for a C only).  Shapes: 262 144 sequences of U(5, 60)
int64 ids from an alphabet of 4 (a CTC-like frame labelling), the north-star raggedness at H = 1 and H = 512 bf16 with
rows drawn from 4 distinct rows, and few but long sequences (the cut geometry).  Every leg is timed over a window of
about --window seconds of work, the legs interleaved inside every repetition: only the ratios inside one run mean
something.  Printed per case: ms per call (median, min .. max over the repetitions) and TB/s of N * H * e (the payload
read once) for the heads.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name)"""
    s = 16 if small else 1
    return [
        ('ids: 262144 x U(5,60) int64, alphabet 4', 262144 // s, 5, 60, (), 'int64'),
        ('north star: 65536 x U(8,512), H=1 bf16', 65536 // s, 8, 512, (1,), 'bfloat16'),
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('cut: 8 x U(100000,200000), H=64 bf16', 8, 100000 // s, 200000 // s, (64,), 'bfloat16'),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.2, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    from compress_probe import timed
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; alphabet 4; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of N*H*e')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, lo, hi, hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden, dtype=np.int64))
        g = torch.Generator(device=dev).manual_seed(0)
        ids = torch.randint(0, 4, (n,), generator=g, device=dev)
        rows = torch.randint(1, 100, (4,) + hidden, generator=g, device=dev).to(dtype)
        rows.view(4, -1)[:, -1] = torch.arange(4, device=dev).to(dtype)       # pairwise different, in the LAST element
        x = rows[ids] if hidden else ids.to(dtype)
        c = ta.with_host_sizes(x, lens)
        starts = torch.zeros(n, dtype=torch.bool, device=dev)
        starts[(torch.cumsum(lens, 0) - lens).to(dev)] = True
        algo = n * h * x.element_size()
        print(f'# {name}: N = {n}, N*H*e = {algo / 1e9:.3f} GB', flush=True)
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            big = M.lay_pack(z) if cont == 'P' else describe(z)
            first = z.unique_consecutive(True, True)
            out = torch.empty_like(x)

            def values():
                return z.unique_consecutive()

            def everything():
                return z.unique_consecutive(return_inverse=True, return_counts=True)

            def heads():
                O.launch_runs_heads(big, z.data, hidden)

            def stock():
                inverse = torch.unique_consecutive(x, dim=0, return_inverse=True)[1]
                head = torch.ones(n, dtype=torch.bool, device=dev)
                head[1:] = inverse[1:] != inverse[:-1]
                head |= starts
                return x[head], ta.segment_sum(head.float(), c.token_sizes).long()

            def copy():
                out.copy_(x)

            legs = [values, everything, heads, stock if cont == 'C' else None, copy]
            v, a, hd, st, cp = timed(legs, args.reps, args.window)
            print(f'  {cont}  values {fmt(v)} | all {fmt(a)} | heads {fmt(hd)} '
                  f'{(algo / hd[0] / 1e9) if hd else float("nan"):6.3f} TB/s | stock {fmt(st)} | copy {fmt(cp)}', flush=True)
            print(f'      values/copy {over(v, cp)}  all/copy {over(a, cp)}  heads/copy {over(hd, cp)}  values/stock {over(v, st)}',
                  flush=True)
            if cont == 'C':
                sv, sl = stock()
                same = torch.equal(first.values.data.view(torch.uint8), sv.contiguous().view(torch.uint8))
                print(f'      fused == stock bit for bit: {same and torch.equal(first.values.token_sizes, sl)}', flush=True)
            del z, big, out, first
        del x, c, ids, starts
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
