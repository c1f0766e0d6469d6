"""The fused per-sequence argmax (rua_segment_argreduce): an interleaved A/B against the library's own reduce_max on the
same container (which reads the same bytes), the padded spelling that was available before it, and the streaming copy.

ONE process, the same tensors, the callables interleaved inside every repetition:

    python scripts/argmax_probe.py [--reps 12] [--small]  > profiles/argmax_probe.txt

    seq_max     z.max(): values and positions, one launch: 1 read of the payload, B*H*(e + 8) bytes out
    argmax      z.argmax(): positions only (values = NULL), B*H*8 bytes out
    reduce_max  ta.reduce_max(z): the segmented reducer (+ its rua_fill_empty), the yardstick: the same bytes in
    padded      z.left(fill_value=-inf) -> .data.argmax(dim=1): the library's mover and ATen's kernel over the PADDED
                [B, T, H] tensor
    copy        out.copy_(data): the streaming copy of the same bytes in the same process (1 read + 1 write)

Per shape and container (C, P): ms (median, and min .. max, of the interleaved repetitions), TB/s of N * H * e read, and
the ratios argmax / reduce_max, seq_max / reduce_max, argmax / padded and argmax / copy (below 1 = the fused operator is
faster).  Box-to-box and process-to-process spread is 4-6 %: only the interleaved ratios mean something.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name).  The first two are the ones the README quotes."""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('[N, 8] bf16 (16-byte rows): 65536 x U(8,512)', 65536 // s, 8, 512, (8,), 'bfloat16'),
        ('1-D fp32: 65536 x U(8,512)', 65536 // s, 8, 512, (), 'float32'),
        ('extra, cut: 8 x U(100000,200000), H=512 bf16', 8, 100000 // s, 200000 // s, (512,), 'bfloat16'),
    ]


def payload(n, hidden, dtype, dev, seed):
    """[n, *hidden] standard normal values of `dtype`, drawn on the device in pieces (no fp32 copy of the whole)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n,) + hidden, dtype=dtype, device=dev)
    step = 1 << 22
    for a in range(0, n, step):
        out[a:a + step] = torch.randn((min(n, a + step) - a,) + hidden, generator=g, device=dev)
    return out


def cases(small):
    """Per shape and container: (name, container tag, container, bytes read)."""
    import numpy as np
    import torch

    import torchrua_amd as ta
    dev = torch.device('cuda:0')
    for name, B, lo, hi, hidden, dtype in shapes(small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n = int(lens.sum())
        x = payload(n, hidden, dtype, dev, 0)
        c = ta.with_host_sizes(x, lens)
        h = 1
        for d in hidden:
            h *= d
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            yield name, cont, z, n * h * x.element_size()
            del z
        del x, c
        torch.cuda.empty_cache()


def timed(fns, reps):
    """Per callable (median, min, max) ms, the callables interleaved inside every repetition."""
    import torch
    for f in fns:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def ab(reps, small):
    import torch

    import torchrua_amd as ta
    print(f'# {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} interleaved repetitions; TB/s of N*H*e read')
    print('# padded: z.left(fill_value=-inf).data.argmax(dim=1); copy: out.copy_(data) (1 read + 1 write)')
    for name, cont, z, algo in cases(small):
        data = z.data
        y = torch.empty_like(data)

        def seq_max():
            return ta.seq_max(z)

        def argmax():
            return ta.argmax(z)

        def reduce_max():
            return ta.reduce_max(z)

        def padded():
            return z.left(fill_value=float('-inf')).data.argmax(dim=1)

        def copy():
            y.copy_(data)

        same = bool(torch.equal(argmax(), padded())) and bool(torch.equal(seq_max().values, reduce_max()))
        labels = ('seq_max', 'argmax', 'reduce_max', 'padded', 'copy')
        res = timed((seq_max, argmax, reduce_max, padded, copy), reps)
        print(f'  {name} | {cont}   (argmax == padded and seq_max.values == reduce_max: {same})', flush=True)
        for label, (m, lo, hi) in zip(labels, res):
            print(f'    {label:10s} {m:9.4f} ms ({lo:8.4f} .. {hi:8.4f})  {algo / m / 1e9:6.3f} TB/s', flush=True)
        t = dict(zip(labels, (r[0] for r in res)))
        print(f'    ratios: argmax/reduce_max {t["argmax"] / t["reduce_max"]:.3f}  seq_max/reduce_max '
              f'{t["seq_max"] / t["reduce_max"]:.3f}  argmax/padded {t["argmax"] / t["padded"]:.3f}  argmax/copy '
              f'{t["argmax"] / t["copy"]:.3f}', flush=True)
        del y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()
    ab(args.reps, args.small)


if __name__ == '__main__':
    main()
