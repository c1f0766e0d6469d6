"""The fused per-sequence linear recurrence (rua_segment_linear_scan): an interleaved A/B against the cumsum on the same
container and against a streaming copy of the same bytes, forward and forward + backward, and its HBM traffic from the
PMC counters.

A/B — ONE process, fresh buffers per shape, the legs interleaved inside every repetition:

    python scripts/linear_scan_probe.py [--reps 12] [--small]  > profiles/linear_scan_probe.txt

    tensor  z.linear_scan(a)       one launch: payload + gate read, result written   (3 * N * H * e)
    scalar  z.linear_scan(0.99)    one launch: payload read, result written           (2 * N * H * e, the cumsum's bytes)
    cumsum  z.cumsum()             the yardstick on the same container                (2 * N * H * e)
    copy    out.copy_(data)        the streaming copy of the same bytes: the floor of 1 read + 1 write
and the same four with their backward (fused kernels; the copy leg copies twice): the tensor leg's backward reads the
cotangent, the gate and the saved output and writes both gradients (5 * N * H * e).

Per shape and container (C, P): ms (median, and min .. max, of the interleaved repetitions), TB/s of the leg's own
algorithmic bytes, and the ratios to cumsum and to the copy (below 1 = faster).  Box-to-box and process-to-process
spread is 4-6 %: only the interleaved ratios mean something.

PMC — counters in a process of its own, one counter per pass, no tracing (as scripts/cumsum_probe.py):

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d prof_out/linear_scan_fetch -o run -- python3 scripts/linear_scan_probe.py pmc
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d prof_out/linear_scan_write -o run -- python3 scripts/linear_scan_probe.py pmc

`pmc` runs, per shape and container, the tensor-gate and the scalar-gate forward: one warm-up and three launches each.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'scripts'))


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name).  The first two are the ones the README quotes."""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('[N, 8] bf16 (16-byte rows): 65536 x U(8,512)', 65536 // s, 8, 512, (8,), 'bfloat16'),
        ('1-D fp32: 65536 x U(8,512)', 65536 // s, 8, 512, (), 'float32'),
        ('cut: 8 x U(100000,200000), H=512 bf16', 8, 100000 // s, 200000 // s, (512,), 'bfloat16'),
    ]


def cases(small):
    """Per shape and container: (name, container tag, container, gate container, lay, hidden, N * H * e) — fresh
    buffers per shape."""
    import numpy as np
    import torch

    import torchrua_amd as ta
    from cumsum_probe import payload
    from torchrua_amd import _meta as M
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    for name, B, lo, hi, hidden, dtype in shapes(small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n = int(lens.sum())
        x = payload(n, hidden, dtype, dev, 0)
        a = payload(n, hidden, dtype, dev, 1).mul_(0.02).exp_()             # gates near 1: nothing overflows or decays
        c, ca = ta.with_host_sizes(x, lens), ta.with_host_sizes(a, lens)
        h = 1
        for d in hidden:
            h *= d
        for cont in ('C', 'P'):
            z, za = (c.pack(), ca.pack()) if cont == 'P' else (c, ca)
            lay = M.lay_pack(z) if cont == 'P' else describe(z)
            yield name, cont, z, za, lay, hidden, n * h * x.element_size()
            del z, za, lay
        del x, a, c, ca
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

    from torchrua_amd import _ops as O
    print(f'# {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} interleaved repetitions; TB/s of each leg\'s own bytes')
    print('# legs: tensor = z.linear_scan(a); scalar = z.linear_scan(0.99); cumsum = z.cumsum(); copy = out.copy_(data)')
    for name, cont, z, za, lay, hidden, nhe in cases(small):
        data, gate = z.data, za.data
        y, y2 = torch.empty_like(data), torch.empty_like(data)
        cot = torch.empty_like(data).normal_()
        fwd = (('tensor', 3, lambda: O.launch_linear_scan(lay, data, gate, False, hidden, out=y)),
               ('scalar', 2, lambda: O.launch_linear_scan(lay, data, 0.99, False, hidden, out=y)),
               ('cumsum', 2, lambda: O.launch_cumsum(lay, data, False, hidden, out=y)),
               ('copy', 2, lambda: y.copy_(data)))

        def both_tensor():
            O.launch_linear_scan(lay, data, gate, False, hidden, out=y)
            O.launch_linear_scan_backward(lay, cot, gate, y, False, hidden)

        def both_scalar():
            O.launch_linear_scan(lay, data, 0.99, False, hidden, out=y)
            O.launch_linear_scan_backward(lay, cot, 0.99, None, False, hidden)

        def both_cumsum():
            O.launch_cumsum(lay, data, False, hidden, out=y)
            O.launch_cumsum(lay, cot, True, hidden, out=y2)

        def both_copy():
            y.copy_(data)
            y2.copy_(cot)
        bwd = (('tensor', 3 + 5, both_tensor), ('scalar', 4, both_scalar), ('cumsum', 4, both_cumsum), ('copy', 4, both_copy))
        for what, legs in (('fwd', fwd), ('fwd+bwd', bwd)):
            res = timed([f for _, _, f in legs], reps)
            cs, cp = res[2][0], res[3][0]
            for (leg, mult, _), (m, lo, hi) in zip(legs, res):
                print(f'  {name:48s} {cont:2s} {what:8s} {leg:7s} {m:9.4f} ms ({lo:7.4f}..{hi:7.4f})  {mult * nhe / m / 1e9:6.3f} TB/s'
                      f'  / cumsum {m / cs:6.3f}  / copy {m / cp:6.3f}', flush=True)
        del y, y2, cot


def pmc(small):
    """Marker-separated groups as scripts/pmc_ops.py cuts them: marker | warm-up | marker | REPS launches | marker."""
    import pmc_ops
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _ops as O
    dev = torch.device('cuda:0')
    tiny = ta.with_host_sizes(torch.zeros(4, 2, device=dev), torch.tensor([1, 3]))
    for name, cont, z, za, lay, hidden, nhe in cases(small):
        data, gate = z.data, za.data
        y = torch.empty_like(data)
        for fn in (lambda: O.launch_linear_scan(lay, data, gate, False, hidden, out=y),
                   lambda: O.launch_linear_scan(lay, data, 0.99, False, hidden, out=y)):
            ta.get_mask(tiny)
            fn()
            torch.cuda.synchronize()
            ta.get_mask(tiny)
            for _ in range(pmc_ops.REPS):
                fn()
            torch.cuda.synchronize()
            ta.get_mask(tiny)
        del y
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='?', default='ab', choices=('ab', 'pmc'))
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()
    if args.mode == 'pmc':
        pmc(args.small)
    else:
        ab(args.reps, args.small)


if __name__ == '__main__':
    main()
