"""The fused per-sequence cumsum (rua_segment_cumsum): an interleaved A/B against the spelling that was available before
it, and its HBM traffic from the PMC counters.

A/B — ONE process, the same tensors, the callables interleaved inside every repetition:

    python scripts/cumsum_probe.py [--reps 12] [--small]  > profiles/cumsum_ab.txt

    fused   z.cumsum()                       one launch: 1 read + 1 write of the payload
    padded  z.left() -> torch.cumsum(dim=1) -> the cast back to the container (cat() / pack()): the library's mover twice
            and ATen's scan over the PADDED [B, T, H] tensor in between
    copy    out.copy_(data): the streaming copy of the same bytes in the same process — the floor of 1 read + 1 write

Per shape, container (C, P) and direction: ms (median, and min .. max, of the interleaved repetitions), TB/s of
2 * N * H * e, and the ratios fused / padded and fused / copy (below 1 = the fused operator is faster).  Box-to-box and
process-to-process spread is 4-6 %: only the interleaved ratios mean something.

PMC — counters in runs of their own, one counter per pass, no tracing; FETCH_SIZE as scripts/pmc_ops.py treats it on
gfx950 (half of a wide read stream is reported: reads are doubled; counter unit KiB), and its marker launches and
`summarize` are reused:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d prof_out/cumsum_fetch -o run -- python3 scripts/cumsum_probe.py pmc
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d prof_out/cumsum_write -o run -- python3 scripts/cumsum_probe.py pmc
    python3 scripts/cumsum_probe.py pmc --time > prof_out/cumsum_time.json      # HIP-event times, no profiler
    python3 scripts/cumsum_probe.py summarize                                   # -> profiles/cumsum_pmc.json

`pmc` runs, per shape and container, the fused forward scan and the fused reverse scan (= the backward of the forward
one): one uncounted warm-up and three counted launches each.  `traffic_over_algorithmic` in the result is
(2 * FETCH_SIZE + WRITE_SIZE) / (2 * N * H * e).
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
    """Per shape and container: (name, container tag, container, lay, hidden, algorithmic bytes)."""
    import numpy as np
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _meta as M
    from torchrua_amd.layout import describe
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
            lay = M.lay_pack(z) if cont == 'P' else describe(z)
            yield name, cont, z, lay, hidden, 2 * n * h * x.element_size()
            del z, lay
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

    from torchrua_amd import _ops as O
    print(f'# {torch.cuda.get_device_name(0)}; median (min .. max) of {reps} interleaved repetitions; TB/s of 2*N*H*e')
    print('# padded: z.left() -> torch.cumsum(dim=1) -> cast back (the spelling before this operator); copy: out.copy_(data)')
    print(f'# {"shape":48s} {"cont":4s} {"dir":3s} {"fused ms":>26s} {"TB/s":>6s} {"padded ms":>26s} {"copy ms":>26s} '
          f'{"fused/padded":>12s} {"fused/copy":>10s}')
    for name, cont, z, lay, hidden, algo in cases(small):
        data = z.data
        y = torch.empty_like(data)
        back = (lambda l: l.pack()) if cont == 'P' else (lambda l: l.cat())

        def copy():
            y.copy_(data)

        for reverse in (False, True):
            def fused():
                O.launch_cumsum(lay, data, reverse, hidden, out=y)

            def padded():
                l = z.rev().left() if reverse else z.left()
                out = back(l._replace(data=torch.cumsum(l.data, dim=1)))
                return out.rev() if reverse else out

            fused()
            err = (y.float() - padded().data.float()).abs().max().item()
            (a, a0, a1), (b, b0, b1), (c, c0, c1) = timed((fused, padded, copy), reps)
            print(f'  {name:48s} {cont:4s} {"rev" if reverse else "fwd":3s} {a:9.4f} ({a0:7.4f}..{a1:7.4f}) '
                  f'{algo / a / 1e9:6.3f} {b:9.4f} ({b0:7.4f}..{b1:7.4f}) {c:9.4f} ({c0:7.4f}..{c1:7.4f}) '
                  f'{a / b:12.3f} {a / c:10.3f}', flush=True)
            print(f'  {"":48s} (fused vs padded: max |diff| {err:.2e})', flush=True)
        del y


def pmc(timed_run, small):
    """Marker-separated groups as scripts/pmc_ops.py cuts them: marker | warm-up | marker | REPS launches | marker."""
    import json

    import pmc_ops
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _ops as O
    dev = torch.device('cuda:0')
    tiny = ta.with_host_sizes(torch.zeros(4, 2, device=dev), torch.tensor([1, 3]))
    order, times = [], {}
    for name, cont, z, lay, hidden, algo in cases(small):
        data = z.data
        y = torch.empty_like(data)
        for direction, fn in (('fwd', lambda: O.launch_cumsum(lay, data, False, hidden, out=y)),
                              ('rev', lambda: O.launch_cumsum(lay, data, True, hidden, out=y))):
            key = f'{name} | {cont} {direction}'
            ta.get_mask(tiny)
            fn()
            torch.cuda.synchronize()
            ta.get_mask(tiny)
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(pmc_ops.REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ta.get_mask(tiny)
            order.append(key)
            times[key] = {'algorithmic_bytes': algo, 'ms_per_call': e0.elapsed_time(e1) / pmc_ops.REPS}
        del y
    torch.cuda.synchronize()
    if timed_run:
        print(json.dumps({'order': order, 'ops': times}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='?', default='ab', choices=('ab', 'pmc', 'summarize'))
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    ap.add_argument('--time', action='store_true', help='pmc: print the HIP-event times and the group order as JSON')
    args = ap.parse_args()
    if args.mode == 'summarize':
        import pmc_ops
        pmc_ops.summarize('cumsum_pmc', 'cumsum')
    elif args.mode == 'pmc':
        pmc(args.time, args.small)
    else:
        ab(args.reps, args.small)


if __name__ == '__main__':
    main()
