"""The fused per-sequence softmax (rua_segment_softmax / rua_segment_softmax_backward): an interleaved A/B against what
the library offered before it, and its HBM traffic from the PMC counters.

A/B — ONE process, the same tensors, the callables interleaved inside every repetition:

    python scripts/softmax_probe.py [--reps 20] [--small]  > profiles/softmax_ab.txt

    forward   fused  vs  reduce_logsumexp (one launch, no `initial` tracking) followed by the logsumexp BACKWARD kernel
              driven with a cotangent of ones: g * exp(x - lse) is the softmax.  Two launches of the library's own
              kernels, 3 * N * H * e bytes: a library-to-library comparison.
    backward  fused  vs  an ATEN-ASSISTED composition: t = g * y (ATen), per-sequence sum (the reducer), its broadcast
              (the reducer's backward), y * (g - s) (ATen), with [N, H] temporaries.  The library had no softmax
              backward of its own; this is what a caller would have written, NOT a library-to-library comparison.

Per shape, container (C, P) and direction: ms (median of the interleaved repetitions), TB/s of 2 * N * H * e, and the
ratio fused / composition (below 1 = the fused operator is faster).  Box-to-box and process-to-process spread is
4-6 %: only the interleaved ratio means something.  The four shapes of the merge condition come first;
the `extra` rows (the streaming form, the cut form) are there for DESIGN 3.2a.

PMC — counters in runs of their own, one counter per pass, no tracing; FETCH_SIZE as scripts/pmc_ops.py treats it on
gfx950 (half of a wide read stream is reported: reads are doubled; counter unit KiB), and its marker launches and
`summarize` are reused:

    rocprofv3 --pmc FETCH_SIZE --output-format csv -d prof_out/softmax_fetch -o run -- python3 scripts/softmax_probe.py pmc
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d prof_out/softmax_write -o run -- python3 scripts/softmax_probe.py pmc
    python3 scripts/softmax_probe.py pmc --time > prof_out/softmax_time.json     # HIP-event times, no profiler
    python3 scripts/softmax_probe.py summarize                                   # -> profiles/softmax_pmc.json

`pmc` runs, per shape and container, the fused forward and the fused backward: one uncounted warm-up and three counted
launches each.  `traffic_over_algorithmic` in the result is (2 * FETCH_SIZE + WRITE_SIZE) / (2 * N * H * e) for the
forward and / (3 * N * H * e) for the backward (which reads y and g).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, 'scripts'))


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name).  The first four are the merge condition's."""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('cfg3: 16384 x U(1,64), H=512 bf16', 16384 // s, 1, 64, (512,), 'bfloat16'),
        ('1-D scores: 65536 x U(8,512), fp32', 65536 // s, 8, 512, (), 'float32'),
        ('[N, 16] bf16: 65536 x U(8,512)', 65536 // s, 8, 512, (16,), 'bfloat16'),
        ('extra, streaming: 2048 x U(1024,4096), H=512 bf16', 2048 // s, 1024, 4096, (512,), 'bfloat16'),
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
    """Per shape and container: (name, container tag, lay, data, cotangent, hidden, algorithmic forward bytes)."""
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
            cot = payload(n, hidden, dtype, dev, 1)
            yield name, cont, lay, z.data, cot, hidden, 2 * n * h * x.element_size()
            del z, lay, cot
        del x, c
        torch.cuda.empty_cache()


def timed(fns, reps):
    """Median ms of every callable, the callables interleaved inside every repetition."""
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
    return [statistics.median(m) for m in ms]


def ab(reps, small):
    import torch

    from torchrua_amd import _lib as K
    from torchrua_amd import _ops as O
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; median of {reps} interleaved repetitions; TB/s of 2*N*H*e')
    print('# fwd: against reduce_logsumexp + the logsumexp backward kernel under a cotangent of ones (the library alone)')
    print('# bwd: against an ATen-assisted composition (g*y and y*(g-s) are ATen kernels with [N, H] temporaries)')
    print(f'# {"shape":50s} {"cont":4s} {"dir":3s} {"fused ms":>9s} {"TB/s":>6s} {"comp ms":>9s} {"TB/s":>6s} '
          f'{"fused/comp":>10s}  composition')
    for name, cont, lay, data, cot, hidden, algo in cases(small):
        ones = torch.ones((lay.B,) + hidden, dtype=data.dtype, device=dev)
        y = torch.empty_like(data)
        gx = torch.empty_like(data)

        def fused_fwd():
            O.launch_softmax(lay, data, False, hidden, out=y)

        def comp_fwd():
            lse = O.launch_reduce(lay, data, K.LOGSUMEXP, hidden=hidden, reference_initial=False)
            return O._ReduceBwd.apply(ones, data, lse, lay, K.LOGSUMEXP, None)

        def fused_bwd():
            O.launch_softmax_backward(lay, y, cot, False, hidden, out=gx)

        def comp_bwd():
            s = O.launch_reduce(lay, cot * y, K.SUM, hidden=hidden)
            return y * (cot - O._ReduceBwd.apply(s, y, s, lay, K.SUM, None))

        fused_fwd()
        err = (y.float() - comp_fwd().float()).abs().max().item()
        for direction, pair, what in (('fwd', (fused_fwd, comp_fwd), 'library alone'),
                                      ('bwd', (fused_bwd, comp_bwd), 'ATen-assisted')):
            a, b = timed(pair, reps)
            print(f'  {name:50s} {cont:4s} {direction:3s} {a:9.4f} {algo / a / 1e9:6.3f} {b:9.4f} {algo / b / 1e9:6.3f} '
                  f'{a / b:10.3f}  {what}', flush=True)
        print(f'  {"":50s} (fused vs composition, forward: max |diff| {err:.2e})', flush=True)
        del ones, y, gx


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
    for name, cont, lay, data, cot, hidden, algo in cases(small):
        y = torch.empty_like(data)
        gx = torch.empty_like(data)
        for direction, nbytes, fn in (
                ('fwd', algo, lambda: O.launch_softmax(lay, data, False, hidden, out=y)),
                ('bwd', algo // 2 * 3, lambda: O.launch_softmax_backward(lay, y, cot, False, hidden, out=gx))):
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
            times[key] = {'algorithmic_bytes': nbytes, 'ms_per_call': e0.elapsed_time(e1) / pmc_ops.REPS}
        del y, gx
    torch.cuda.synchronize()
    if timed_run:
        print(json.dumps({'order': order, 'ops': times}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', nargs='?', default='ab', choices=('ab', 'pmc', 'summarize'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    ap.add_argument('--time', action='store_true', help='pmc: print the HIP-event times and the group order as JSON')
    args = ap.parse_args()
    if args.mode == 'summarize':
        import pmc_ops
        pmc_ops.summarize('softmax_pmc', 'softmax')
    elif args.mode == 'pmc':
        pmc(args.time, args.small)
    else:
        ab(args.reps, args.small)


if __name__ == '__main__':
    main()
