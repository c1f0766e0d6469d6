"""The per-sequence cummax (values only / with indices) and logcumsumexp scans (csrc/rua_cumext.hip): interleaved legs in
ONE process on the same tensors.

    python scripts/cumext_probe.py [--reps 7] [--window 0.1] [--small] [--no-padded]  > profiles/cumext_probe.txt

    cummax v     rua_segment_cumextreme, values only              1 read + 1 write of the payload (the cumsum's bytes)
    cummax v+i   values and int64 indices                         + 8 bytes per element written
    lse          rua_segment_logcumsumexp                         1 read + 1 write
    cummax bwd   rua_segment_cumextreme_backward                  reads grad and the indices, writes grad_in
    lse bwd      rua_segment_logcumsumexp_backward                reads grad, x and y, writes grad_in
    cumsum       z.cumsum() on the same container: the yardstick with the same skeleton and the payload's bytes
    copy         out.copy_(data): the streaming copy of 1 read + 1 write of the payload
    copy v+i     the same plus an int64 tensor of the payload's shape written (a fill): the bytes of `cummax v+i`
    padded       the spelling that was available before: z.left(fill_value=-inf), torch.cummax(dim=1), the cast back of
                 the values (C only; it does not exist for a PackedSequence)

Shapes: the north star 65 536 x U(8, 512) with H = 512 bf16, H = 8 (rows of one vector), 1-D, and the cut geometry
8 x U(100 000, 200 000) with H = 64; a CattedSequence and a PackedSequence.  Every leg is timed over a window of about
--window seconds of work, the legs interleaved inside every repetition: only the ratios inside one run mean something.
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
        ('[N, 8] bf16 (16-byte rows): 65536 x U(8,512)', 65536 // s, 8, 512, (8,), 'bfloat16'),
        ('[N] f32 (1-D): 65536 x U(8,512)', 65536 // s, 8, 512, (), 'float32'),
        ('cut: 8 x U(100000,200000), H=64 bf16', 8, 100000 // s, 200000 // s, (64,), 'bfloat16'),
    ]


def payload(n, hidden, dtype, dev, seed):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n,) + hidden, dtype=dtype, device=dev)
    step = 1 << 22
    for a in range(0, n, step):
        out[a:a + step] = torch.randn((min(n, a + step) - a,) + hidden, generator=g, device=dev)
    return out


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call, the callables interleaved inside every repetition; None: it failed."""
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
        try:
            f()
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
    ap.add_argument('--window', type=float, default=0.1, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    ap.add_argument('--no-padded', action='store_true', help='leave the padded torch.cummax spelling out')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _lib as K
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved windows of '
          f'~{args.window} s')

    def fmt(t):
        return f'{"failed":>9s}' if t is None else f'{t[0]:8.4f} ({t[1]:.4f}..{t[2]:.4f})'

    for name, B, lo, hi, hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden))
        x = payload(n, hidden, dtype, dev, 0)
        c = ta.with_host_sizes(x, lens)
        pay = n * h * x.element_size()
        print(f'# {name}: N = {n}, payload {pay / 1e9:.3f} GB, int64 indices {n * h * 8 / 1e9:.3f} GB', flush=True)
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            lay = M.lay_pack(z) if cont == 'P' else describe(z)
            data = z.data
            y, g = torch.empty_like(data), payload(n, hidden, dtype, dev, 3)
            _, idx = O.launch_cumextreme(lay, data, K.MAX, False, hidden, want_values=False)
            lse = O.launch_logcumsumexp(lay, data, False, hidden)

            def cummax_v():
                O.launch_cumextreme(lay, data, K.MAX, False, hidden, want_indices=False)

            def cummax_vi():
                O.launch_cumextreme(lay, data, K.MAX, False, hidden)

            def lse_fwd():
                O.launch_logcumsumexp(lay, data, False, hidden)

            def cummax_bwd():
                O.launch_cumextreme_backward(lay, g, idx, False, hidden)

            def lse_bwd():
                O.launch_logcumsumexp_backward(lay, g, data, lse, False, hidden)

            def cumsum():
                O.launch_cumsum(lay, data, False, hidden, out=y)

            def copy():
                y.copy_(data)

            def copy_vi():
                y.copy_(data)
                torch.empty_like(idx).fill_(1)              # (the allocator hands back the block `cummax v+i` freed)

            def padded():
                l = z.left(fill_value=-math.inf)
                return l._replace(data=torch.cummax(l.data, dim=1)[0]).cat()

            legs = [cummax_v, cummax_vi, lse_fwd, cummax_bwd, lse_bwd, cumsum, copy, copy_vi]
            with_padded = cont == 'C' and not args.no_padded
            res = timed(legs + ([padded] if with_padded else []), args.reps, args.window)
            cv, cvi, lf, cb, lb, cs, cp, cpi = res[:8]
            pd = res[8] if with_padded else None
            print(f'  {cont}  cummax v {fmt(cv)} | v+i {fmt(cvi)} | lse {fmt(lf)} | cummax bwd {fmt(cb)} | lse bwd {fmt(lb)}',
                  flush=True)
            print(f'     cumsum {fmt(cs)} | copy {fmt(cp)} | copy v+i {fmt(cpi)} | padded cummax {fmt(pd)}', flush=True)
            print(f'     TB/s: cummax v {2 * pay / cv[0] / 1e9:.3f}  v+i {(2 * pay + n * h * 8) / cvi[0] / 1e9:.3f}  '
                  f'lse {2 * pay / lf[0] / 1e9:.3f}  cumsum {2 * pay / cs[0] / 1e9:.3f}  copy {2 * pay / cp[0] / 1e9:.3f}',
                  flush=True)
            print(f'     ratios: cummax v/cumsum {cv[0] / cs[0]:.3f}  cummax v/copy {cv[0] / cp[0]:.3f}  '
                  f'v+i/copy v+i {cvi[0] / cpi[0]:.3f}  lse/cumsum {lf[0] / cs[0]:.3f}  lse/copy {lf[0] / cp[0]:.3f}  '
                  f'cumsum/copy {cs[0] / cp[0]:.3f}' + (f'  cummax v/padded {cv[0] / pd[0]:.3f}' if pd else ''), flush=True)
            del z, lay, data, y, g, idx, lse
        del x, c
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
