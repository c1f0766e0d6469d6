"""Per-sequence repeat_interleave (rua_segment_repeat_plan + rua_segment_repeat_move + rua_segment_repeat_sum):
interleaved legs in ONE process on the same tensors.  No speed threshold is set anywhere: this reports.

    python scripts/repeat_probe.py [--reps 7] [--window 0.2] [--small]  > profiles/repeat_probe.txt

    fwd        c.repeat_interleave(counts), the public call: the plan (counts read once, 8 bytes written per row), the
               ONE read-back of the new lengths, their offset scan, the move (every output row read and written once)
    fwd+bwd    the same with a payload that requires grad, then backward of a cotangent (the run sum: reads every row of
               the cotangent once, writes every row of the input's storage); float payloads only
    plan/move/sum  the launches alone on preallocated tensors (no read-back, no allocation)
    stock      the spelling that was available before, for a C: torch.repeat_interleave(data, counts, dim=0) plus
               segment_sum(counts.float(), sizes).long() for the new lengths (the library's segment_sum takes the float
               types); stock+bwd: with its backward
    copy       out.copy_(again): a streaming copy of N' rows each way.  The move reads only the N distinct source rows
               from memory (a run's repeated reads hit cache), so this is an UPPER bound of its traffic and
               move/copy flatters the kernel by up to that difference

Counts U(0, 3) (seeded), for a CattedSequence and a PackedSequence (the stock spelling exists for a C only), at the
north-star shape, the same lengths with 1-D int64 payloads, few but long sequences (the cut geometry), and one SKEWED
case: short sequences of ones with a single count of 100 000 (one workgroup per column chunk walks that sequence in the
move; one thread group sums that run in the backward).  Every leg is timed over a window of about --window seconds of
work, the legs interleaved inside every repetition: only the ratios inside one run mean something.  Printed per case: ms
per call (median, min .. max over the repetitions) and TB/s of 2 * N' * H * e for the move.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name, skewed)"""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16, counts U(0,3)', 65536 // s, 8, 512, (512,), 'bfloat16', False),
        ('1-D int64: 65536 x U(8,512), counts U(0,3)', 65536 // s, 8, 512, (), 'int64', False),
        ('cut: 8 x U(100000,200000), H=64 bf16, counts U(0,3)', 8, 100000 // s, 200000 // s, (64,), 'bfloat16', False),
        ('skew: 4096 x U(8,512), H=64 bf16, counts 1 and ONE count of 100000', 4096 // s, 8, 512, (64,), 'bfloat16', True),
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
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of 2*N\'*H*e')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, lo, hi, hidden, dtype, skewed in shapes(args.small):
        dtype = getattr(torch, dtype)
        rs = np.random.RandomState(0)
        lens = torch.from_numpy(rs.randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden, dtype=np.int64))
        if skewed:
            counts_host = torch.ones(n, dtype=torch.int64)
            counts_host[n // 2] = 100000
        else:
            counts_host = torch.from_numpy(rs.randint(0, 4, n).astype(np.int64))
        x = payload(n, hidden, dtype, dev, 0)
        counts_c = counts_host.to(dev)
        c = ta.with_host_sizes(x, lens)
        n_out = int(counts_host.sum())
        algo = 2 * n_out * h * x.element_size()
        print(f'# {name}: N = {n}, N\' = {n_out}, 2*N\'*H*e = {algo / 1e9:.3f} GB', flush=True)
        is_float = dtype.is_floating_point
        again = payload(n_out, hidden, dtype, dev, 3)             # the copy's source; the cotangent of the float cases
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            counts = ta.C(counts_c, c.token_sizes).pack().data if cont == 'P' else counts_c
            src = M.lay_pack(z) if cont == 'P' else describe(z)
            result = z.repeat_interleave(counts)                  # the result once: its layout for the bare launches
            dst = M.lay_pack(result) if cont == 'P' else describe(result)
            first, _ = O.launch_repeat_plan(src, counts)
            out = result.data                                     # (the bare move writes the result's own buffer again)
            back = torch.empty_like(z.data)
            leaf = z.data.detach().clone().requires_grad_(True) if is_float else None
            zl = (ta.P(leaf, z.batch_sizes, z.sorted_indices, z.unsorted_indices) if cont == 'P' else
                  ta.C(leaf, z.token_sizes)) if is_float else None

            def fwd():
                return z.repeat_interleave(counts)

            def fwd_bwd():
                leaf.grad = None
                zl.repeat_interleave(counts).data.backward(again)

            def plan():
                O.launch_repeat_plan(src, counts)

            def move():
                O.launch_repeat_move(dst, src, first, 0, z.data, hidden, out.shape, out=out)

            def run_sum():
                O.launch_repeat_sum(src, dst, first, counts, 0, again, hidden, back.shape, out=back)

            def stock():
                return (torch.repeat_interleave(x, counts_c, dim=0),
                        ta.segment_sum(counts_c.float(), c.token_sizes).long())

            def stock_bwd():
                leaf.grad = None
                torch.repeat_interleave(leaf, counts_c, dim=0).backward(again)
                return ta.segment_sum(counts_c.float(), c.token_sizes).long()

            def copy():
                out.copy_(again)

            legs = [fwd, fwd_bwd if is_float else None, plan, move, run_sum if is_float else None,
                    stock if cont == 'C' else None, stock_bwd if cont == 'C' and is_float else None, copy]
            f_, fb, pl, mv, sm, st, sb, cp = timed(legs, args.reps, args.window)
            print(f'  {cont}  fwd {fmt(f_)} | fwd+bwd {fmt(fb)} | plan {fmt(pl)} | move {fmt(mv)} '
                  f'{algo / mv[0] / 1e9:6.3f} TB/s | sum {fmt(sm)} | stock {fmt(st)} | stock+bwd {fmt(sb)} | copy {fmt(cp)}',
                  flush=True)
            print(f'      fwd/copy {over(f_, cp)}  move/copy {over(mv, cp)}  sum/copy {over(sm, cp)}  plan/copy {over(pl, cp)}  '
                  f'fwd/stock {over(f_, st)}  (fwd+bwd)/copy {over(fb, cp)}  (fwd+bwd)/(stock+bwd) {over(fb, sb)}', flush=True)
            if cont == 'C':
                move()
                same = torch.equal(out.view(torch.uint8),
                                   torch.repeat_interleave(x, counts_c, dim=0).contiguous().view(torch.uint8))
                print(f'      fused == torch.repeat_interleave bit for bit: {same}', flush=True)
            del z, counts, src, dst, first, out, back, leaf, zl, result
        del x, c, counts_c, again
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
