"""Per-sequence sliding-window pooling (rua_window_lens + rua_segment_window_pool / rua_segment_window_spread): interleaved
legs in ONE process on the same tensors.  No speed threshold is set anywhere: this reports, the legs that lose included.

    python scripts/window_probe.py [--reps 7] [--window 0.2] [--small]  > profiles/window_probe.txt

    pool       z.window_pool(K, S, mode), the public call with host lengths: the length launch, the host formula, the
               result's offsets / PackedSequence metadata, the ONE pooling launch
    kernel     the pooling launch alone on a prebuilt plan (O.launch_window_pool)
    fwd+bwd    the public call under autograd and the backward of a ones cotangent (the spread launch)
    padded     the spelling that was available before, for a C: left(), transpose to [B, H, T], F.max_pool1d /
               F.avg_pool1d(ceil_mode=True, count_include_pad=False), transpose, the hand-computed new lengths, and the
               cast back to a C (its windows at a sequence's end read the padding: the values differ there)
    copy       a streaming copy of the bytes the pool reads plus the bytes it writes (one out.copy_ of that many bytes)

For a CattedSequence and a PackedSequence (the padded spelling exists for a C only), mode max and mean, (K, S) = (2, 2)
and (3, 2), ceil mode.  Shapes: the north-star raggedness at H = 512 bf16, H = 8 bf16 and 1-D fp32, and few but long
sequences (the cut geometry).  Every leg is timed over a window of about --window seconds of work, the legs interleaved
inside every repetition: only the ratios inside one run mean something.  Printed per case: ms per call (median,
min .. max over the repetitions) and TB/s of (N + N') * H * e for the kernel.
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
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('north star: 65536 x U(8,512), H=8 bf16', 65536 // s, 8, 512, (8,), 'bfloat16'),
        ('north star: 65536 x U(8,512), 1-D fp32', 65536 // s, 8, 512, (), 'float32'),
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
    import torch.nn.functional as F

    import torchrua_amd as ta
    from compress_probe import timed
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.core import result_like
    from torchrua_amd.layout import lay_hidden
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ceil mode; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of (N + N\')*H*e')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, lo, hi, hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden, dtype=np.int64))
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn((n,) + hidden, generator=g, device=dev).to(dtype)
        c = ta.with_host_sizes(x, lens)
        print(f'# {name}: N = {n}', flush=True)
        for k, s in ((2, 2), (3, 2)):
            for mode in ('max', 'mean'):
                for cont in ('C', 'P'):
                    z = c.pack() if cont == 'P' else c
                    first = z.window_pool(k, s, mode, True)
                    n_new = int(first.data.shape[0])
                    algo = (n + n_new) * h * x.element_size()
                    big, _ = lay_hidden(z)
                    plan = None
                    if cont == 'C':
                        small, shape, _ = result_like(type(z), first.token_sizes, B, hidden, x)
                        plan = O.WindowPlan(small, big, hidden, shape, tuple(x.shape), k, s)
                    m1 = (torch.clamp(lens - k, min=0) + s - 1) // s
                    new_host = torch.where(m1 * s >= lens, m1, m1 + 1)        # the hand-computed lengths of the spelling
                    new_dev = new_host.to(dev)
                    M.attach_host(new_dev, new_host)
                    both = torch.empty(algo // 2, dtype=torch.uint8, device=dev)
                    both_out = torch.empty_like(both)
                    leaf = z.data.detach().clone().requires_grad_()
                    zl = z._replace(data=leaf)

                    def pool():
                        return z.window_pool(k, s, mode, True)

                    def kernel():
                        O.launch_window_pool(plan, z.data, O.WINDOW_MODES[mode], want_arg=False)

                    def fwd_bwd():
                        leaf.grad = None
                        zl.window_pool(k, s, mode, True).data.sum().backward()

                    def padded():
                        left = c.left()
                        t = left.data.reshape(B, left.data.shape[1], h).transpose(1, 2)
                        if mode == 'max':
                            y = F.max_pool1d(t, k, s, ceil_mode=True)
                        else:
                            y = F.avg_pool1d(t, k, s, ceil_mode=True, count_include_pad=False)
                        y = y.transpose(1, 2).reshape((B, y.shape[2]) + hidden).contiguous()
                        return ta.L(y, new_dev).cat()

                    def copy():
                        both_out.copy_(both)

                    legs = [pool, kernel if cont == 'C' else None, fwd_bwd, padded if cont == 'C' else None, copy]
                    p, kn, fb, pd, cp = timed(legs, args.reps, args.window)
                    print(f'  K={k} S={s} {mode:4s} {cont}  pool {fmt(p)} | kernel {fmt(kn)} '
                          f'{(algo / kn[0] / 1e9) if kn else float("nan"):6.3f} TB/s | fwd+bwd {fmt(fb)} | padded {fmt(pd)} '
                          f'| copy {fmt(cp)}', flush=True)
                    print(f'      pool/copy {over(p, cp)}  kernel/copy {over(kn, cp)}  fwd+bwd/copy {over(fb, cp)}  '
                          f'pool/padded {over(p, pd)}', flush=True)
                    del z, first, both, both_out, leaf, zl, plan, big
                    torch.cuda.empty_cache()
        del x, c
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
