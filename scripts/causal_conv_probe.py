"""The fused per-sequence causal depthwise convolution (rua_segment_causal_conv): interleaved legs in ONE process on
the same tensors.

    python scripts/causal_conv_probe.py [--reps 7] [--window 0.1] [--small] [--no-padded]  > profiles/causal_conv_probe.txt

    fwd      z.causal_conv(w, b)                         one launch: 1 read + 1 write of the payload
    fwd+bwd  the forward, then the fused backward with all three gradients (reads the cotangent and the payload,
             writes grad_input; a small finish adds the [K, H] partial sums): 5 passes over [N, H] in all
    copy     out.copy_(data): the streaming copy of the same bytes — the floor of 1 read + 1 write
    cumsum   z.cumsum(): a member of the family with the same traffic
    padded   the spelling that was available before: z.left(), a transpose to [B, H, T], F.conv1d(groups=H,
             padding=K-1), a slice, a transpose and the cast back to the container

K = 4, with and without a bias, for a CattedSequence and a PackedSequence, at the north-star shape, at rows of one vector
(H = 8) and at few but long sequences (the cut geometry).  Every leg is timed over a window of about --window seconds of
work (the callable repeated; the count is fixed by a calibration call), the legs interleaved inside every repetition:
only the ratios inside one run mean something.  Printed per case: ms per call (median, min .. max over the
repetitions), TB/s of 2 * N * H * e for the forward, and the ratios to the copy and to cumsum.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 4


def shapes(small):
    """(name, sequences, shortest, longest, hidden, dtype name)"""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512), H=512 bf16', 65536 // s, 8, 512, (512,), 'bfloat16'),
        ('[N, 8] bf16 (16-byte rows): 65536 x U(8,512)', 65536 // s, 8, 512, (8,), 'bfloat16'),
        ('cut: 8 x U(100000,200000), H=64 bf16', 8, 100000 // s, 200000 // s, (64,), 'bfloat16'),
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


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call; every window repeats its callable for about `window` seconds, the
    callables interleaved inside every repetition.  A callable that fails is reported as None."""
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
            f()                                               # warm-up
            torch.cuda.synchronize()
            counts.append(max(1, min(1000, math.ceil(window * 1e3 / max(once(f, 1), 1e-3)))))
        except Exception as e:                                # (the padded spelling may not fit, or not exist for a layout)
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
    ap.add_argument('--no-padded', action='store_true', help='leave the padded F.conv1d spelling out')
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import torchrua_amd as ta
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; K = {K}; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of 2*N*H*e')

    def fmt(t):
        return f'{"failed":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    for name, B, lo, hi, hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n, h = int(lens.sum()), int(np.prod(hidden))
        x = payload(n, hidden, dtype, dev, 0)
        w = payload(K, hidden, dtype, dev, 1)
        bias = payload(1, hidden, dtype, dev, 2)[0]
        c = ta.with_host_sizes(x, lens)
        algo = 2 * n * h * x.element_size()
        print(f'# {name}: N = {n}, 2*N*H*e = {algo / 1e9:.3f} GB', flush=True)
        for cont in ('C', 'P'):
            z = c.pack() if cont == 'P' else c
            lay = M.lay_pack(z) if cont == 'P' else describe(z)
            data = z.data
            y, g = torch.empty_like(data), payload(n, hidden, dtype, dev, 3)
            back = (lambda l: l.pack()) if cont == 'P' else (lambda l: l.cat())
            for b in (bias, None):
                def fwd():
                    O.launch_causal_conv(lay, data, w, b, False, hidden, out=y)

                def fwd_bwd():
                    O.launch_causal_conv(lay, data, w, b, False, hidden, out=y)
                    return O.launch_causal_conv_backward(lay, g, data, w, False, hidden, K, True, True, b is not None)

                def copy():
                    y.copy_(data)

                def cumsum():
                    O.launch_cumsum(lay, data, False, hidden, out=y)

                def padded():
                    l = z.left()
                    t = F.conv1d(l.data.transpose(1, 2), w.reshape(K, h).t()[:, None, :], b, padding=K - 1, groups=h)
                    return back(l._replace(data=t[..., :l.data.shape[1]].transpose(1, 2).contiguous()))

                legs = [fwd, fwd_bwd, copy, cumsum] + ([] if args.no_padded else [padded])
                res = timed(legs, args.reps, args.window) + ([None] if args.no_padded else [])
                f_, fb, cp, cs, pd = res
                err = ''
                if pd is not None:
                    fwd()
                    err = f'; fused vs padded: max |diff| {(y.float() - padded().data.float()).abs().max().item():.2e}'
                print(f'  {cont} bias={int(b is not None)}  fwd {fmt(f_)} {algo / f_[0] / 1e9:6.3f} TB/s | fwd+bwd {fmt(fb)} | '
                      f'copy {fmt(cp)} | cumsum {fmt(cs)} | padded {fmt(pd)}', flush=True)
                print(f'      fwd/copy {f_[0] / cp[0]:.3f}  fwd/cumsum {f_[0] / cs[0]:.3f}  cumsum/copy {cs[0] / cp[0]:.3f}  '
                      f'(fwd+bwd)/copy {fb[0] / cp[0]:.3f}' + (f'  fwd/padded {f_[0] / pd[0]:.3f}' if pd else '') + err,
                      flush=True)
            del z, lay, data, y, g
        del x, c
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
