"""standardize / var_mean against their floors and against the composed spelling, on the GPU.

Legs, interleaved round by round so that clock and cache state drift over all of them alike:
    standardize   z.standardize()                                     the fused operator
    composed      mean, broadcast, sub, square, mean, rsqrt, mul      segment_mean + repeat_interleave + ATen (C only)
    softmax       z.softmax()                                         the same two-walk kernel shape with one exp per element
    copy          dst.copy_(payload)                                  a streaming copy of the payload (read + write)
    var_mean      z.var_mean()                                        the first walk alone: payload in, [B, H] out
    reduce_mean   ta.reduce_mean(z)                                   the same bytes in, [B, H] out: var_mean's floor
forward only and forward + backward (standardize, composed, softmax), at the north-star shape (65 536 sequences of
8 .. 512 tokens, H = 512, bf16; C and P), at 16-byte rows (H = 8, bf16) and at 8 sequences of 100 000 .. 200 000 tokens
(H = 64, bf16: the cut form).

    python scripts/standardize_probe.py [--seqs 65536] [--rounds 7] [--window 0.1]  > profiles/standardize_probe.txt

A sample is one event pair around `reps` back-to-back calls of a leg, `reps` chosen per leg after the warm-up so that
the window lasts about `--window` seconds; the time per call is the window over `reps`.  Prints one line per (shape,
leg): the median over the rounds, and the ratios standardize / composed, / softmax, / copy and var_mean / reduce_mean."""
import argparse
import math
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torchrua_amd as ta  # noqa: E402


def timed(fn, reps=1):
    """ms per call over one window of `reps` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def legs(z, lens_dev):
    """{name: callable} for one container `z`; the composed spelling exists for a CattedSequence only."""
    payload = z.data
    cot = torch.randn(payload.shape, device=payload.device).to(payload.dtype)
    dst = torch.empty_like(payload)

    def wrap(data):
        if isinstance(z, ta.P):
            return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
        return z._replace(data=data)

    def composed(zz):
        x = zz.data
        mean = ta.segment_mean(x, lens_dev)
        dev = x - torch.repeat_interleave(mean, lens_dev, dim=0)
        var = ta.segment_mean(dev * dev, lens_dev)
        return dev * torch.repeat_interleave((var + 1e-5).rsqrt(), lens_dev, dim=0)

    def fwd_bwd(op):
        def run():
            op(wrap(payload.detach().requires_grad_(True))).backward(cot)
        return run

    def no_grad(fn):
        return lambda: torch.no_grad()(fn)()

    table = {
        'standardize fwd': no_grad(lambda: z.standardize()),
        'softmax fwd': no_grad(lambda: z.softmax()),
        'copy': lambda: dst.copy_(payload),
        'var_mean fwd': no_grad(lambda: z.var_mean()),
        'reduce_mean fwd': no_grad(lambda: ta.reduce_mean(z)),
        'standardize fwd+bwd': fwd_bwd(lambda zz: zz.standardize().data),
        'softmax fwd+bwd': fwd_bwd(lambda zz: zz.softmax().data),
    }
    if isinstance(z, ta.C):
        table['composed fwd'] = no_grad(lambda: composed(z))
        table['composed fwd+bwd'] = fwd_bwd(composed)
    return table


def measure(label, z, lens_dev, n, H, args):
    table = legs(z, lens_dev)
    times = {k: [] for k in table}
    reps = {}
    for k, fn in table.items():                  # warm-up, then one call sizes the leg's window
        timed(fn)
        reps[k] = max(1, math.ceil(args.window * 1e3 / timed(fn)))
    for _ in range(args.rounds):
        for k, fn in table.items():
            times[k].append(timed(fn, reps[k]))
    med = {k: statistics.median(ts) for k, ts in times.items()}
    gb = n * H * 2 / 1e9
    for k in table:
        print(f'{label} {k:20s} {med[k]:8.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f}, '
              f'{reps[k]} calls per window)  payload {gb / med[k] * 1e3:7.0f} GB/s')
    line = (f'{label} ratios: standardize/softmax fwd {med["standardize fwd"] / med["softmax fwd"]:.2f}, '
            f'standardize/copy fwd {med["standardize fwd"] / med["copy"]:.2f}, '
            f'standardize/softmax fwd+bwd {med["standardize fwd+bwd"] / med["softmax fwd+bwd"]:.2f}, '
            f'var_mean/reduce_mean {med["var_mean fwd"] / med["reduce_mean fwd"]:.2f}')
    if 'composed fwd' in med:
        line += (f', standardize/composed fwd {med["standardize fwd"] / med["composed fwd"]:.2f}, '
                 f'standardize/composed fwd+bwd {med["standardize fwd+bwd"] / med["composed fwd+bwd"]:.2f}')
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seqs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.1, help='seconds of work per timed window')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    print(f'device {torch.cuda.get_device_name(0)}; bf16; median of {args.rounds} interleaved rounds of one '
          f'~{args.window:g} s window per leg, ms per call')
    shapes = [('north star', torch.from_numpy(rng.randint(8, 513, args.seqs).astype(np.int64)), 512, 'CP'),
              ('16-byte rows', torch.from_numpy(rng.randint(8, 513, args.seqs).astype(np.int64)), 8, 'CP'),
              ('8 long', torch.from_numpy(rng.randint(100000, 200001, 8).astype(np.int64)), 64, 'C')]
    for title, lens, H, kinds in shapes:
        n = int(lens.sum())
        x = (3.0 + torch.randn((n, H), device=dev)).to(torch.bfloat16)
        c = ta.with_host_sizes(x, lens)
        lens_dev = lens.to(dev)
        print(f'{title}: {lens.numel()} sequences of {int(lens.min())} .. {int(lens.max())} tokens, {n} tokens, H = {H}')
        for kind in kinds:
            z = c if kind == 'C' else c.pack()
            measure(f'{title} H={H} {kind}', z, lens_dev, n, H, args)
            del z
        del x, c
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
