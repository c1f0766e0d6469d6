"""Per-sequence self-attention over C and P against the padded spelling (left() + masked scaled_dot_product_attention),
forward and forward + backward, bf16, heads = 8, D = 64 and 128, at 65 536 x U(8, 512) tokens and 256 x U(200, 1 600).
Interleaved legs (every repetition runs every leg once, in turn), HIP events, medians.  A batch that does not fit the
device with its gradients is halved until it does, and the line says so; the padded leg runs wherever it fits.
FLOPs are the algorithm's: 4 heads D sum_b T_b^2 for the forward, 2.5 x that for the backward, halved under `causal`
(not used here).  No threshold is set: the lines go to profiles/attention_probe.txt as they come out.

    python scripts/attention_probe.py [--reps 5] [--out profiles/attention_probe.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchrua_amd as ta  # noqa: E402

DEV = torch.device('cuda:0')
HEADS = 8


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def legs_of(lens, D):
    n = int(lens.sum())
    x = torch.randn(n, HEADS, D, device=DEV, dtype=torch.bfloat16).requires_grad_()
    g = torch.randn(n, HEADS, D, device=DEV, dtype=torch.bfloat16)
    c = ta.with_host_sizes(x, lens)
    p = c.pack()
    xp = p.data.detach().requires_grad_()
    p = ta.P(xp, p.batch_sizes, p.sorted_indices, p.unsorted_indices)
    gp = ta.with_host_sizes(g, lens).pack().data

    def fwd(z):
        with torch.no_grad():
            z.attention(z, z)

    def both(z, leaf, cot):
        leaf.grad = None
        z.attention(z, z).data.backward(cot)

    legs = {'C fwd': lambda: fwd(c), 'P fwd': lambda: fwd(p), 'C fwd+bwd': lambda: both(c, x, g),
            'P fwd+bwd': lambda: both(p, xp, gp)}
    B, t_max = lens.numel(), int(lens.max())
    free = torch.cuda.mem_get_info(DEV)[0]
    if 10 * B * t_max * HEADS * D * 2 + 2 * B * HEADS * t_max * t_max < free:        # the padded tensors, their gradients, the mask
        mask = (torch.arange(t_max, device=DEV) < lens.to(DEV)[:, None])[:, None, None, :]

        def padded(grad):
            leaf = x.detach().requires_grad_(grad)
            pad = ta.with_host_sizes(leaf, lens).left(0).data.transpose(1, 2)
            out = F.scaled_dot_product_attention(pad, pad, pad, attn_mask=mask)
            if grad:
                out.backward(out.detach())

        legs['padded fwd'] = lambda: torch.no_grad()(padded)(False)
        legs['padded fwd+bwd'] = lambda: padded(True)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_probe: {torch.cuda.get_device_name(0)}, bf16, heads={HEADS}, self-attention, reps={args.reps}, median ms']
    gen = torch.Generator().manual_seed(0)
    for B, lo, hi in ((65536, 8, 512), (256, 200, 1600)):
        for D in (64, 128):
            lens = torch.randint(lo, hi + 1, (B,), generator=gen)
            while 8 * int(lens.sum()) * HEADS * D * 2 > 0.8 * torch.cuda.mem_get_info(DEV)[0]:
                lens = lens[:lens.numel() // 2]
            flops = 4.0 * HEADS * D * float((lens.double() ** 2).sum())
            legs = legs_of(lens, D)
            times = {k: [] for k in legs}
            for rep in range(args.reps + 1):
                for k, fn in list(legs.items()):
                    try:
                        t = timed(fn)
                    except torch.OutOfMemoryError:               # (the padded leg's temporaries): the leg is dropped
                        lines.append(f'B={lens.numel()} U({lo},{hi}) D={D} {k}: does not fit the device')
                        del legs[k], times[k]
                        torch.cuda.empty_cache()
                        continue
                    if rep:                                      # repetition 0 warms every leg up
                        times[k].append(t)
            for k, ts in times.items():
                ms = statistics.median(ts)
                work = flops * (3.5 if 'bwd' in k else 1.0)
                lines.append(f'B={lens.numel()} (asked {B}) U({lo},{hi}) tokens={int(lens.sum())} D={D} {k}: {ms:.3f} ms  '
                             f'{work / ms / 1e9:.1f} TFLOP/s of useful work  (min {min(ts):.3f} max {max(ts):.3f})')
            print('\n'.join(lines[-len(times):]), flush=True)
            del legs, times
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
