"""softmax_pool against its floor and against the composed spelling, on the GPU.

Legs, interleaved round by round so that clock and cache state drift over all of them alike:
    pool        z.softmax_pool(s)                                   the fused operator
    reduce_sum  ta.reduce_sum(z)                                    same payload bytes in, [B, H] out: the floor
    composed    reduce_sum(z * broadcast(s.softmax()))              the library's own softmax + ATen multiply + reduce_sum
    copy        dst.copy_(payload)                                  a streaming copy of the payload (read + write)
each forward only and forward + backward (pool, reduce_sum, composed), at the north-star shape (65 536 sequences of
8 .. 512 tokens, H = 512, bf16; C and P; G = 1 and G = 8) and at 16-byte rows (H = 8, bf16).

    python scripts/pool_probe.py [--seqs 65536] [--rounds 7] [--window 0.1]  > profiles/pool_probe.txt

A sample is one event pair around `reps` back-to-back calls of a leg, `reps` chosen per leg after the warm-up so that
the window lasts about `--window` seconds; the time per call is the window over `reps`.  Prints one line per (shape,
leg): the median over the rounds, and the ratios pool / reduce_sum and pool / composed."""
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


def legs(z, s, G, hidden):
    """{name: callable} for one container `z` with scores `s` (same container type)."""
    H = int(np.prod(hidden))
    payload = z.data
    cot = torch.randn((s_batch(z),) + hidden, device=payload.device).to(payload.dtype)
    dst = torch.empty_like(payload)

    def wrap(data):
        if isinstance(z, ta.P):
            return ta.P(data, z.batch_sizes, z.sorted_indices, z.unsorted_indices)
        return z._replace(data=data)

    def composed(zz, ss):
        w = ss.softmax().data
        wide = (w.reshape(w.shape[0], G, 1) * zz.data.reshape(w.shape[0], G, H // G)).reshape(zz.data.shape)
        return ta.reduce_sum(wrap(wide))

    def fwd_bwd(op):
        def run():
            vd = payload.detach().requires_grad_(True)
            sd = s.data.detach().requires_grad_(True)
            op(wrap(vd), wrap(sd)).backward(cot)
        return run

    return {
        'pool fwd': lambda: torch.no_grad()(lambda: z.softmax_pool(s))(),
        'reduce_sum fwd': lambda: torch.no_grad()(lambda: ta.reduce_sum(z))(),
        'composed fwd': lambda: torch.no_grad()(lambda: composed(z, s))(),
        'copy': lambda: dst.copy_(payload),
        'pool fwd+bwd': fwd_bwd(lambda zz, ss: zz.softmax_pool(ss)),
        'reduce_sum fwd+bwd': fwd_bwd(lambda zz, ss: ta.reduce_sum(zz)),
        'composed fwd+bwd': fwd_bwd(composed),
    }


def s_batch(z):
    return int(z.batch_sizes[0]) if isinstance(z, ta.P) else int(z.token_sizes.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seqs', type=int, default=65536)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.1, help='seconds of work per timed window')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(0)
    lens = torch.from_numpy(rng.randint(8, 513, args.seqs).astype(np.int64))
    n = int(lens.sum())
    print(f'device {torch.cuda.get_device_name(0)}; {args.seqs} sequences of 8 .. 512 tokens, {n} tokens, bf16; '
          f'median of {args.rounds} interleaved rounds of one ~{args.window:g} s window per leg, ms per call')
    for hidden, G in (((512,), 1), ((8, 64), 8), ((8,), 1)):
        H = int(np.prod(hidden))
        v = torch.randn((n,) + hidden, device=dev, dtype=torch.bfloat16)
        sc = torch.randn((n,) + hidden[:len(hidden) - 1] if G > 1 else (n,), device=dev, dtype=torch.bfloat16)
        c, cs = ta.with_host_sizes(v, lens), ta.with_host_sizes(sc, lens)
        for kind, z, s in (('C', c, cs), ('P', c.pack(), cs.pack())):
            table = legs(z, s, G, hidden)
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
                print(f'H={H} G={G} {kind} {k:20s} {med[k]:8.3f} ms  (min {min(times[k]):.3f}, max {max(times[k]):.3f}, '
                      f'{reps[k]} calls per window)'
                      f'  payload {gb / med[k] * 1e3:7.0f} GB/s')
            print(f'H={H} G={G} {kind} ratios: pool/reduce_sum fwd {med["pool fwd"] / med["reduce_sum fwd"]:.2f}, '
                  f'pool/composed fwd {med["pool fwd"] / med["composed fwd"]:.2f}, '
                  f'pool/reduce_sum fwd+bwd {med["pool fwd+bwd"] / med["reduce_sum fwd+bwd"]:.2f}, '
                  f'pool/composed fwd+bwd {med["pool fwd+bwd"] / med["composed fwd+bwd"]:.2f}')
            del table, z, s
        del v, sc, c, cs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
