"""attention_decode against the band form of `attention` at decode shapes, bf16, C layouts, host lengths.  Interleaved
legs (every repetition runs every leg of a group once, in turn), HIP events around INNER calls of one leg, medians over
the repetitions of the time per call; repetition 0 warms up.  The lines go to profiles/attention_decode_probe.txt as they
come out; the one condition (below) is printed as `holds` / `DOES NOT HOLD` and is the exit status.

  decode   64 sequences with U(1 024, 8 192) cached keys, 32 query heads over 8 kv heads, D in {64, 128}, T_b in {1, 4}:
             attention_decode          (kv_chunk=None: the plan chooses)
             attention(causal, end)    the same inputs through the flash-style band forward
             copy                      k.data and v.data copied once each (a streaming copy READS and WRITES the bytes)
  long     4 sequences of 32 768 keys, T_b = 1, D = 64: the same three legs — only splitting gives parallelism here.

THE CONDITION: at T_b = 1 the decode median is below the band form's by more than the larger of the two legs' max - min
spread, at both D.  The fraction of the copy's time is reported as it comes out, with no promise.

    python scripts/attention_decode_probe.py [--reps 5] [--inner 20] [--out profiles/attention_decode_probe.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchrua_amd as ta  # noqa: E402

DEV = torch.device('cuda:0')
H, HKV = 32, 8


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def measure(legs, reps, inner):
    """{leg: (median ms per call, min, max)} of interleaved repetitions."""
    times = {name: [] for name in legs}
    for rep in range(reps + 1):
        for name, fn in legs.items():
            t = timed(fn, inner)
            if rep:
                times[name].append(t)
    return {name: (statistics.median(ts), min(ts), max(ts)) for name, ts in times.items()}


def group(lines, tag, klens, T, D, reps, inner):
    """The three legs of one shape; True iff decode beats the band form by more than the larger spread."""
    B = klens.numel()
    cont = lambda lens, heads: ta.with_host_sizes(  # noqa: E731
        torch.randn(int(lens.sum()), heads, D, device=DEV, dtype=torch.bfloat16), lens)
    q, k, v = cont(torch.full((B,), T), H), cont(klens, HKV), cont(klens, HKV)
    kc, vc = torch.empty_like(k.data), torch.empty_like(v.data)
    with torch.no_grad():
        ref = q.attention(k, v, causal=True, align='end').data.float()
        err = (q.attention_decode(k, v).data.float() - ref).abs().max().item()
        got = measure({'decode': lambda: q.attention_decode(k, v),
                       'band': lambda: q.attention(k, v, causal=True, align='end'),
                       'copy': lambda: (kc.copy_(k.data), vc.copy_(v.data))}, reps, inner)
    nbytes = 2 * k.data.numel() * 2
    head = f'{tag} B={B} T={T} D={D} heads={H}/{HKV} keys={int(klens.sum())} K+V={nbytes / 2 ** 20:.0f} MiB'
    for name, s in got.items():
        note = ''
        if name == 'decode':
            note = (f'  {nbytes / s[0] / 1e9:.2f} TB/s of K + V read  band/decode {got["band"][0] / s[0]:.2f}x'
                    f'  copy/decode {got["copy"][0] / s[0]:.3f}  max |decode - band| {err:.3g}')
        lines.append(f'{head} {name}: {s[0]:.4f} ms  (min {s[1]:.4f} max {s[2]:.4f}){note}')
    spread = max(got[n][2] - got[n][1] for n in ('decode', 'band'))
    return got['band'][0] - got['decode'][0] > spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_decode_probe: {torch.cuda.get_device_name(0)}, bf16, C layouts, reps={args.reps}, '
             f'inner={args.inner}, median ms per call']
    klens = torch.randint(1024, 8193, (64,), generator=torch.Generator().manual_seed(1))
    holds = True
    for D in (64, 128):
        for T in (1, 4):
            n = len(lines)
            ok = group(lines, 'decode', klens, T, D, args.reps, args.inner)
            if T == 1:
                holds = holds and ok
                lines.append(f'condition T=1 D={D}: band - decode > larger spread: {"holds" if ok else "DOES NOT HOLD"}')
            print('\n'.join(lines[n:]), flush=True)
            torch.cuda.empty_cache()
    n = len(lines)
    group(lines, 'long', torch.full((4,), 32768), 1, 64, args.reps, args.inner)
    print('\n'.join(lines[n:]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if holds else 1


if __name__ == '__main__':
    sys.exit(main())
