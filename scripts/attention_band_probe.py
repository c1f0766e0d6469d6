"""The band form of per-sequence attention (grouped-query heads, windows, end-aligned masks), bf16, D = 64, C layout.
Interleaved legs (every repetition runs every leg of a group once, in turn), HIP events, medians; repetition 0 warms up.
No threshold is set: the lines go to profiles/attention_band_probe.txt as they come out.

  1. window   64 sequences of 8 192 tokens, causal self-attention, heads 8, window in {127, 1 023, None}, forward and
              forward + backward.  The ratio of a windowed leg to the unwindowed one is the evidence that tiles are
              skipped; it is printed next to (W + 128) / (T / 2), the keys a block of 128 queries visits over the keys
              the causal walk visits on average.
  2. gqa      32 query heads over 8 kv heads at 256 x U(200, 1 600), forward and forward + backward, against the same
              operator over repeat_interleave'd K / V (the only spelling without grouped heads).
  3. chunk    T = 128 new queries against S = U(1 024, 8 192) keys, align='end', causal, forward only, 64 sequences,
              32 query heads over 8 kv heads.

    python scripts/attention_band_probe.py [--reps 5] [--out profiles/attention_band_probe.txt]
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
D = 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cont(lens, heads, grad=False):
    x = torch.randn(int(lens.sum()), heads, D, device=DEV, dtype=torch.bfloat16).requires_grad_(grad)
    return ta.with_host_sizes(x, lens)


def fwd(q, k, v, **kw):
    def leg():
        with torch.no_grad():
            q.attention(k, v, **kw)
    return leg


def both(q, k, v, cot, **kw):
    def leg():
        for z in (q, k, v):
            z.data.grad = None
        q.attention(k, v, **kw).data.backward(cot)
    return leg


def measure(legs, reps):
    """{leg: (median ms, min, max)} of interleaved repetitions."""
    times = {name: [] for name in legs}
    for rep in range(reps + 1):
        for name, fn in legs.items():
            t = timed(fn)
            if rep:
                times[name].append(t)
    return {name: (statistics.median(ts), min(ts), max(ts)) for name, ts in times.items()}


def line(group, name, stat, note=''):
    return f'{group} {name}: {stat[0]:.3f} ms  (min {stat[1]:.3f} max {stat[2]:.3f}){note}'


def window_legs(lines, reps):
    B, T, H = 64, 8192, 8
    lens = torch.full((B,), T)
    x, cot = cont(lens, H, True), cont(lens, H).data
    legs = {}
    for w in (127, 1023, None):
        legs[f'window={w} fwd'] = fwd(x, x, x, causal=True, window=w)
        legs[f'window={w} fwd+bwd'] = both(x, x, x, cot, causal=True, window=w)
    got = measure(legs, reps)
    for name, stat in got.items():
        w, kind = name.split()[0][7:], name.split()[1]
        note = ''
        if w != 'None':
            note = (f'  ratio to window=None {stat[0] / got[f"window=None {kind}"][0]:.4f}'
                    f'  (W + 128) / (T / 2) = {(int(w) + 1 + 128) / (T / 2):.4f}')
        lines.append(line(f'window B={B} T={T} heads={H} causal', name, stat, note))


def gqa_legs(lines, reps):
    B, H, HKV = 256, 32, 8
    lens = torch.randint(200, 1601, (B,), generator=torch.Generator().manual_seed(0))
    q, k, v, cot = cont(lens, H, True), cont(lens, HKV, True), cont(lens, HKV, True), cont(lens, H).data
    # the expanded K / V are leaves of their own: the spelling's repeat_interleave and the sum back are NOT timed
    ke, ve = (ta.with_host_sizes(z.data.detach().repeat_interleave(H // HKV, 1).requires_grad_(), lens) for z in (k, v))
    got = measure({'grouped fwd': fwd(q, k, v), 'expanded fwd': fwd(q, ke, ve), 'grouped fwd+bwd': both(q, k, v, cot),
                   'expanded fwd+bwd': both(q, ke, ve, cot)}, reps)
    for name, stat in got.items():
        note = ''
        if name.startswith('grouped'):
            note = f'  ratio to expanded {stat[0] / got["expanded" + name[7:]][0]:.4f}'
        lines.append(line(f'gqa B={B} U(200,1600) tokens={int(lens.sum())} heads={H}/{HKV}', name, stat, note))


def chunk_legs(lines, reps):
    B, T, H, HKV = 64, 128, 32, 8
    klens = torch.randint(1024, 8193, (B,), generator=torch.Generator().manual_seed(1))
    q, k, v = cont(torch.full((B,), T), H), cont(klens, HKV), cont(klens, HKV)
    got = measure({'fwd': fwd(q, k, v, causal=True, align='end')}, reps)
    flops = 4.0 * H * D * T * float(klens.sum())
    lines.append(line(f'chunk B={B} T={T} S=U(1024,8192) keys={int(klens.sum())} heads={H}/{HKV} end causal', 'fwd', got['fwd'],
                      f'  {flops / got["fwd"][0] / 1e9:.1f} TFLOP/s of useful work'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_band_probe: {torch.cuda.get_device_name(0)}, bf16, D={D}, C layout, reps={args.reps}, median ms']
    for legs in (window_legs, gqa_legs, chunk_legs):
        n = len(lines)
        legs(lines, args.reps)
        print('\n'.join(lines[n:]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
