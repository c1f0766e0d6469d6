"""attention_decode over a float8_e4m3fn cache against attention_decode over the bf16 cache of the same batch, bf16 q, C
layouts, host lengths, 32 query heads over 8 kv heads.  Interleaved legs (every repetition runs every leg of a group
once, in turn), HIP events around INNER calls of one leg, medians over the repetitions of the time per call; repetition 0
warms up.  The lines go to profiles/attention_decode_fp8_probe.txt as they come out; the one condition (below) is printed
as `holds` / `DOES NOT HOLD` and is the exit status.

  decode   64 sequences with U(1 024, 8 192) cached keys, D in {64, 128}, T_b in {1, 4}:
             fp8      attention_decode of the cache quantised per kv head (scale = amax / 448, tensors [heads_kv])
             bf16     attention_decode of the bf16 cache the codes were made from (the kernel of rua_attention_decode.hip)
             copy8    the fp8 K and V bytes copied once each (a streaming copy READS and WRITES the bytes)
  long     4 sequences of 32 768 keys, T_b = 1, D = 64: the same three legs.

THE CONDITION: at T_b = 1 the fp8 median is below the bf16 median by more than the larger of the two legs' max - min
spread, at both D.  The ratio to the copy is reported as it comes out, with no promise.

    python scripts/attention_decode_fp8_probe.py [--reps 5] [--inner 20] [--out profiles/attention_decode_fp8_probe.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchrua_amd as ta  # noqa: E402
from attention_decode_probe import DEV, H, HKV, measure  # noqa: E402


def group(lines, tag, klens, T, D, reps, inner):
    """The three legs of one shape; True iff fp8 beats bf16 by more than the larger spread."""
    B = klens.numel()
    cont = lambda lens, heads: ta.with_host_sizes(  # noqa: E731
        torch.randn(int(lens.sum()), heads, D, device=DEV, dtype=torch.bfloat16), lens)
    q, k, v = cont(torch.full((B,), T), H), cont(klens, HKV), cont(klens, HKV)
    ks, vs = (x.data.float().abs().amax((0, 2)) / 448 for x in (k, v))
    k8, v8 = (ta.C((x.data.float() / s[None, :, None]).to(torch.float8_e4m3fn), x.token_sizes) for x, s in ((k, ks), (v, vs)))
    kc, vc = torch.empty_like(k8.data), torch.empty_like(v8.data)
    with torch.no_grad():
        err = (q.attention_decode(k8, v8, k_scale=ks, v_scale=vs).data.float() - q.attention_decode(k, v).data.float()).abs().max().item()
        got = measure({'fp8': lambda: q.attention_decode(k8, v8, k_scale=ks, v_scale=vs),
                       'bf16': lambda: q.attention_decode(k, v),
                       'copy8': lambda: (kc.copy_(k8.data), vc.copy_(v8.data))}, reps, inner)
    nbytes = 2 * k8.data.numel()
    head = f'{tag} B={B} T={T} D={D} heads={H}/{HKV} keys={int(klens.sum())} K+V={nbytes / 2 ** 20:.0f} MiB fp8'
    for name, s in got.items():
        note = ''
        if name == 'fp8':
            note = (f'  {nbytes / s[0] / 1e9:.2f} TB/s of K + V read  bf16/fp8 {got["bf16"][0] / s[0]:.2f}x'
                    f'  copy8/fp8 {got["copy8"][0] / s[0]:.3f}  max |fp8 - bf16| {err:.3g} (the quantisation)')
        lines.append(f'{head} {name}: {s[0]:.4f} ms  (min {s[1]:.4f} max {s[2]:.4f}){note}')
    spread = max(got[n][2] - got[n][1] for n in ('fp8', 'bf16'))
    return got['bf16'][0] - got['fp8'][0] > spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_decode_fp8_probe: {torch.cuda.get_device_name(0)}, bf16 q, C layouts, reps={args.reps}, '
             f'inner={args.inner}, median ms per call']
    klens = torch.randint(1024, 8193, (64,), generator=torch.Generator().manual_seed(1))
    holds = True
    for D in (64, 128):
        for T in (1, 4):
            n = len(lines)
            ok = group(lines, 'decode', klens, T, D, args.reps, args.inner)
            if T == 1:
                holds = holds and ok
                lines.append(f'condition T=1 D={D}: bf16 - fp8 > larger spread: {"holds" if ok else "DOES NOT HOLD"}')
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
