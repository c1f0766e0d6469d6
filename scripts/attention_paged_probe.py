"""attention_paged against the only spelling a chunk of a prompt over a paged pool has without it, bf16 q, C layout, host
lengths, the pages of the pool in a shuffled order.  Interleaved legs (every repetition runs every leg of a group once,
in turn), HIP events around INNER calls of one leg, medians over the repetitions of the time per call; repetition 0
warms up.  The lines go to profiles/attention_paged_probe.txt as they come out; the one condition (below) is printed as
`holds` / `DOES NOT HOLD` and is the exit status.

  chunk    64 chunks of 512 queries over U(512, 8 192) cached keys, heads 32 / 8, D in {128, 64}, page 16 and 128, a
           bf16 and a float8_e4m3fn pool
  short    64 chunks of 16 queries, heads 32 / 4, D = 128
  g1       64 chunks of 512 queries, heads 8 / 8 (G = 1: nothing is shared between heads), D = 128
  legs:      paged     attention_paged over the pool and its block table
             gather    index_select of the rows the table names (K and V each; the row indices precomputed), for codes
                       the upcast of the gathered cache times its scales, then `attention(causal, end)`
             gather'   the same leg a second time: |gather - gather'| is the spread of the run
             cont      `attention(causal, end)` over an already gathered (and upcast) cache

THE CONDITION: at every shape with G >= 4, paged is not slower than gather by more than |gather - gather'|.  paged /
cont and the G = 1 shape are reported as they come out.

    python scripts/attention_paged_probe.py [--reps 3] [--inner 3] [--out profiles/attention_paged_probe.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torchrua_amd as ta  # noqa: E402
from attention_decode_probe import DEV, measure  # noqa: E402
from attention_decode_paged_probe import paged  # noqa: E402

E4M3, BF16 = torch.float8_e4m3fn, torch.bfloat16


def group(lines, tag, klens, T, heads, D, f8, ps, reps, inner):
    """The four legs of one shape; True iff paged - gather <= |gather - gather'|."""
    B, (H, HKV) = klens.numel(), heads
    cont = lambda lens, h: ta.with_host_sizes(torch.randn(int(lens.sum()), h, D, device=DEV, dtype=BF16), lens)  # noqa: E731
    q, k, v = cont(torch.full((B,), T), H), cont(klens, HKV), cont(klens, HKV)
    sizes, scales, ks, vs = k.token_sizes, {}, None, None
    kd, vd = k.data, v.data                                     # what the pool holds
    if f8:
        ks, vs = (x.float().abs().amax((0, 2)) / 448 for x in (kd, vd))
        kd, vd = ((x.float() / s[None, :, None]).to(E4M3) for x, s in ((kd, ks), (vd, vs)))
        scales = dict(k_scale=ks, v_scale=vs)
        k, v = (ta.C((x.to(BF16) * s[None, :, None].to(BF16)), sizes) for x, s in ((kd, ks), (vd, vs)))
    table, rows, n_pages = paged(klens, ps, 2)
    bits = torch.uint8 if f8 else torch.int16                   # (rows are moved as integers: index ops on fp8 are few)
    pools = []
    for x in (kd, vd):
        flat = torch.zeros(n_pages * ps, HKV, D, dtype=bits, device=DEV)
        flat[rows] = x.view(bits)
        pools.append(flat)
    kp, vp = (p.view(kd.dtype).view(n_pages, ps, HKV, D) for p in pools)

    def gather():
        kg, vg = (p.index_select(0, rows).view(kd.dtype) for p in pools)
        if f8:
            kg, vg = (x.to(BF16) * s[None, :, None].to(BF16) for x, s in ((kg, ks), (vg, vs)))
        return q.attention(ta.C(kg, sizes), ta.C(vg, sizes), causal=True, align='end')

    with torch.no_grad():
        err = (q.attention_paged(kp, vp, table, sizes, **scales).data.float() - gather().data.float()).abs().max().item()
        got = measure({'paged': lambda: q.attention_paged(kp, vp, table, sizes, **scales), 'gather': gather,
                       "gather'": gather, 'cont': lambda: q.attention(k, v, causal=True, align='end')}, reps, inner)
    spread = abs(got['gather'][0] - got["gather'"][0])
    head = (f'{tag} B={B} T={T} D={D} heads={H}/{HKV} keys={int(klens.sum())} {"fp8" if f8 else "bf16"} page={ps}')
    for name, s in got.items():
        note = ''
        if name == 'paged':
            note = (f'  gather/paged {got["gather"][0] / s[0]:.2f}x  paged/cont {s[0] / got["cont"][0]:.3f}'
                    f'  spread |gather - gather\'| {spread:.4f} ms  max |paged - gather| {err:.3g}')
        lines.append(f'{head} {name}: {s[0]:.4f} ms  (min {s[1]:.4f} max {s[2]:.4f}){note}')
    return got['paged'][0] - got['gather'][0] <= spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_paged_probe: {torch.cuda.get_device_name(0)}, bf16 q, C layout, shuffled pages, '
             f'reps={args.reps}, inner={args.inner}, median ms per call']
    klens = torch.randint(512, 8193, (64,), generator=torch.Generator().manual_seed(1))
    shapes = ([('chunk', 512, (32, 8), D, f8, ps) for D in (128, 64) for f8 in (False, True) for ps in (16, 128)] +
              [('short', 16, (32, 4), 128, f8, 16) for f8 in (False, True)] + [('g1', 512, (8, 8), 128, False, 16)])
    holds = True
    for tag, T, heads, D, f8, ps in shapes:
        n = len(lines)
        ok = group(lines, tag, klens, T, heads, D, f8, ps, args.reps, args.inner)
        if heads[0] // heads[1] >= 4:
            holds = holds and ok
            lines.append(f'condition {tag} D={D} {"fp8" if f8 else "bf16"} page={ps}: paged - gather <= |gather - gather\'|: '
                         f'{"holds" if ok else "DOES NOT HOLD"}')
        print('\n'.join(lines[n:]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if holds else 1


if __name__ == '__main__':
    sys.exit(main())
