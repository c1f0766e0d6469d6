"""attention_decode_paged against the two spellings a paged pool has without it, bf16 q, C layout, host lengths, 32 query
heads over 8 kv heads, bf16 and float8_e4m3fn caches, page_size 16 and 128, the pages of the pool in a shuffled order.
Interleaved legs (every repetition runs every leg of a group once, in turn), HIP events around INNER calls of one leg,
medians over the repetitions of the time per call; repetition 0 warms up.  The lines go to
profiles/attention_decode_paged_probe.txt as they come out; the one condition (below) is printed as `holds` / `DOES NOT
HOLD` and is the exit status.

  decode   64 sequences with U(1 024, 8 192) cached keys, D in {64, 128}, T_b in {1, 4}:
             paged    attention_decode_paged over the pool and its block table
             cont     attention_decode over the same keys already gathered into a C container (the gather NOT timed)
             gather   today's spelling: index_select of the rows the table names (the row indices precomputed, K and V
                      each), then `cont`
  long     4 sequences of 32 768 keys, T_b = 1, D = 64: the same three legs.

THE CONDITION: at T_b = 1 the paged median is below the gather median by more than the larger of the two legs' max - min
spread, at every shape, cache and page size.  paged / cont — what the lookup costs — is reported as it comes out.

    python scripts/attention_decode_paged_probe.py [--reps 5] [--inner 20] [--out profiles/attention_decode_paged_probe.txt]
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

E4M3 = torch.float8_e4m3fn


def paged(klens, ps, seed):
    """(page_table [B, max_pages] int32, the pool row of every key in cat order, the number of pages), shuffled pages."""
    n_pg = (klens + ps - 1) // ps
    perm = torch.randperm(int(n_pg.sum()), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    table = torch.zeros(klens.numel(), int(n_pg.max()), dtype=torch.int32)
    rows, at = [], 0
    for b, (n, p) in enumerate(zip(klens.tolist(), n_pg.tolist())):
        table[b, :p] = perm[at:at + p]
        at += p
        s = torch.arange(n)
        rows.append(table[b, s // ps].long() * ps + s % ps)
    return table.to(DEV), torch.cat(rows).to(DEV), perm.numel()


def group(lines, tag, klens, T, D, f8, ps, reps, inner):
    """The three legs of one shape; True iff paged beats gather + cont by more than the larger spread."""
    B = klens.numel()
    cont = lambda lens, heads: ta.with_host_sizes(  # noqa: E731
        torch.randn(int(lens.sum()), heads, D, device=DEV, dtype=torch.bfloat16), lens)
    q, k, v = cont(torch.full((B,), T), H), cont(klens, HKV), cont(klens, HKV)
    scales = {}
    if f8:
        ks, vs = (x.data.float().abs().amax((0, 2)) / 448 for x in (k, v))
        k, v = (ta.C((x.data.float() / s[None, :, None]).to(E4M3), x.token_sizes) for x, s in ((k, ks), (v, vs)))
        scales = dict(k_scale=ks, v_scale=vs)
    table, rows, n_pages = paged(klens, ps, 2)
    bits = torch.uint8 if f8 else torch.int16                   # (rows are moved as integers: index ops on fp8 are few)
    pools = []
    for x in (k, v):
        flat = torch.zeros(n_pages * ps, HKV, D, dtype=bits, device=DEV)
        flat[rows] = x.data.view(bits)
        pools.append(flat)
    kp, vp = (p.view(k.data.dtype).view(n_pages, ps, HKV, D) for p in pools)
    sizes = k.token_sizes

    def gather():
        kg, vg = (p.index_select(0, rows).view(k.data.dtype) for p in pools)
        return q.attention_decode(ta.C(kg, sizes), ta.C(vg, sizes), **scales)

    with torch.no_grad():
        same = torch.equal(q.attention_decode_paged(kp, vp, table, sizes, **scales).data, q.attention_decode(k, v, **scales).data)
        got = measure({'paged': lambda: q.attention_decode_paged(kp, vp, table, sizes, **scales),
                       'cont': lambda: q.attention_decode(k, v, **scales), 'gather': gather}, reps, inner)
    nbytes = 2 * k.data.numel() * k.data.element_size()
    head = (f'{tag} B={B} T={T} D={D} heads={H}/{HKV} keys={int(klens.sum())} {"fp8" if f8 else "bf16"} page={ps} '
            f'K+V={nbytes / 2 ** 20:.0f} MiB')
    for name, s in got.items():
        note = ''
        if name == 'paged':
            note = (f'  {nbytes / s[0] / 1e9:.2f} TB/s of K + V read  paged/cont {s[0] / got["cont"][0]:.3f}'
                    f'  gather/paged {got["gather"][0] / s[0]:.2f}x  the bits of cont: {same}')
        lines.append(f'{head} {name}: {s[0]:.4f} ms  (min {s[1]:.4f} max {s[2]:.4f}){note}')
    spread = max(got[n][2] - got[n][1] for n in ('paged', 'gather'))
    return got['gather'][0] - got['paged'][0] > spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    lines = [f'attention_decode_paged_probe: {torch.cuda.get_device_name(0)}, bf16 q, C layout, shuffled pages, '
             f'reps={args.reps}, inner={args.inner}, median ms per call']
    klens = torch.randint(1024, 8193, (64,), generator=torch.Generator().manual_seed(1))
    shapes = [('decode', klens, T, D) for D in (64, 128) for T in (1, 4)] + [('long', torch.full((4,), 32768), 1, 64)]
    holds = True
    for tag, lens, T, D in shapes:
        for f8 in (False, True):
            for ps in (16, 128):
                n = len(lines)
                ok = group(lines, tag, lens, T, D, f8, ps, args.reps, args.inner)
                if T == 1:
                    holds = holds and ok
                    lines.append(f'condition {tag} T=1 D={D} {"fp8" if f8 else "bf16"} page={ps}: gather - paged > larger '
                                 f'spread: {"holds" if ok else "DOES NOT HOLD"}')
                print('\n'.join(lines[n:]), flush=True)
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0 if holds else 1


if __name__ == '__main__':
    sys.exit(main())
