"""Per-sequence join / unjoin (rua_segment_join_lens + rua_segment_join): interleaved legs in ONE process on the same
tensors.  No speed threshold is set anywhere: this reports.

    python scripts/join_probe.py [--reps 5] [--window 0.15] [--small]  > profiles/join_probe.txt

    join        ta.join([za, zb]), the public call: the length launch, the offset scan (P: the host sort of the summed
                lengths and rua_pack_prepare), the move (every payload byte read once, written once)
    join+bwd    the same with payloads that require grad, then backward of a cotangent (the unjoin); floats only
    unjoin      ta.unjoin(z, [len_a, len_b]) of the joined container: the inverse, one launch for both parts
    unjoin+bwd  ... and its backward (the join of the two cotangents); floats only
    copy        out.copy_(src) over the same number of bytes: the streaming copy — the floor of the move
    stock       the spelling that was available before, for a C: ONE gather of torch.cat([a, b]) through an index built
                with repeat_interleave / arange, index construction and the torch.cat included; stock+bwd: its backward

Two parts with host lengths (no read-back in any leg), for a CattedSequence and a PackedSequence (the stock spelling
exists for a C only), at the north-star shape, the same lengths with 1-D int64 payloads, and few but long sequences (the
cut geometry).  Every leg is timed over a window of about --window seconds of work, the legs interleaved inside every
repetition: only the ratios inside one run mean something.  Printed per case: ms per call (median, min .. max over the
repetitions) and TB/s of 2 * N * H * e (joined bytes read + written) for the join.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, (shortest, longest) of part a, of part b, hidden, dtype name)"""
    s = 16 if small else 1
    return [
        ('north star: 65536 x (U(8,512) + U(1,64)), H=512 bf16', 65536 // s, (8, 512), (1, 64), (512,), 'bfloat16'),
        ('1-D int64: 65536 x (U(8,512) + U(1,64))', 65536 // s, (8, 512), (1, 64), (), 'int64'),
        ('cut: 8 x (U(100000,200000) + U(100000,200000)), H=64 bf16', 8, (100000 // s, 200000 // s),
         (100000 // s, 200000 // s), (64,), 'bfloat16'),
    ]


def payload(n, hidden, dtype, dev, seed):
    """[n, *hidden] values of `dtype`, drawn on the device in pieces (no fp32 copy of the whole)."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = torch.empty((n,) + hidden, dtype=dtype, device=dev)
    step = 1 << 22
    for a in range(0, n, step):
        m = min(n, a + step) - a
        if dtype.is_floating_point:
            out[a:a + step] = torch.randn((m,) + hidden, generator=g, device=dev)
        else:
            out[a:a + step] = torch.randint(0, 50000, (m,) + hidden, generator=g, device=dev)
    return out


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call; every window repeats its callable for about `window` seconds, the
    callables interleaved inside every repetition.  None for a leg that is None or fails."""
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
        if f is None:
            counts.append(0)
            continue
        try:
            f()                                               # warm-up
            torch.cuda.synchronize()
            counts.append(max(1, min(1000, math.ceil(window * 1e3 / max(once(f, 1), 1e-3)))))
        except Exception as e:
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.15, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; two parts; ms per call: median (min .. max) of {args.reps} interleaved '
          f'windows of ~{args.window} s; TB/s of 2*N*H*e')

    def fmt(t):
        return f'{"n/a":>27s}' if t is None else f'{t[0]:9.4f} ({t[1]:7.4f}..{t[2]:7.4f})'

    def over(a, b):
        return 'n/a' if a is None or b is None else f'{a[0] / b[0]:.3f}'

    for name, B, (alo, ahi), (blo, bhi), hidden, dtype in shapes(args.small):
        dtype = getattr(torch, dtype)
        rs = np.random.RandomState(0)
        la = torch.from_numpy(rs.randint(alo, ahi + 1, B).astype(np.int64))
        lb = torch.from_numpy(rs.randint(blo, bhi + 1, B).astype(np.int64))
        na, nb, h = int(la.sum()), int(lb.sum()), int(np.prod(hidden, dtype=np.int64))
        n = na + nb
        xa, xb = payload(na, hidden, dtype, dev, 0), payload(nb, hidden, dtype, dev, 1)
        ca, cb = ta.with_host_sizes(xa, la), ta.with_host_sizes(xb, lb)
        algo = 2 * n * h * xa.element_size()
        print(f'# {name}: N_a = {na}, N_b = {nb}, 2*N*H*e = {algo / 1e9:.3f} GB', flush=True)
        is_float = dtype.is_floating_point
        g = payload(n, hidden, dtype, dev, 3) if is_float else None
        ga, gb = (g[:na], g[na:]) if is_float else (None, None)
        src, out = payload(n, hidden, dtype, dev, 4), torch.empty((n,) + hidden, dtype=dtype, device=dev)
        da, db = la.to(dev), lb.to(dev)
        for cont in ('C', 'P'):
            za, zb = (ca.pack(), cb.pack()) if cont == 'P' else (ca, cb)
            joined = ta.join([za, zb])
            sa, sb = za.cat().token_sizes, zb.cat().token_sizes          # (device lengths with their host copies)

            def leafed(z):
                leaf = z.data.detach().clone().requires_grad_(True)
                return leaf, (ta.P(leaf, z.batch_sizes, z.sorted_indices, z.unsorted_indices) if cont == 'P' else
                              ta.C(leaf, z.token_sizes))
            (fa, wa), (fb, wb), (fj, wj) = (leafed(za), leafed(zb), leafed(joined)) if is_float else ((None,) * 2,) * 3

            def join():
                return ta.join([za, zb])

            def join_bwd():
                fa.grad = fb.grad = None
                ta.join([wa, wb]).data.backward(g)

            def unjoin():
                return ta.unjoin(joined, [sa, sb])

            def unjoin_bwd():
                fj.grad = None
                pa, pb = ta.unjoin(wj, [sa, sb])
                torch.autograd.backward([pa.data, pb.data], [ga, gb])

            def copy():
                out.copy_(src)

            def stock_index():
                new = da + db
                ends = torch.cumsum(new, 0)
                seq = torch.repeat_interleave(torch.arange(B, device=dev), new)
                pos = torch.arange(n, device=dev) - (ends - new)[seq]
                off_a, off_b = torch.cumsum(da, 0) - da, torch.cumsum(db, 0) - db + na
                return torch.where(pos < da[seq], off_a[seq] + pos, off_b[seq] + pos - da[seq]), new

            def stock():
                idx, new = stock_index()
                return torch.cat([xa, xb])[idx], new

            def stock_bwd():
                fa.grad = fb.grad = None
                idx, new = stock_index()
                torch.cat([fa, fb])[idx].backward(g)

            legs = [join, join_bwd if is_float else None, unjoin, unjoin_bwd if is_float else None, copy,
                    stock if cont == 'C' else None, stock_bwd if cont == 'C' and is_float else None]
            jo, jb, un, ub, cp, st, sb_ = timed(legs, args.reps, args.window)
            print(f'  {cont}  join {fmt(jo)} {algo / jo[0] / 1e9:6.3f} TB/s | join+bwd {fmt(jb)} | unjoin {fmt(un)} | '
                  f'unjoin+bwd {fmt(ub)} | copy {fmt(cp)} | stock {fmt(st)} | stock+bwd {fmt(sb_)}', flush=True)
            print(f'      join/copy {over(jo, cp)}  unjoin/copy {over(un, cp)}  join/stock {over(jo, st)}  '
                  f'(join+bwd)/copy {over(jb, cp)}  (join+bwd)/(stock+bwd) {over(jb, sb_)}', flush=True)
            if cont == 'C':
                same = torch.equal(joined.data.view(torch.uint8), stock()[0].contiguous().view(torch.uint8))
                print(f'      join == the stock gather bit for bit: {same}', flush=True)
            back = ta.unjoin(joined, [sa, sb])
            print(f'      unjoin(join) == the parts bit for bit: '
                  f'{torch.equal(back[0].data.view(torch.uint8), za.data.view(torch.uint8)) and torch.equal(back[1].data.view(torch.uint8), zb.data.view(torch.uint8))}',
                  flush=True)
            del za, zb, joined, fa, fb, fj, wa, wb, wj, back
        del xa, xb, ca, cb, g, ga, gb, src, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
