"""Per-sequence edit distance (csrc/rua_edit.hip): interleaved legs in ONE process on the same tensors.

    python scripts/edit_probe.py [--reps 5] [--window 0.05] [--small]  > profiles/edit_probe.txt

    dist C / P   rua_segment_edit_forward, the distance only, hyp and ref both C / both P        no table
    align C / P  the same writing the [rows, S_max] code table, then rua_segment_edit_backtrace
    padded       the padded GPU spelling: left() on both containers, then a Python loop over T_max rows of elementwise
                 ops plus torch.cummin on [B, S_max + 1] (the same scan identity), the distance only
    host         the host spelling: tolist() and a Python DP — timed on a SLICE of the first pairs and EXTRAPOLATED by
                 the number of cells (labelled as such; the full batch would take minutes)

Shapes: 65 536 pairs of U(8, 128) tokens (lanes form), 256 pairs of U(200, 1 600) hyps against refs capped to the lanes
form (512), and the same 256 with refs of up to 1 600 (workgroup form).  Every leg is timed over a window of about
--window seconds of work, the legs interleaved inside every repetition: only the ratios inside one run mean something.
No threshold: nobody has measured this operator before.
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fns, reps, window):
    """Per callable (median, min, max) ms per call, the callables interleaved inside every repetition; None: it failed."""
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
            f()
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


def host_dp(hyp, ref):
    """The host spelling's inner loop: two rows of Python ints."""
    prev = list(range(len(ref) + 1))
    for i, h in enumerate(hyp, 1):
        cur = [i]
        for j, r in enumerate(ref, 1):
            cur.append(min(prev[j - 1] + (h != r), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.05, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the pairs (a functional run)')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import lay_hidden, lead_shape
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved windows of '
          f'~{args.window} s; int64 tokens, an alphabet of 32')

    def fmt(t):
        return f'{"-":>9s}' if t is None else f'{t[0]:9.3f} ({t[1]:.3f}..{t[2]:.3f})'

    div = 16 if args.small else 1
    shapes = [('65536 x U(8,128)', 65536 // div, 8, 128, 128, 'lanes R=2'),
              ('256 x U(200,1600), ref <= 512', 256 // div, 200, 1600, 512, 'lanes R=8'),
              ('256 x U(200,1600)', 256 // div, 200, 1600, 1600, 'workgroup')]
    for title, B, lo, hi, cap, form in shapes:
        rs = np.random.RandomState(B + cap)
        hlens = torch.from_numpy(rs.randint(lo, hi + 1, B).astype(np.int64))
        rlens = torch.from_numpy(rs.randint(lo, hi + 1, B).astype(np.int64)).clamp(max=cap)
        g = torch.Generator(device=dev).manual_seed(B)
        hyp = torch.randint(0, 32, (int(hlens.sum()),), generator=g, device=dev)
        ref = torch.randint(0, 32, (int(rlens.sum()),), generator=g, device=dev)
        zc, rc = ta.with_host_sizes(hyp, hlens), ta.with_host_sizes(ref, rlens)
        zp, rp = zc.pack(), rc.pack()
        s_max = int(rlens.max())
        cells = int((hlens * rlens).sum())
        plans = {k: O.EditPlan(lay_hidden(z)[0], lay_hidden(r)[0], s_max) for k, (z, r) in (('C', (zc, rc)), ('P', (zp, rp)))}
        print(f'# {title} ({form} form): B = {B}, hyp tokens {hyp.numel()}, ref tokens {ref.numel()}, S_max = {s_max}, '
              f'{cells / 1e9:.3f} G cells, code table {hyp.numel() * s_max / 1e9:.3f} GB', flush=True)

        def dist(k, z, r):
            return lambda: O.launch_edit_forward(plans[k], z.data, r.data)[0]

        def align(k, z, r):
            def f():
                d, codes = O.launch_edit_forward(plans[k], z.data, r.data, want_codes=True)
                return O.launch_edit_backtrace(plans[k], codes, lead_shape(z))
            return f

        cols = torch.arange(s_max + 1, device=dev)
        rlens_dev, hlens_dev = rlens.to(dev), hlens.to(dev)

        def padded():
            h, r = zc.left(0).data, rc.left(0).data              # [B, T_max], [B, S_max]
            prev = cols.expand(B, -1).clone()
            out = rlens_dev.clone()                              # T = 0: D[0][S] = S
            for i in range(1, h.size(1) + 1):
                t = torch.minimum(prev[:, :-1] + (r != h[:, i - 1:i]), prev[:, 1:] + 1)
                t = torch.cat([torch.full((B, 1), i, device=dev), t], 1)
                prev = torch.cummin(t - cols, 1).values + cols
                out = torch.where(hlens_dev == i, prev.gather(1, rlens_dev.unsqueeze(1)).squeeze(1), out)
            return out

        want = O.launch_edit_forward(plans['C'], hyp, ref)[0]
        assert torch.equal(padded(), want), 'the padded spelling disagrees'      # (a check as well as a leg)
        assert torch.equal(O.launch_edit_forward(plans['P'], zp.data, rp.data)[0], want)
        legs = [dist('C', zc, rc), dist('P', zp, rp), align('C', zc, rc), align('P', zp, rp), padded]
        dc, dp, ac, apk, pd = timed(legs, args.reps, args.window)
        print(f'  dist C {fmt(dc)} | dist P {fmt(dp)} | align C {fmt(ac)} | align P {fmt(apk)}', flush=True)
        print(f'  padded {fmt(pd)}', flush=True)
        # the host spelling on a slice, extrapolated by the number of cells
        n = max(1, min(B, 4 if lo >= 200 else 64))
        t0 = time.perf_counter()
        hs, rs_ = zc.tolist(), rc.tolist()
        t_copy = time.perf_counter() - t0
        t0 = time.perf_counter()
        got = [host_dp(a, b) for a, b in zip(hs[:n], rs_[:n])]
        t_dp = time.perf_counter() - t0
        assert got == want[:n].tolist(), 'the host spelling disagrees'
        part = int((hlens[:n] * rlens[:n]).sum())
        host_ms = (t_copy + t_dp * cells / max(part, 1)) * 1e3
        print(f'  host   tolist {t_copy * 1e3:9.3f} ms + DP {t_dp * 1e3:.1f} ms on {n} pairs ({part / 1e6:.2f} M cells) '
              f'-> EXTRAPOLATED {host_ms:.0f} ms for the batch', flush=True)
        if dc and pd and ac:
            print(f'  ratios: dist/padded {dc[0] / pd[0]:.3f}  align/dist {ac[0] / dc[0]:.2f}  P/C {dp[0] / dc[0]:.2f}  '
                  f'host(extrapolated)/dist {host_ms / dc[0]:.0f}  G cells/s dist {cells / dc[0] / 1e6:.1f}  '
                  f'align {cells / ac[0] / 1e6:.1f}', flush=True)
        del hyp, ref, zc, rc, zp, rp
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
