"""Per-sequence CTC (csrc/rua_ctc.hip): interleaved legs in ONE process on the same tensors.

    python scripts/ctc_probe.py [--reps 5] [--window 0.05] [--small]  > profiles/ctc_probe.txt

    fwd          rua_segment_ctc_forward (LOG), the loss only                 reads the gathered log-probabilities once
    fwd+bwd      the same writing the [rows, 2 S_max + 1] table, then rua_segment_ctc_backward (every V-wide row once)
    align        rua_segment_ctc_forward (MAX) + rua_segment_ctc_backtrace
    bwd          rua_segment_ctc_backward alone, on a table made before
    copy         out.copy_(log_probs): the streaming copy of N x V elements (1 read + 1 write) the backward is held against
    torch fwd    the padded spelling: left() on both containers, a transpose to [T, B, V], a cast to float32 (F.ctc_loss
                 takes no 16-bit input) and F.ctc_loss(reduction='none'), casts included
    torch f+b    the same with the backward to the padded float32 log-probabilities

Shapes: 256 x U(200, 1 600) frames, V in {32, 1 024, 5 000}, bf16 and f32, target length about T / 4 capped to the lanes
form (255 labels); one further shape with targets of up to 400 labels, which runs in the workgroup form.  Every leg is
timed over a window of about --window seconds of work, the legs interleaved inside every repetition: only the ratios
inside one run mean something.  No threshold: nobody has measured this operator before.
"""
import argparse
import math
import os
import statistics
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.05, help='seconds of work per timed window')
    ap.add_argument('--small', action='store_true', help='1/16 of the sequences (a functional run)')
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F

    import torchrua_amd as ta
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved windows of '
          f'~{args.window} s; fp32 accumulation')

    def fmt(t):
        return f'{"-":>9s}' if t is None else f'{t[0]:9.3f} ({t[1]:.3f}..{t[2]:.3f})'

    B = 256 // (16 if args.small else 1)
    rs = np.random.RandomState(0)
    lens = torch.from_numpy(rs.randint(200, 1601, B).astype(np.int64))
    n = int(lens.sum())
    quarter = (lens // 4).clamp(min=1)
    shapes = [(V, dt, 255, 'lanes') for V in (32, 1024, 5000) for dt in (torch.bfloat16, torch.float32)]
    shapes.append((1024, torch.bfloat16, 400, 'workgroup'))
    for V, dtype, cap, form in shapes:
        ylens = quarter.clamp(max=cap)
        g = torch.Generator(device=dev).manual_seed(V)
        lp = torch.randn((n, V), generator=g, device=dev).log_softmax(-1).to(dtype)
        y = torch.randint(1, V, (int(ylens.sum()),), generator=g, device=dev)
        z, tg = ta.with_host_sizes(lp, lens), ta.with_host_sizes(y, ylens)
        s_max = int(ylens.max())
        plan = O.CtcPlan(describe(z), describe(tg), V, s_max, 0)
        print(f'# 256 x U(200,1600), V = {V}, {str(dtype)[6:]}, targets <= {s_max} ({form} form): B = {B}, N = {n}, log_probs '
              f'{n * V * lp.element_size() / 1e9:.3f} GB, alpha {n * (2 * s_max + 1) * 4 / 1e9:.3f} GB', flush=True)
        w = torch.ones(B, device=dev)
        out = torch.empty_like(lp)
        _, logz0, alpha0, _, _ = O.launch_ctc_forward(plan, lp, y, want_alpha=True)
        lens_dev, ylens_dev = lens.to(dev), ylens.to(dev)

        def fwd():
            return O.launch_ctc_forward(plan, lp, y)[0]

        def fwd_bwd():
            _, logz, alpha, _, _ = O.launch_ctc_forward(plan, lp, y, want_alpha=True)
            return O.launch_ctc_backward(plan, w, lp, y, alpha, logz)

        def bwd():
            return O.launch_ctc_backward(plan, w, lp, y, alpha0, logz0)

        def align():
            _, _, _, codes, last = O.launch_ctc_forward(plan, lp, y, viterbi=True)
            return O.launch_ctc_backtrace(plan, y, codes, last, lp.shape[:1])

        def copy():
            out.copy_(lp)

        def padded(grad):
            x = z.left(0).data.transpose(0, 1).float()
            if grad:
                x.requires_grad_(True)
            loss = F.ctc_loss(x, tg.left(0).data, lens_dev, ylens_dev, blank=0, reduction='none')
            if grad:
                loss.sum().backward()
                return x.grad
            return loss

        res = timed([fwd, fwd_bwd, bwd, align, copy, lambda: padded(False), lambda: padded(True)], args.reps, args.window)
        fw, fb, bw, al, cp, tf, tb = res
        print(f'  fwd {fmt(fw)} | fwd+bwd {fmt(fb)} | bwd {fmt(bw)} | align {fmt(al)}', flush=True)
        print(f'  copy {fmt(cp)} | torch fwd {fmt(tf)} | torch f+b {fmt(tb)}', flush=True)
        if fw and fb and bw and cp and tf and tb:
            print(f'  ratios: fwd/torch {fw[0] / tf[0]:.2f}  fwd+bwd/torch {fb[0] / tb[0]:.2f}  bwd/copy {bw[0] / cp[0]:.1f}  '
                  f'frames/us fwd {n / fw[0] / 1e3:.2f}  fwd+bwd {n / fb[0] / 1e3:.2f}', flush=True)
        del lp, out, z, alpha0
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
