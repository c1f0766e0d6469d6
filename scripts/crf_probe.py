"""The per-sequence linear-chain CRF (csrc/rua_crf.hip): interleaved legs in ONE process on the same tensors.

    python scripts/crf_probe.py [--reps 5] [--window 0.05] [--small] [--no-padded]  > profiles/crf_probe.txt

    logZ         rua_segment_crf_forward (LOG), logZ only              reads the emissions once
    logZ+alpha   the same, writing the [rows, K] fp32 table            what the autograd forward does
    fwd+bwd      logZ+alpha, then rua_segment_crf_backward with all four gradients and its finish launch
    viterbi      rua_segment_crf_forward (MAX) + rua_segment_crf_backtrace
    copy         out.copy_(emissions): the streaming copy of the emission bytes (1 read + 1 write)
    padded       the spelling that was available before (C only, where it fits): z.left(), then a Python loop of T steps
                 of torch.logsumexp over a [B, K, K] broadcast with a mask that stops finished sequences — forward only

Shapes, for K in {8, 32, 64} and bf16 emissions: the north star 65 536 x U(8, 512) as a CattedSequence and a
PackedSequence, and the cut geometry 8 x U(100 000, 200 000) (one wave per sequence: the known limit).  Every leg is
timed over a window of about --window seconds of work, the legs interleaved inside every repetition: only the ratios
inside one run mean something.
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(small):
    """(name, sequences, shortest, longest, run the padded loop?)"""
    s = 16 if small else 1
    return [
        ('north star: 65536 x U(8,512)', 65536 // s, 8, 512, True),
        ('cut: 8 x U(100000,200000)', 8, 100000 // s, 200000 // s, False),
    ]


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
    ap.add_argument('--no-padded', action='store_true', help='leave the padded Python-loop spelling out')
    args = ap.parse_args()

    import numpy as np
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _meta as M
    from torchrua_amd import _ops as O
    from torchrua_amd.layout import describe
    dev = torch.device('cuda:0')
    print(f'# {torch.cuda.get_device_name(0)}; ms per call: median (min .. max) of {args.reps} interleaved windows of '
          f'~{args.window} s; bf16 emissions, fp32 accumulation')

    def fmt(t):
        return f'{"-":>9s}' if t is None else f'{t[0]:9.3f} ({t[1]:.3f}..{t[2]:.3f})'

    for name, B, lo, hi, with_loop in shapes(args.small):
        lens = torch.from_numpy(np.random.RandomState(0).randint(lo, hi + 1, B).astype(np.int64))
        n = int(lens.sum())
        for K in (8, 32, 64):
            g = torch.Generator(device=dev).manual_seed(K)
            x = torch.randn((n, K), generator=g, device=dev).bfloat16()
            tr = torch.randn((K, K), generator=g, device=dev).bfloat16()
            st, en = torch.randn(K, generator=g, device=dev).bfloat16(), torch.randn(K, generator=g, device=dev).bfloat16()
            c = ta.with_host_sizes(x, lens)
            pay = n * K * x.element_size()
            print(f'# {name}, K = {K}: N = {n}, emissions {pay / 1e9:.3f} GB, alpha {n * K * 4 / 1e9:.3f} GB', flush=True)
            for cont in ('C', 'P'):
                z = c.pack() if cont == 'P' else c
                lay = M.lay_pack(z) if cont == 'P' else describe(z)
                data = z.data
                y = torch.empty_like(data)
                w = torch.ones(B, device=dev)

                def logz():
                    return O.launch_crf_forward(lay, data, tr, st, en, K)[0]

                def logz_alpha():
                    return O.launch_crf_forward(lay, data, tr, st, en, K, want_alpha=True)

                def fwd_bwd():
                    lz, alpha, _, _ = O.launch_crf_forward(lay, data, tr, st, en, K, want_alpha=True)
                    return O.launch_crf_backward(lay, w, data, tr, en, alpha, lz, K)

                def viterbi():
                    _, _, bp, last = O.launch_crf_forward(lay, data, tr, st, en, K, viterbi=True)
                    return O.launch_crf_backtrace(lay, bp, last, data.shape[:1], K)

                def copy():
                    y.copy_(data)

                def padded():
                    l = z.left(0)
                    xs, t32, live = l.data.float(), tr.float(), l.token_sizes.to(dev)
                    a = xs[:, 0] + st.float()
                    for t in range(1, xs.size(1)):
                        nxt = xs[:, t] + torch.logsumexp(a.unsqueeze(2) + t32, 1)
                        a = torch.where((live > t).unsqueeze(1), nxt, a)
                    return torch.logsumexp(a + en.float(), 1)

                legs = [logz, logz_alpha, fwd_bwd, viterbi, copy]
                loop = with_loop and cont == 'C' and not args.no_padded
                res = timed(legs + ([padded] if loop else []), args.reps, args.window)
                lz, la, fb, vt, cp = res[:5]
                pd = res[5] if loop else None
                print(f'  {cont}  logZ {fmt(lz)} | logZ+alpha {fmt(la)} | fwd+bwd {fmt(fb)} | viterbi {fmt(vt)}', flush=True)
                print(f'     copy {fmt(cp)} | padded loop {fmt(pd)}', flush=True)
                if lz and cp and fb:
                    print(f'     ratios: logZ/copy {lz[0] / cp[0]:.1f}  fwd+bwd/copy {fb[0] / cp[0]:.1f}  '
                          f'fwd+bwd/logZ {fb[0] / lz[0]:.2f}  tokens/us logZ {n / lz[0] / 1e3:.1f}  fwd+bwd {n / fb[0] / 1e3:.1f}'
                          + (f'  logZ/padded {lz[0] / pd[0]:.4f}' if pd else ''), flush=True)
                del z, lay, data, y
            del x, c
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
