"""Host cost of one small call of the per-sequence operators whose Python front end is shared (layout.py's container
helpers, _meta.py's read-back helpers): wall clock over --calls calls with ONE synchronise at the end, microseconds per
call.  No speed threshold is set anywhere: this reports.

    python scripts/front_probe.py [--root DIR] [--calls 2000] [--reps 3] [--label NAME]  >> NAME.jsonl
    python scripts/front_probe.py --table PARENT_A.jsonl PARENT_B.jsonl TREE.jsonl       > profiles/front_refactor_host.txt

The first form is ONE process timing every call once per repetition and printing one JSON line per call: its median over
the repetitions.  --root names the directory whose `torchrua_amd` is imported (a checkout of another commit; the kernels'
library of this tree is used when that copy holds none), so that a driver can start the same probe on two copies of the
parent commit and on this tree, one fresh process after another, round by round.  The second form reads what the rounds
appended and prints the table: per call the median of the rounds per run, tree - parent a, and the parent-against-parent
margin by the same statistic (|parent a - parent b| of the medians), as profiles/move_plan_refactor_host.txt did.

Inputs: B = 8 sequences of 1 .. 16 tokens, hidden 64, float32, as a CattedSequence with host lengths and as its pack().
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(paths):
    runs = []
    for path in paths:
        per_call = {}
        for line in open(path):
            rec = json.loads(line)
            per_call.setdefault(rec['call'], []).append(rec['us'])
        runs.append(per_call)
    a, b, tree = runs
    print(f'{"call":28s}  parent a  parent b this tree  tree - a    margin   rounds')
    within = 0
    for call in a:
        ma, mb, mt = (statistics.median(r[call]) for r in (a, b, tree))
        margin, lo, hi = abs(ma - mb), min(ma, mb), max(ma, mb)
        verdict = 'within' if lo - margin <= mt <= hi + margin else ('over' if mt > hi else 'under')
        within += verdict == 'within'
        print(f'{call:28s} {ma:9.2f} {mb:9.2f} {mt:9.2f} {mt - ma:+9.2f} {margin:9.2f} {len(tree[call]):8d}   {verdict}')
    print(f'{within} of {len(a)} lines within the parent-against-parent margin of the medians')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=ROOT, help='the directory whose torchrua_amd package is measured')
    ap.add_argument('--calls', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--label', default='tree')
    ap.add_argument('--table', nargs=3, metavar='JSONL')
    args = ap.parse_args()
    if args.table:
        return table(args.table)

    root = os.path.abspath(args.root)
    if not os.path.exists(os.path.join(root, 'torchrua_amd', 'librua_hip.so')):
        os.environ.setdefault('RUA_LIB_PATH', os.path.join(ROOT, 'torchrua_amd', 'librua_hip.so'))
    sys.path.insert(0, root)

    import numpy as np
    import torch

    import torchrua_amd as ta
    assert os.path.dirname(os.path.dirname(os.path.abspath(ta.__file__))) == root, ta.__file__
    dev = torch.device('cuda:0')
    lens = torch.from_numpy(np.random.RandomState(0).randint(1, 17, 8).astype(np.int64))
    n = int(lens.sum())
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((n, 64), generator=g, device=dev)
    c = ta.with_host_sizes(x, lens)
    for kind, z in (('C', c), ('P', c.pack())):
        mask = torch.rand(n, generator=g, device=dev) < 0.5
        counts = torch.randint(0, 3, (n,), generator=g, device=dev)
        order = z.argsort().data[:, 0].contiguous()
        scores = torch.randn(n, generator=g, device=dev)
        gate = torch.rand((n, 64), generator=g, device=dev)
        joined = z.join(z)
        legs = [
            ('compress (device mask)', lambda: z.compress(mask)),
            ('repeat_interleave (int)', lambda: z.repeat_interleave(2)),
            ('repeat_interleave (tensor)', lambda: z.repeat_interleave(counts)),
            ('join (host lengths)', lambda: z.join(z)),
            ('unjoin', lambda: joined.unjoin(4, 100)),
            ('window_pool', lambda: z.window_pool(2)),
            ('sort', lambda: z.sort()),
            ('reorder', lambda: z.reorder(order)),
            ('unique_consecutive', lambda: z.unique_consecutive()),
            ('softmax_pool', lambda: z.softmax_pool(scores)),
            ('linear_scan', lambda: z.linear_scan(gate)),
        ]
        for name, leg in legs:
            for _ in range(50):
                leg()
            torch.cuda.synchronize()
            took = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    leg()
                torch.cuda.synchronize()
                took.append((time.perf_counter() - t0) / args.calls * 1e6)
            print(json.dumps({'label': args.label, 'call': f'{name} {kind}', 'us': statistics.median(took),
                              'reps': [round(t, 3) for t in took]}), flush=True)


if __name__ == '__main__':
    main()
