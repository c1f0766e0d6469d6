"""A/B of an autograd-visible `z[batch_ptr, token_ptr] = v`, forward + backward, between checkouts of this project.

    python scripts/setitem_grad_ab.py --trees NEW=. PARENT=path/to/parent/checkout --rounds 3 --out prof_out/setitem_ab/ab.txt

Every tree needs its librua_hip.so built.  The driver starts ONE worker process per tree and round, alternating the trees
(A B A B ...), on one GPU in one session: between boxes and processes the same code differs by 4-6 %, so
only such an interleaved run says anything.  A worker builds the north-star shape (65 536 sequences, lengths U(8, 512),
H = 512, bf16; the keys are a permutation of all tokens), warms up and times with device events:
    leg `value`       only `value` requires grad (the storage is a plain tensor)
    leg `value+raw`   the storage is a non-leaf that requires grad as well
A tree that has the fused backward also reports the gather-and-zero kernel's rate beside the same process's copy ceiling
(C.roll(0)): bytes the algorithm needs (one read and one write of every row) over the time between two device events.
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arg(flag, default):
    if flag in sys.argv:
        return sys.argv[sys.argv.index(flag) + 1]
    return default


def worker(tree: str, B: int, reps: int, warmup: int):
    sys.path.insert(0, os.path.abspath(tree))
    import torch

    import torchrua_amd as ta
    from torchrua_amd import _ops as O
    assert os.path.abspath(ta.__file__).startswith(os.path.abspath(tree)), ta.__file__
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(8, 513, (B,), generator=g)
    n, H = int(lens.sum()), 512
    gd = torch.Generator(device=dev).manual_seed(1)

    def rand():
        return torch.randn(n, H, generator=gd, device=dev, dtype=torch.float32).to(torch.bfloat16)

    store, value, cot = rand(), rand().requires_grad_(True), rand()
    c = ta.with_host_sizes(store, lens)
    bp, tp = c.ptr()
    perm = torch.randperm(n, generator=gd, device=dev)
    bp, tp = bp[perm].contiguous(), tp[perm].contiguous()
    leaf = store.clone().requires_grad_(True)
    torch.cuda.synchronize()

    def timed(fn, setup=lambda: None):
        out = []
        for i in range(warmup + reps):
            state = setup()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(state)
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                out.append(e0.elapsed_time(e1))
        return out

    def leg_value(_):
        z = ta.C(store.detach(), c.token_sizes)
        z[bp, tp] = value
        torch.autograd.grad(z.data, [value], cot)

    def leg_both(raw):
        z = ta.C(raw, c.token_sizes)
        z[bp, tp] = value
        torch.autograd.grad(z.data, [leaf, value], cot)

    res = {'tree': tree, 'rows': n, 'row_bytes': 2 * H,
           'value': timed(leg_value),
           'value+raw': timed(leg_both, setup=lambda: leaf.clone())}    # (CloneBackward hands the gradient on: no kernel)
    if hasattr(O, 'setitem_backward'):
        from torchrua_amd import _lib as K
        from torchrua_amd import _meta as M
        from torchrua_amd.layout import describe
        plan = O.MovePlan(M.lay_list(bp, tp), describe(c), store.shape, flags=K.MOVE_SCATTER, name='setitem')
        res['kernel_gather'] = timed(lambda _: O.setitem_backward(plan, cot, (H,), True, False))
        res['kernel_gather_zero_copy'] = timed(lambda _: O.setitem_backward(plan, cot, (H,), True, True))
    res['copy_ceiling'] = timed(lambda _: c.roll(0))
    res['peak_gib'] = torch.cuda.max_memory_allocated() / 2 ** 30
    print('RESULT ' + json.dumps(res), flush=True)


def driver():
    trees = [t.split('=', 1) for t in sys.argv[sys.argv.index('--trees') + 1:] if '=' in t and not t.startswith('--')]
    rounds, B = int(_arg('--rounds', '3')), int(_arg('--seqs', '65536'))
    reps, warmup = int(_arg('--reps', '5')), int(_arg('--warmup', '2'))
    out_path = os.path.join(ROOT, _arg('--out', os.path.join('prof_out', 'setitem_ab', 'ab.txt')))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    samples = {}
    meta = {}
    peaks = {}
    for r in range(rounds):
        for name, tree in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--worker', tree, '--seqs', str(B), '--reps', str(reps),
                                '--warmup', str(warmup)], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:                       # a failed worker ends the session: nothing more is started
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(p.returncode or 1)
            line = next(ln for ln in p.stdout.splitlines() if ln.startswith('RESULT '))
            res = json.loads(line[len('RESULT '):])
            meta = {'rows': res['rows'], 'row_bytes': res['row_bytes']}
            peaks.setdefault(name, []).append(res['peak_gib'])
            for k, v in res.items():
                if isinstance(v, list):
                    samples.setdefault((name, k), []).extend(v)
            print(f'round {r} {name}: ' + '  '.join(f'{k} {statistics.median(v):.2f} ms' for k, v in res.items() if isinstance(v, list)),
                  flush=True)
    payload = meta['rows'] * meta['row_bytes']
    lines = ['# scripts/setitem_grad_ab.py: forward + backward of an autograd-visible z[batch_ptr, token_ptr] = v at the',
             f'# north-star shape ({B} sequences, lengths U(8, 512), H = 512, bf16: {meta["rows"]} rows of {meta["row_bytes"]} bytes,',
             f'# keys = a permutation of all tokens).  {rounds} rounds per tree, one fresh process each, trees alternating on one GPU;',
             f'# {reps} timed iterations per process after {warmup} warm-up ones; device events.  ms: median [min .. max] over all samples.',
             '# The interval of a leg holds the write and torch.autograd.grad, output allocations included.  The storage of leg',
             '# value+raw is a fresh clone of a leaf per iteration, enqueued BEFORE the first event: outside the interval, on',
             '# both trees (its CloneBackward hands the gradient on without a kernel).',
             '']
    for leg in ('value', 'value+raw'):
        lines.append(f'leg {leg}:')
        for name, _ in trees:
            v = samples[(name, leg)]
            lines.append(f'  {name:8s} {statistics.median(v):8.2f} ms  [{min(v):.2f} .. {max(v):.2f}]  n = {len(v)}')
        if len(trees) == 2:
            a, b = (statistics.median(samples[(trees[i][0], leg)]) for i in (0, 1))
            lines.append(f'  {trees[0][0]} / {trees[1][0]} = {a / b:.3f}')
    lines.append('')
    lines.append('kernels (TB/s = bytes the algorithm needs over the time between two device events, allocation of the outputs included):')
    for name, _ in trees:
        for k, nbytes, what in (('kernel_gather', 2 * payload, 'gather only (grad_value; one read + one write per row)'),
                                ('kernel_gather_zero_copy', 5 * payload, 'copy + gather-and-zero (grad_value and grad_raw; 2 reads + 3 writes per row)'),
                                ('copy_ceiling', 2 * payload, 'C.roll(0), the same process\'s streaming copy')):
            if (name, k) in samples:
                v = samples[(name, k)]
                t = statistics.median(v)
                lines.append(f'  {name:8s} {k:24s} {t:8.2f} ms  [{min(v):.2f} .. {max(v):.2f}]  {nbytes / t / 1e9:6.2f} TB/s   {what}')
    lines.append('')
    lines.append('peak device memory of a worker process (torch.cuda.max_memory_allocated, GiB), by round: ' +
                 ';  '.join(f'{name} ' + ' '.join(f'{x:.1f}' for x in peaks[name]) for name, _ in trees))
    text = '\n'.join(lines) + '\n'
    open(out_path, 'w').write(text)
    print(text)


if __name__ == '__main__':
    if '--worker' in sys.argv:
        worker(_arg('--worker', '.'), int(_arg('--seqs', '65536')), int(_arg('--reps', '5')), int(_arg('--warmup', '2')))
    else:
        driver()
