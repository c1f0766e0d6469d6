"""CTC: what can be checked without a GPU — the public surface, the C ABI, the refusals before any launch, and the
yardsticks themselves (tests/ctc_util.py): the float64 DP against F.ctc_loss and a brute-force enumeration, the documented
deviation of torch's gradient, and an fp32 restatement of the recursion against the derived bound on the GPU tests' own
inputs."""
import importlib
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import torchrua_amd as ta
from torchrua_amd import _lib
import ctc_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_segment_ctc_forward', 'rua_segment_ctc_backtrace', 'rua_segment_ctc_backward')
NAMES = ('SeqAlign', 'ctc_loss', 'segment_ctc_loss', 'ctc_align')
METHODS = ('ctc_loss', 'ctc_align')
EDGES = (0, 1, 31, 32, 63, 64, 127, 128, 255, 256)


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.ctc')
    assert sorted(mod.__all__) == sorted(NAMES)
    for name in NAMES:
        assert getattr(mod, name) is getattr(ta, name), name
    for cls in (ta.C, ta.L, ta.P, ta.R):
        for name in METHODS:
            assert getattr(cls, name) is getattr(ta, name), (cls, name)
    assert ta.SeqAlign._fields == ('labels', 'positions', 'score')
    from torchrua_amd import _ops
    assert issubclass(_ops._CtcLoss, torch.autograd.Function)
    for text in (mod.__doc__, ta.ctc_loss.__doc__):
        assert 'F.ctc_loss' in text and 'log_softmax(-1)' in text and "'mean'" in text


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import ctc_loss, ctc_align, SeqAlign; '
            'from torchrua.ctc import segment_ctc_loss as s2; '
            'assert ctc_align is ta.ctc_align and s2 is ta.segment_ctc_loss and SeqAlign is ta.SeqAlign; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_CTC_MAX_TARGET\s+1023\b', header) and _lib.CTC_MAX_TARGET == 1023
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.rua_abi_version() == 6
    lf = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    lt = _lib.RuaLayout(kind=_lib.CAT, n_rows=2, B=1, len_add=2)
    two = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=2, len_add=2)
    fwd, bwd, bt = lib.rua_segment_ctc_forward, lib.rua_segment_ctc_backward, lib.rua_segment_ctc_backtrace
    LOG, MAX = _lib.CRF_LOG, _lib.CRF_MAX

    def f(frames=lf, targets=lt, lp=8, y=8, alpha=None, codes=None, out=8, logz=None, last=None, V=5, S=2, blank=0,
          dtype=_lib.F32, semiring=LOG, zi=0):
        return fwd(frames, targets, lp, y, alpha, codes, out, logz, last, V, S, blank, dtype, semiring, zi, None)

    # -1 before any launch
    assert f(frames=None) == -1 and f(targets=None) == -1 and f(targets=two) == -1          # layouts; another B
    assert f(dtype=_lib.I64) == -1 and f(dtype=_lib.I32) == -1                              # dtype
    assert f(V=0) == -1 and f(S=-1) == -1 and f(S=1024) == -1                               # ranges
    assert f(blank=-1) == -1 and f(blank=5) == -1 and f(semiring=2) == -1
    assert f(lp=None) == -1 and f(y=None) == -1 and f(out=None) == -1                        # required pointers
    assert f(semiring=MAX, codes=8) == -1 and f(semiring=MAX, last=8) == -1                  # alignment: codes and last

    def t(frames=lf, targets=lt, y=8, codes=8, last=8, labels=8, positions=8, V=5, S=2, blank=0):
        return bt(frames, targets, y, codes, last, labels, positions, V, S, blank, None)

    assert t(frames=None) == -1 and t(targets=None) == -1 and t(targets=two) == -1 and t(S=1024) == -1 and t(blank=5) == -1
    assert t(y=None) == -1 and t(codes=None) == -1 and t(last=None) == -1 and t(labels=None) == -1 and t(positions=None) == -1

    def b(frames=lf, targets=lt, grad=8, lp=8, y=8, alpha=8, logz=8, gx=8, V=5, S=2, blank=0, dtype=_lib.F32):
        return bwd(frames, targets, grad, lp, y, alpha, logz, gx, V, S, blank, dtype, None)

    assert b(frames=None) == -1 and b(targets=None) == -1 and b(targets=two) == -1 and b(dtype=_lib.I64) == -1
    assert b(V=0) == -1 and b(S=1024) == -1 and b(blank=5) == -1
    for missing in ('grad', 'lp', 'y', 'alpha', 'logz', 'gx'):
        assert b(**{missing: None}) == -1, missing
    # nothing to do: 0 without a launch
    empty = _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0, len_add=0)
    assert f(frames=empty, targets=empty, lp=None, y=None, out=None) == 0
    assert t(frames=empty, targets=empty) == 0 and b(frames=empty, targets=empty, grad=None) == 0


def _raises(match, fn, *args, **kw):
    with pytest.raises(ta.RuaError, match=match):
        fn(*args, **kw)


def test_no_cpu_fallback_and_refusals_before_launch():
    sizes, tsizes = torch.tensor([3, 4]), torch.tensor([1, 2])
    x, y = torch.randn(7, 5), torch.tensor([1, 2, 3])
    z, tg = ta.C(x, sizes), ta.C(y, tsizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(4, 5), torch.randn(3, 5)])
    ptg = torch.nn.utils.rnn.pack_sequence([torch.tensor([2, 3]), torch.tensor([1])])
    containers = (z, ta.L(torch.randn(2, 4, 5), sizes), ta.R(torch.randn(2, 4, 5), sizes), p)
    targets = (tg, ta.L(torch.zeros(2, 2, dtype=torch.long), tsizes), ta.R(torch.zeros(2, 2, dtype=torch.long), tsizes), ptg)
    for a in containers:                                        # a CPU tensor: every function, every pair of types
        for b in targets:
            _raises('`log_probs` lives on cpu', a.ctc_loss, b)
            _raises('`log_probs` lives on cpu', ta.ctc_align, a, b, 1)
    _raises('`log_probs` lives on cpu', ta.segment_ctc_loss, x, sizes, y, tsizes)
    _raises('takes a container', ta.ctc_loss, x, tg)
    _raises('`targets` is a container', ta.ctc_loss, z, y)
    _raises('`targets` is a container', ta.ctc_align, z, None)
    for fn in (ta.ctc_loss, ta.ctc_align,
               lambda a, b, *r, **k: ta.segment_ctc_loss(a.data, a.token_sizes, b.data, b.token_sizes, *r, **k)):
        _raises('`log_probs` is one of', fn, ta.C(torch.zeros(7, 5, dtype=torch.long), sizes), tg)   # integer log_probs
        _raises('ONE hidden dimension', fn, ta.C(torch.randn(7), sizes), tg)
        _raises('ONE hidden dimension', fn, ta.C(torch.randn(7, 5, 2), sizes), tg)
        _raises('torch.int64 labels', fn, z, ta.C(y.int(), tsizes))
        _raises('torch.int64 labels', fn, z, ta.C(y.float(), tsizes))
        _raises('ONE label per token', fn, z, ta.C(y.unsqueeze(1), tsizes))
        _raises('`targets` holds 3 sequences', fn, z, ta.C(y, torch.tensor([1, 1, 1])))
        _raises('`targets` lives on meta', fn, z, ta.C(y.to('meta'), tsizes))
        _raises('`blank` = 5', fn, z, tg, 5)
        _raises('`blank` = -1', fn, z, tg, blank=-1)
        _raises('`blank` = 1.0', fn, z, tg, 1.0)
        _raises('`targets` has 1024 labels', fn, z, ta.C(torch.ones(1025, dtype=torch.long), torch.tensor([1, 1024])))
    _raises('ONE hidden dimension', ta.ctc_loss, ta.L(torch.randn(2, 4), sizes), tg)
    long_p = torch.nn.utils.rnn.pack_sequence([torch.ones(1024, dtype=torch.long), torch.ones(1, dtype=torch.long)])
    _raises('`targets` has 1024 labels', ta.ctc_loss, z, long_p)


# ------------------------------------------------------------------ the yardsticks themselves
# (The tests below check tests/ctc_util.py alone, so, unlike every test above and every GPU test, they would pass without
# the feature.)
def _padded(lp, lens, y, ylens):
    B, T = len(lens), max(int(lens.max()), 1)
    pad = torch.zeros(T, B, lp.size(1), dtype=U.F64)
    for b, p in enumerate(U.pieces(lp, lens)):
        pad[:p.size(0), b] = p.double()
    ypad = torch.zeros(B, max(int(ylens.max()), 1), dtype=U.I64)
    for b, q in enumerate(U.pieces(y, ylens)):
        ypad[b, :q.numel()] = q
    return pad, ypad


@pytest.mark.parametrize('s_max', EDGES)
def test_float64_dp_equals_torch_and_pins_the_deviation_of_its_gradient(s_max):
    """On the GPU tests' own inputs: the DP equals F.ctc_loss(reduction='none') in float64 on the CPU, and the DP's autograd
    gradient PLUS exp(lp) equals torch's `grad` — the documented deviation."""
    lp, lens, y, ylens = U.edge_case(s_max, U.F32)
    w = torch.ones(len(lens), dtype=U.F64)
    loss, grad = U.grads64(lp, lens, y, ylens, 0, w)
    pad, ypad = _padded(lp, lens, y, ylens)
    pad.requires_grad_(True)
    want = F.ctc_loss(pad, ypad, lens, ylens, blank=0, reduction='none')
    assert torch.allclose(loss, want, rtol=1e-12, atol=1e-12)
    want.sum().backward()
    torch_grad = torch.cat([pad.grad[:int(n), b] for b, n in enumerate(lens)])
    assert torch.allclose(grad + lp.double().exp(), torch_grad, rtol=1e-9, atol=1e-11)
    assert float((grad - torch_grad).abs().max()) > 0.1, 'torch returns another gradient than that of its own value'


def test_dp_equals_brute_force_enumeration():
    seen_inf = seen_empty = 0
    for seed in range(60):
        gen = torch.Generator().manual_seed(seed)
        V = int(torch.randint(2, 4, (1,), generator=gen))
        T, S = int(torch.randint(0, 7, (1,), generator=gen)), int(torch.randint(0, 4, (1,), generator=gen))
        blank = seed % V
        lp = torch.randn(T, V, generator=gen, dtype=U.F64)
        if seed % 4 == 0 and T:
            lp[:, seed % V] = U.NINF
        y = (blank + 1 + torch.randint(0, V - 1, (S,), generator=gen)) % V     # (a collapse cannot produce a blank label)
        want, got = U.brute(lp, y, blank), U.forward_seq(lp, y, blank)
        seen_inf += bool(torch.isinf(want))
        seen_empty += T == 0
        if torch.isinf(want):
            assert got.item() == U.NINF, seed
            continue
        assert abs(got.item() - want.item()) <= 1e-12 * (1 + abs(want.item())), seed
        labels, positions, score = U.viterbi_seq(lp, y, blank)
        assert U.collapse(labels.tolist(), blank) == y.tolist(), seed
        picked = lp[torch.arange(T), labels].sum() if T else torch.tensor(0.0, dtype=U.F64)
        assert abs(picked.item() - score.item()) <= 1e-12 * (1 + abs(score.item())), seed
        # the state posteriors of the tables add up to one per frame, and their class sums are minus the gradient
        alpha, beta, z = U.tables64(lp, y, blank)
        if T:
            post = torch.exp(alpha + beta - z)
            assert torch.allclose(post.sum(1), torch.ones(T, dtype=U.F64), atol=1e-10), seed
            ext, _ = U.extended(y, blank)
            _, grad = U.grads64(lp, torch.tensor([T]), y, torch.tensor([S]), blank, torch.ones(1))
            assert torch.allclose(torch.zeros(T, V, dtype=U.F64).index_add_(1, ext, post), -grad, atol=1e-10), seed
    assert seen_inf >= 5 and seen_empty >= 2


@pytest.mark.parametrize('s_max', EDGES)
def test_fp32_restatement_stays_inside_the_derived_bound(s_max):
    """An fp32 torch restatement of the recursion in the library's order, on the CPU, on the GPU tests' own inputs: inside
    the bound — a failing GPU test then indicts the kernel, not the bound — and the bound is not implausibly loose."""
    for dtype in (U.F32, U.BF16, U.F16):
        lp, lens, y, ylens = U.edge_case(s_max, dtype)
        want = U.loss64(lp, lens, y, ylens, 0)
        got = U.loss64(lp, lens, y, ylens, 0, U.F32)
        bd = U.bounds(lp, lens, y, ylens, 0, dtype)
        r = U.ratio(got, want, bd['z'])
        print(f'ctc report: fp32 torch restatement {U.name(dtype)} S_max={s_max} worst achieved/bound = {r:.4f}')
        assert r <= 1.0
        # the worst case of a sequential recursion is T * u * |alpha|
        assert bool((bd['z'] <= 2e-5 * (1 + want.abs())).all()), 'the derived bound is implausibly loose'
