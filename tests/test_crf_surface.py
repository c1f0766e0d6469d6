"""The linear-chain CRF: what can be checked without a GPU — the public surface, the C ABI, the refusals before any
launch, and the yardsticks themselves (tests/crf_util.py): the float64 recursion against a brute-force enumeration of
all paths, and an fp32 restatement of the recursion against the derived bound on the GPU tests' own inputs."""
import importlib
import math
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib
import crf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_crf_ws_bytes', 'rua_segment_crf_forward', 'rua_segment_crf_backtrace', 'rua_segment_crf_backward')
NAMES = ('SeqPath', 'crf_partition', 'segment_crf_partition', 'crf_marginals', 'crf_decode', 'crf_score')
METHODS = ('crf_partition', 'crf_marginals', 'crf_decode', 'crf_score')


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.crf')
    assert sorted(mod.__all__) == sorted(NAMES)
    for name in NAMES:
        assert getattr(mod, name) is getattr(ta, name), name
    for cls in (ta.C, ta.L, ta.P, ta.R):
        for name in METHODS:
            assert getattr(cls, name) is getattr(ta, name), (cls, name)
    assert ta.SeqPath._fields == ('tags', 'score')
    from torchrua_amd import _ops
    assert issubclass(_ops._CrfPartition, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import crf_partition, crf_marginals, crf_decode, crf_score, SeqPath; '
            'from torchrua.crf import segment_crf_partition as s2; '
            'assert crf_decode is ta.crf_decode and s2 is ta.segment_crf_partition and SeqPath is ta.SeqPath; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_CRF_MAX_TAGS\s+64\b', header) and _lib.CRF_MAX_TAGS == 64
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.rua_abi_version() == 6
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    fwd, bwd, bt = lib.rua_segment_crf_forward, lib.rua_segment_crf_backward, lib.rua_segment_crf_backtrace
    # (layout, x, transitions, start, end, alpha, backptr, out, last, K, dtype, semiring, stream): -1 before any launch
    assert fwd(None, 8, 8, None, None, None, None, 8, None, 5, _lib.F32, _lib.CRF_LOG, None) == -1     # null layout
    assert fwd(lay, 8, 8, None, None, None, None, 8, None, 5, _lib.I64, _lib.CRF_LOG, None) == -1      # dtype
    assert fwd(lay, 8, 8, None, None, None, None, 8, None, 5, _lib.I32, _lib.CRF_LOG, None) == -1
    assert fwd(lay, 8, 8, None, None, None, None, 8, None, 0, _lib.F32, _lib.CRF_LOG, None) == -1      # K outside [1, 64]
    assert fwd(lay, 8, 8, None, None, None, None, 8, None, 65, _lib.F32, _lib.CRF_LOG, None) == -1
    assert fwd(lay, 8, 8, None, None, None, None, 8, None, 5, _lib.F32, 2, None) == -1                 # semiring
    assert fwd(lay, None, 8, None, None, None, None, 8, None, 5, _lib.F32, _lib.CRF_LOG, None) == -1   # no emissions
    assert fwd(lay, 8, None, None, None, None, None, 8, None, 5, _lib.F32, _lib.CRF_LOG, None) == -1   # no transitions
    assert fwd(lay, 8, 8, None, None, None, None, None, None, 5, _lib.F32, _lib.CRF_LOG, None) == -1   # no out
    assert fwd(lay, 8, 8, None, None, None, None, 8, 8, 5, _lib.F32, _lib.CRF_MAX, None) == -1         # Viterbi: no backptr
    assert fwd(lay, 8, 8, None, None, None, 8, 8, None, 5, _lib.F32, _lib.CRF_MAX, None) == -1         # Viterbi: no last
    assert bt(None, 8, 8, 8, 5, None) == -1 and bt(lay, 8, 8, 8, 65, None) == -1 and bt(lay, 8, 8, 8, 0, None) == -1
    assert bt(lay, None, 8, 8, 5, None) == -1 and bt(lay, 8, None, 8, 5, None) == -1 and bt(lay, 8, 8, None, 5, None) == -1
    # (layout, grad, x, transitions, end, alpha, logz, gx, gt, gs, ge, K, dtype, ws, stream)
    assert bwd(None, 8, 8, 8, None, 8, 8, 8, None, None, None, 5, _lib.F32, None, None) == -1
    assert bwd(lay, 8, 8, 8, None, 8, 8, 8, None, None, None, 5, _lib.I64, None, None) == -1
    assert bwd(lay, 8, 8, 8, None, 8, 8, 8, None, None, None, 65, _lib.F32, None, None) == -1
    assert bwd(lay, None, 8, 8, None, 8, 8, 8, None, None, None, 5, _lib.F32, None, None) == -1        # no cotangent
    assert bwd(lay, 8, 8, 8, None, None, 8, 8, None, None, None, 5, _lib.F32, None, None) == -1        # no alpha
    assert bwd(lay, 8, 8, 8, None, 8, None, 8, None, None, None, 5, _lib.F32, None, None) == -1        # no logZ
    assert bwd(lay, 8, 8, 8, None, 8, 8, 8, 8, None, None, 5, _lib.F32, None, None) == -1              # sums without ws
    # nothing to do: 0 without a launch
    empty = _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0, len_add=0)
    assert fwd(empty, None, 8, None, None, None, None, None, None, 5, _lib.F32, _lib.CRF_LOG, None) == 0
    assert bwd(empty, None, None, 8, None, None, None, None, None, None, None, 5, _lib.F32, None, None) == 0
    # the workspace of the backward: a part [K * K + 2 K] in the accumulator type per wave, 4 waves per workgroup, at
    # most 1 024 parts
    ws = lib.rua_crf_ws_bytes
    for B, K, dtype, acc in ((1, 5, _lib.F32, 4), (10, 64, _lib.BF16, 4), (10, 9, _lib.F64, 8), (5000, 5, _lib.F16, 4),
                             (1023, 33, _lib.F32, 4), (1 << 20, 64, _lib.F64, 8)):
        lay_b = _lib.RuaLayout(kind=_lib.CAT, n_rows=4 * B, B=B, len_add=4)
        assert ws(lay_b, K, dtype) == 4 * min(-(-B // 4), 256) * (K * K + 2 * K) * acc, (B, K)
    assert ws(lay, 5, _lib.I64) == 0 and ws(lay, 65, _lib.F32) == 0 and ws(None, 5, _lib.F32) == 0
    assert ws(empty, 5, _lib.F32) == 0


def _raises(match, fn, *args, **kw):
    with pytest.raises(ta.RuaError, match=match):
        fn(*args, **kw)


def test_no_cpu_fallback_and_refusals_before_launch():
    sizes = torch.tensor([3, 4])
    x, tr, v = torch.randn(7, 3), torch.randn(3, 3), torch.randn(3)
    e = ta.C(x, sizes)
    tags = ta.C(torch.zeros(7, dtype=torch.long), sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(4, 3), torch.randn(3, 3)])
    ptags = torch.nn.utils.rnn.pack_sequence([torch.zeros(4, dtype=torch.long), torch.zeros(3, dtype=torch.long)])
    # a CPU tensor: every function, every container type
    for z, t in ((e, tags), (ta.L(torch.randn(2, 4, 3), sizes), ta.L(torch.zeros(2, 4, dtype=torch.long), sizes)),
                 (ta.R(torch.randn(2, 4, 3), sizes), ta.R(torch.zeros(2, 4, dtype=torch.long), sizes)), (p, ptags)):
        for name in ('crf_partition', 'crf_marginals', 'crf_decode'):
            _raises('emissions live on cpu', getattr(z, name), tr)
            _raises('emissions live on cpu', getattr(ta, name), z, tr, v, v)
        _raises('emissions live on cpu', z.crf_score, t, tr)
    _raises('emissions live on cpu', ta.segment_crf_partition, x, tr, sizes)
    _raises('takes a container', ta.crf_partition, x, tr)
    for fn in (ta.crf_partition, ta.crf_marginals, ta.crf_decode, lambda z, *a, **k: ta.crf_score(z, tags, *a, **k),
               lambda z, *a, **k: ta.segment_crf_partition(z.data, a[0], z.token_sizes, *a[1:], **k)):
        _raises('emissions are one of', fn, ta.C(torch.zeros(7, 3, dtype=torch.long), sizes), tr)       # integer payload
        _raises('K = 65', fn, ta.C(torch.randn(7, 65), sizes), torch.randn(65, 65))
        _raises('K = 0', fn, ta.C(torch.randn(7, 0), sizes), torch.randn(0, 0))
        _raises('ONE hidden dimension', fn, ta.C(torch.randn(7, 2, 3), sizes), tr)
        _raises('ONE hidden dimension', fn, ta.C(torch.randn(7), sizes), tr)
        _raises('`transitions` has shape', fn, e, torch.randn(3, 2))
        _raises('`transitions` has shape', fn, e, torch.randn(9))
        _raises('`transitions` is a tensor', fn, e, None)
        _raises('`start` has shape', fn, e, tr, torch.randn(4))
        _raises('`end` has shape', fn, e, tr, None, torch.randn(3, 1))
        _raises('`transitions` has dtype', fn, e, tr.double())
        _raises('`start` has dtype', fn, e, tr, v.half())
        _raises('`end` has dtype', fn, e, tr, end=v.bfloat16())
        _raises('`start` lives on', fn, e, tr, v.to('meta'))
    _raises('ONE hidden dimension', ta.crf_partition, ta.L(torch.randn(2, 4), sizes), tr)
    # crf_score: the tags
    _raises('`tags` is a CattedSequence', ta.crf_score, e, ta.L(torch.zeros(2, 4, dtype=torch.long), sizes), tr)
    _raises('`tags` is a CattedSequence', ta.crf_score, e, torch.zeros(7, dtype=torch.long), tr)
    _raises('`tags` has dtype', ta.crf_score, e, ta.C(torch.zeros(7, dtype=torch.int32), sizes), tr)
    _raises('`tags` has shape', ta.crf_score, e, ta.C(torch.zeros(6, dtype=torch.long), torch.tensor([3, 3])), tr)
    _raises('`tags` has shape', ta.crf_score, e, ta.C(torch.zeros(7, 1, dtype=torch.long), sizes), tr)
    _raises('another raggedness', ta.crf_score, e, ta.C(torch.zeros(7, dtype=torch.long), torch.tensor([3, 3, 1])), tr)
    # the same number of sequences, other lengths: host tensors are compared by value (no read-back needed)
    _raises('another raggedness', ta.crf_score, e, ta.C(torch.zeros(7, dtype=torch.long), torch.tensor([4, 3])), tr)
    _raises('another raggedness', ta.crf_score, ta.L(torch.randn(2, 4, 3), sizes),
            ta.L(torch.zeros(2, 4, dtype=torch.long), torch.tensor([4, 3])), tr)
    other = torch.nn.utils.rnn.pack_sequence([torch.zeros(5, dtype=torch.long), torch.zeros(2, dtype=torch.long)])
    _raises('another raggedness', ta.crf_score, p, other, tr)


# ------------------------------------------------------------------ the yardsticks themselves
# (The tests below check tests/crf_util.py alone — the float64 recursion, the tie rule, the batched form and the fp32
# restatement against the bound — so, unlike every test above and every GPU test, they would pass without the feature.)
def _tiny(seed):
    gen = torch.Generator().manual_seed(seed)
    K = int(torch.randint(1, 4, (1,), generator=gen))
    n = int(torch.randint(0, 6, (1,), generator=gen))
    x = torch.randn(n, K, generator=gen, dtype=torch.float64)
    tr = torch.randn(K, K, generator=gen, dtype=torch.float64)
    st, en = torch.randn(K, generator=gen, dtype=torch.float64), torch.randn(K, generator=gen, dtype=torch.float64)
    if seed % 3 == 0:                                   # forbidden moves
        tr = torch.where(torch.rand(K, K, generator=gen) < 0.3, torch.full_like(tr, -math.inf), tr)
    if seed % 6 == 0:
        st = torch.where(torch.rand(K, generator=gen) < 0.4, torch.full_like(st, -math.inf), st)
    return x, tr, (None if seed % 5 == 1 else st), (None if seed % 7 == 2 else en)


def test_recursion_equals_brute_force_enumeration():
    seen_empty = seen_inf = seen_dead = 0
    for seed in range(72):
        x, tr, st, en = _tiny(seed)
        z, best, marg = U.brute(x, tr, st, en)
        _, got = U.forward_seq(x, tr, st, en)
        seen_empty += x.size(0) == 0
        seen_inf += bool(torch.isinf(tr).any())
        if torch.isinf(z):
            seen_dead += 1
            assert got.item() == -math.inf
            continue
        assert abs(got.item() - z.item()) <= 1e-12 * (1 + abs(z.item())), seed
        lens = torch.tensor([x.size(0)])
        got_marg = U.marginals64(x, tr, st, en, lens)
        assert torch.allclose(got_marg, marg, rtol=1e-10, atol=1e-12), seed
        if x.size(0):
            assert torch.allclose(marg.sum(1), torch.ones(x.size(0), dtype=torch.float64), atol=1e-10)
        tags, score = U.viterbi_seq(x, tr, st, en)
        assert torch.equal(tags, best), seed
        want = U.path_score_seq(x, best, tr, st, en)
        assert abs(score.item() - want.item()) <= 1e-12 * (1 + abs(want.item())), seed
    assert seen_empty >= 3 and seen_inf >= 10 and seen_dead >= 1


def test_viterbi_tie_rule_on_exact_ties():
    """Integer scores: the ties are real, and the brute force's "smallest path read from its end" is what the
    smallest-backpointer rule returns."""
    for seed in range(40):
        gen = torch.Generator().manual_seed(1000 + seed)
        K, n = int(torch.randint(2, 4, (1,), generator=gen)), int(torch.randint(1, 6, (1,), generator=gen))
        x = torch.randint(-1, 2, (n, K), generator=gen).double()
        tr = torch.randint(-1, 2, (K, K), generator=gen).double()
        st, en = torch.randint(-1, 2, (K,), generator=gen).double(), torch.randint(-1, 2, (K,), generator=gen).double()
        _, best, _ = U.brute(x, tr, st, en)
        tags, _ = U.viterbi_seq(x, tr, st, en)
        assert torch.equal(tags, best), seed
    tags, score = U.viterbi_seq(torch.zeros(3, 3), torch.zeros(3, 3), None, None)
    assert tags.tolist() == [0, 0, 0] and score.item() == 0


def test_batched_yardstick_equals_the_per_sequence_one():
    """The bounds (and the yardstick of batches of many sequences) run the recursions for all sequences at once."""
    for K in (1, 5, 33):
        x, tr, st, en, lens = U.case(K, U.F32)
        alpha, beta, z, _, _ = U.batched64(x, tr, st, en, lens)
        for b, p in enumerate(U.pieces(x, lens)):
            a_seq, z_seq = U.forward_seq(p, tr, st, en)
            assert abs(z[b].item() - z_seq.item()) <= 1e-12 * (1 + abs(z_seq.item()))
            if p.size(0):
                assert torch.allclose(alpha[b, :p.size(0)], a_seq, rtol=1e-13, atol=1e-12)
                assert torch.allclose(beta[b, :p.size(0)], U.backward_seq(p, tr, en), rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize('K', U.TAGS)
def test_fp32_restatement_stays_inside_the_derived_bound(K):
    """An fp32 torch restatement of the recursion, on the CPU, on the GPU tests' own inputs: inside the bound — a failing
    GPU test then indicts the kernel, not the bound."""
    for dtype in (U.F32, U.BF16, U.F16):
        x, tr, st, en, lens = U.case(K, dtype)
        want = U.logz64(x, tr, st, en, lens)
        got = U.logz32(x, tr, st, en, lens)
        bd = U.bounds(x, tr, st, en, lens, dtype)
        r = U.ratio(got, want, bd['z'])
        print(f'crf report: fp32 torch restatement {U.name(dtype)} K={K} worst achieved/bound = {r:.4f}')
        assert r <= 1.0
        # the worst case of a sequential recursion is n * u * |alpha|: at n = 130, |logZ| = 240 that is 3e-3, 1.2e-5 |logZ|
        assert bool((bd['z'] <= 2e-5 * (1 + want.abs())).all()), 'the derived bound is implausibly loose'
