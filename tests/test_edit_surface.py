"""Edit distance: what can be checked without a GPU — the public surface, the C ABI, the refusals before any launch, and
the yardstick itself (tests/edit_util.py): the numpy row-wise DP against the plain triple loop, the count identities and
the symmetry of the distance."""
import importlib
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib
import edit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_segment_edit_forward', 'rua_segment_edit_backtrace')
NAMES = ('SeqEdit', 'edit_distance', 'segment_edit_distance', 'edit_align')
METHODS = ('edit_distance', 'edit_align')


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.edit')
    assert sorted(mod.__all__) == sorted(NAMES)
    for name in NAMES:
        assert getattr(mod, name) is getattr(ta, name), name
    for cls in (ta.C, ta.L, ta.P, ta.R):
        for name in METHODS:
            assert getattr(cls, name) is getattr(ta, name), (cls, name)
    assert ta.SeqEdit._fields == ('positions', 'distance', 'substitutions', 'insertions', 'deletions')
    assert 'LIMITS' in mod.__doc__ and 'ONE BYTE per cell' in mod.__doc__ and 'swaps' in mod.__doc__


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import edit_distance, edit_align, SeqEdit; '
            'from torchrua.edit import segment_edit_distance as s2; '
            'assert edit_align is ta.edit_align and s2 is ta.segment_edit_distance and SeqEdit is ta.SeqEdit '
            'and edit_distance is ta.edit_distance; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_EDIT_MAX_REF\s+2048\b', header) and _lib.EDIT_MAX_REF == 2048
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()
    assert lib.rua_abi_version() == 6 and _lib.ABI_VERSION == 6
    lh = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    lr = _lib.RuaLayout(kind=_lib.CAT, n_rows=2, B=1, len_add=2)
    two = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=2, len_add=2)
    bad = _lib.RuaLayout(kind=7, n_rows=4, B=1)
    fwd, bt = lib.rua_segment_edit_forward, lib.rua_segment_edit_backtrace

    def f(hyp=lh, ref=lr, h=8, r=8, dist=8, codes=None, S=2):
        return fwd(hyp, ref, h, r, dist, codes, S, None)

    # -1 before any launch
    assert f(hyp=None) == -1 and f(ref=None) == -1 and f(ref=two) == -1 and f(hyp=bad) == -1 and f(ref=bad) == -1
    assert f(S=-1) == -1 and f(S=2049) == -1
    assert f(h=None) == -1 and f(r=None) == -1 and f(dist=None) == -1
    assert f(codes=8, dist=None) == -1

    def t(hyp=lh, ref=lr, codes=8, pos=8, sub=8, ins=8, dele=8, S=2):
        return bt(hyp, ref, codes, pos, sub, ins, dele, S, None)

    assert t(hyp=None) == -1 and t(ref=None) == -1 and t(ref=two) == -1 and t(hyp=bad) == -1
    assert t(S=-1) == -1 and t(S=2049) == -1
    for missing in ('codes', 'pos', 'sub', 'ins', 'dele'):
        assert t(**{missing: None}) == -1, missing
    # nothing to do: 0 without a launch
    empty = _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0, len_add=0)
    assert f(hyp=empty, ref=empty, h=None, r=None, dist=None) == 0
    assert t(hyp=empty, ref=empty, codes=None, pos=None, sub=None, ins=None, dele=None) == 0


def _raises(match, fn, *args, **kw):
    with pytest.raises(ta.RuaError, match=match):
        fn(*args, **kw)


def _four(data, sizes, dtype=torch.long, hidden=()):
    """The same sequences as C, L, R and P (CPU; zeros, only the shapes and types matter)."""
    B, t = len(sizes), int(max(sizes))
    pieces = [torch.zeros((int(n),) + hidden, dtype=dtype) for n in sizes]
    order = sorted(range(B), key=lambda b: -int(sizes[b]))
    p = torch.nn.utils.rnn.pack_sequence([pieces[b] for b in order])
    sz = torch.tensor(sizes)
    return (ta.C(torch.zeros((int(sz.sum()),) + hidden, dtype=dtype), sz), ta.L(torch.zeros((B, t) + hidden, dtype=dtype), sz),
            ta.R(torch.zeros((B, t) + hidden, dtype=dtype), sz), p)


def test_no_cpu_fallback_and_refusals_before_launch():
    hyps, refs = _four(None, [3, 4]), _four(None, [2, 1])
    fns = (ta.edit_distance, ta.edit_align)
    seg = lambda a, b: ta.segment_edit_distance(a.data, a.token_sizes, b.data, b.token_sizes)       # noqa: E731
    for a in hyps:                                              # every refusal, every pair of container types
        for fn in fns:
            _raises('takes a container', fn, a.data, refs[0])
            _raises('`ref` is a container', fn, a, refs[0].data)
            _raises('`ref` is a container', fn, a, None)
        for b in refs:
            for fn in fns:
                _raises('`hyp` lives on cpu', fn, a, b)
            _raises('`hyp` lives on cpu', a.edit_distance, b)
            _raises('`hyp` lives on cpu', a.edit_align, b)
        for kb in range(4):
            for fn in fns:
                for dt in (torch.int32, torch.float32):
                    _raises('`ref` holds torch.int64 tokens', fn, a, _four(None, [2, 1], dt)[kb])
                _raises('`ref` holds ONE token per position', fn, a, _four(None, [2, 1], hidden=(2,))[kb])
                _raises('`ref` holds 3 sequences, `hyp` 2', fn, a, _four(None, [2, 1, 1])[kb])
                _raises('`ref` has 2049 tokens', fn, a, _four(None, [2049, 1])[kb])
    for ka in range(4):
        for b in refs:
            for fn in fns:
                for dt in (torch.int32, torch.float32):
                    _raises('`hyp` holds torch.int64 tokens', fn, _four(None, [3, 4], dt)[ka], b)
                _raises('`hyp` holds ONE token per position', fn, _four(None, [3, 4], hidden=(2,))[ka], b)
    # another device
    c, r = hyps[0], refs[0]
    for fn in fns + (seg,):
        _raises('`ref` lives on meta, `hyp` on cpu', fn, c, ta.C(r.data.to('meta'), r.token_sizes))
    meta_l = ta.L(refs[1].data.to('meta'), refs[1].token_sizes)
    _raises('`ref` lives on meta', ta.edit_distance, hyps[3], meta_l)
    # the segment form
    _raises('`hyp` lives on cpu', seg, c, r)
    _raises('`other` is a tensor', ta.segment_edit_distance, c.data, c.token_sizes, None, r.token_sizes)
    _raises('`hyp` holds torch.int64 tokens', seg, ta.C(c.data.int(), c.token_sizes), r)
    _raises('`ref` holds torch.int64 tokens', seg, c, ta.C(r.data.float(), r.token_sizes))
    _raises('`ref` holds ONE token per position', seg, c, ta.C(r.data.unsqueeze(1), r.token_sizes))
    _raises('`ref` holds 3 sequences, `hyp` 2', seg, c, ta.C(r.data, torch.tensor([1, 1, 1])))
    _raises('`ref` has 2049 tokens', seg, c, _four(None, [2049, 1])[0])
    # 2 048 itself passes the bound and is refused only for the device
    _raises('`hyp` lives on cpu', ta.edit_distance, c, _four(None, [2048, 1])[0])


# ------------------------------------------------------------------ the yardstick itself
# (The tests below check tests/edit_util.py alone, so, unlike every test above and every GPU test, they would pass without
# the feature.)
def test_kitten_sitting():
    e = U.edit_loop([ord(c) for c in 'kitten'], [ord(c) for c in 'sitting'])
    assert e.distance == 3 and (e.substitutions, e.insertions, e.deletions) == (2, 0, 1)
    assert e.positions == [0, 1, 2, 3, 4, 5]                   # the diagonal first: 'g' is the deleted ref token
    e = U.edit_loop([ord(c) for c in 'sitting'], [ord(c) for c in 'kitten'])
    assert e.distance == 3 and (e.substitutions, e.insertions, e.deletions) == (2, 1, 0)
    assert U.edit_loop([], [1, 2]) == U.Edit([], 2, 0, 0, 2)
    assert U.edit_loop([1, 2, 3], []) == U.Edit([-1, -1, -1], 3, 0, 3, 0)
    assert U.edit_loop([], []) == U.Edit([], 0, 0, 0, 0)


def _random_pairs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    for k in range(n):
        alphabet = (1, 2, 3, 7)[k % 4]
        T, S = (int(v) for v in torch.randint(0, 14, (2,), generator=gen))
        yield (torch.randint(0, alphabet, (T,), generator=gen).tolist(),
               torch.randint(0, alphabet, (S,), generator=gen).tolist())


def test_numpy_version_equals_the_triple_loop():
    for hyp, ref in _random_pairs(400, 1):
        assert U.table_numpy(torch.tensor(hyp, dtype=U.I64).numpy(), torch.tensor(ref, dtype=U.I64).numpy()).tolist() \
            == U.table_loop(hyp, ref)
        assert U.edit_numpy(hyp, ref) == U.edit_loop(hyp, ref), (hyp, ref)


def test_count_identities_monotone_positions_and_alignment_cost():
    for hyp, ref in _random_pairs(400, 2):
        e = U.edit_loop(hyp, ref)
        named = [p for p in e.positions if p >= 0]
        matches = len(named) - e.substitutions
        assert e.substitutions + e.insertions + e.deletions == e.distance
        assert matches + e.substitutions + e.insertions == len(hyp)
        assert matches + e.substitutions + e.deletions == len(ref)
        assert all(a < b for a, b in zip(named, named[1:])) and all(0 <= p < len(ref) for p in named)
        assert U.alignment_cost(e, hyp, ref) == e.distance


def test_distance_is_symmetric_and_insertions_swap_with_deletions():
    for hyp, ref in _random_pairs(400, 3):
        a, b = U.edit_loop(hyp, ref), U.edit_loop(ref, hyp)
        assert a.distance == b.distance
        # (the two backtraces may split a tie differently between substitutions and insertion + deletion pairs; what
        # always holds is that the surplus of insertions over deletions changes sign)
        assert a.insertions - a.deletions == b.deletions - b.insertions == len(hyp) - len(ref)


def test_generators_hit_what_they_promise():
    for s_max in (0, 1, 63, 64, 65, 2048):
        hyps, refs = U.edge_case(s_max)
        assert max(int(r.numel()) for r in refs) == s_max and sum(int(r.numel()) == s_max for r in refs) >= 1
        assert [int(h.numel()) for h in hyps] == list(U.HYP_LENS)
