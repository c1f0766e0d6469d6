"""Per-sequence join / unjoin: what can be checked without a GPU — the public surface, every Python-side refusal (raised
on host tensors, before the device check), the C ABI's argument checks (none of them touches a device), the host plan
under the sanitizers, and the yardstick of tests/join_util.py against a plain loop."""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import torchrua_amd as ta
from join_util import as_seqs, cat, join_by_loop, join_seqs, padded, same_bits, split, unjoin_seqs
from torchrua_amd import _lib
from torchrua_amd import join as _join_attr                  # (the package attribute is the FUNCTION, like compress)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_segment_join_lens', 'rua_segment_unjoin_lens', 'rua_segment_join')
NAMES = ['join', 'segment_join', 'segment_unjoin', 'unjoin']
EINVAL, EALIGN = -1, -2


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.join')
    assert _join_attr is mod.join
    assert sorted(mod.__all__) == NAMES
    for name in mod.__all__:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert callable(cls.join) and callable(cls.unjoin), cls
        assert cls.join is ta.C.join and cls.unjoin is ta.C.unjoin
    from torchrua_amd import _ops
    for name in ('launch_join_lens', 'launch_unjoin_lens', 'launch_join', 'join', 'unjoin'):
        assert callable(getattr(_ops, name)), name
    assert issubclass(_ops._Join, torch.autograd.Function) and issubclass(_ops._Unjoin, torch.autograd.Function)
    assert _lib.JOIN_MAX_PARTS == 8


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.join"); '
            'from torchrua import join, unjoin, segment_join, segment_unjoin; '
            'from torchrua.join import segment_join as s2; '
            'assert join is ta.join and unjoin is ta.unjoin and s2 is ta.segment_join and m.join is ta.join; '
            'assert torchrua.C.join is ta.C.join and torchrua.P.unjoin is ta.P.unjoin; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers():
    sizes = torch.tensor([3, 2])
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    return (ta.C(torch.randn(5, 2), sizes), ta.L(torch.randn(2, 4, 2), sizes), ta.R(torch.randn(2, 4, 2), sizes), p)


def test_no_cpu_fallback():
    for z in _containers():
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            ta.join([z, z])
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            z.join(torch.randn(2, 2))                             # a tensor part [B, *hidden]
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            ta.unjoin(z, [1, torch.tensor([1, 1])])
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            z.unjoin(2)
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_join([torch.randn(5, 2), torch.randn(3, 2)], [torch.tensor([3, 2]), torch.tensor([1, 2])])
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_join([torch.arange(5)], [torch.tensor([3, 2])])                      # 1-D int64
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_unjoin(torch.randn(5, 2), torch.tensor([3, 2]), [1, 1])


def test_python_refuses_unfit_parts_before_any_launch():
    """Each of these is raised before the device check (the tensors are host tensors: the message tells them apart)."""
    c, l, r, p = _containers()
    with pytest.raises(ta.RuaError, match='no container among the parts'):
        ta.join([torch.randn(2, 2), torch.randn(2, 2)])
    with pytest.raises(ta.RuaError, match='mixed container types'):
        ta.join([c, l])
    with pytest.raises(ta.RuaError, match='mixed container types'):
        p.join(c)
    with pytest.raises(ta.RuaError, match='mixed container types'):
        ta.join([torch.randn(2, 2), r, l])
    for z in (c, l, r, p):
        with pytest.raises(ta.RuaError, match='1 to 8 parts; got 9'):
            ta.join([z] * 9)
        with pytest.raises(ta.RuaError, match='1 to 8 parts; got 0'):
            ta.join([])
        with pytest.raises(ta.RuaError, match='takes a list of parts'):
            ta.join(z)
        with pytest.raises(ta.RuaError, match='a part is a container or a tensor'):
            ta.join([z, 3])
        with pytest.raises(ta.RuaError, match='shape \\[B, \\*hidden\\]'):
            ta.join([z, torch.randn(3, 2)])                       # another B
        with pytest.raises(ta.RuaError, match='shape \\[B, \\*hidden\\]'):
            ta.join([torch.randn(2, 3), z])                       # another hidden shape
        with pytest.raises(ta.RuaError, match='shape \\[B, \\*hidden\\]'):
            ta.join([z, torch.randn(2, 1, 2)])                    # a time dimension: that is an L, not a tensor part
        with pytest.raises(ta.RuaError, match='the dtype differs'):
            ta.join([z, torch.randn(2, 2).double()])
        with pytest.raises(ta.RuaError, match='tensors on different devices'):
            ta.join([z, torch.randn(2, 2, device='meta')])
    with pytest.raises(ta.RuaError, match='the number of sequences B differs'):
        ta.join([c, ta.C(torch.randn(5, 2), torch.tensor([3, 1, 1]))])
    with pytest.raises(ta.RuaError, match='the hidden shape differs'):
        ta.join([c, ta.C(torch.randn(5, 3), torch.tensor([3, 2]))])
    with pytest.raises(ta.RuaError, match='the hidden shape differs'):
        ta.join([l, ta.L(torch.randn(2, 4), torch.tensor([3, 2]))])
    with pytest.raises(ta.RuaError, match='the dtype differs'):
        ta.join([c, ta.C(torch.randn(5, 2).half(), torch.tensor([3, 2]))])
    with pytest.raises(ta.RuaError, match='tensors on different devices'):
        ta.join([c, ta.C(torch.randn(5, 2, device='meta'), torch.tensor([3, 2], device='meta'))])
    with pytest.raises(ta.RuaError, match='list of tensors and a list'):
        ta.segment_join([torch.randn(5, 2)], [])


def test_python_refuses_unfit_sizes_before_any_launch():
    for z in _containers():
        with pytest.raises(ta.RuaError, match='1 to 8 sizes; got 0'):
            ta.unjoin(z, [])
        with pytest.raises(ta.RuaError, match='1 to 8 sizes; got 9'):
            z.unjoin(*([1] * 9))
        with pytest.raises(ta.RuaError, match='takes a list of sizes'):
            ta.unjoin(z, 2)
        with pytest.raises(ta.RuaError, match='takes a list of sizes'):
            ta.unjoin(z, torch.tensor([1, 1]))
        for bad in (-1, 1.5, True, None, 'x', torch.tensor([1, 1], dtype=torch.int32), torch.tensor([1.0, 1.0]),
                    torch.tensor([1, 1, 1]), torch.tensor([[1, 1]]), torch.tensor(1)):
            with pytest.raises(ta.RuaError, match='sizes are int64 \\[B\\] tensors .* or non-negative ints'):
                ta.unjoin(z, [1, bad])
        with pytest.raises(ta.RuaError, match='tensors on different devices'):
            ta.unjoin(z, [torch.tensor([1, 1], device='meta')])
    with pytest.raises(ta.RuaError, match='takes a container'):
        ta.unjoin(torch.randn(2, 2), [1])


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_JOIN_MAX_PARTS\s+8\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    assert lib.rua_abi_version() == 6
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def _lay(kind=_lib.CAT, **kw):
    if kind == _lib.CAT:
        kw = dict(dict(n_rows=8, B=2, len_add=4), **kw)
    elif kind == _lib.PACK:
        kw = dict(dict(n_rows=8, B=2, T=4, boff=0x1000), **kw)
    else:
        kw = dict(dict(n_rows=8, B=2, T_phys=4, T_log=4), **kw)
    return _lib.RuaLayout(kind=kind, **kw)


def _lays(*lays):
    return (_lib.RuaLayout * len(lays))(*lays)


def _ptrs(*values):
    return (ctypes.c_void_p * len(values))(*values)


def test_argument_checks_need_no_device():
    """Made-up addresses (multiples of 8), never dereferenced by a check.  Every call here returns before a launch."""
    lib = _lib.load()
    lens, unlens, move = lib.rua_segment_join_lens, lib.rua_segment_unjoin_lens, lib.rua_segment_join
    a, b = _lay(), _lay(_lib.LEFT)
    two = _lays(a, b)
    bad_layouts = (_lay(n_rows=-1), _lay(B=-1), _lib.RuaLayout(kind=7, n_rows=8, B=2),
                   _lib.RuaLayout(kind=_lib.LIST, n_rows=8, B=2), _lay(_lib.PACK, boff=None), _lay(_lib.LEFT, T_phys=-1),
                   _lay(lens=0x100, off=None))

    # the lengths of a join
    assert lens(None, 2, 64, None, None) == EINVAL
    for n in (0, 9, -1):
        assert lens(two, n, 64, None, None) == EINVAL
    for bad in bad_layouts:
        assert lens(_lays(a, bad), 2, 64, None, None) == EINVAL
        assert lens(_lays(bad), 1, 64, None, None) == EINVAL
    assert lens(_lays(a, _lay(B=3, n_rows=12)), 2, 64, None, None) == EINVAL         # another B
    assert lens(two, 2, None, None, None) == EINVAL
    assert lens(two, 2, 64, 64, None) == EINVAL                                      # one place for both outputs
    assert lens(two, 2, 68, None, None) == EALIGN
    assert lens(two, 2, 64, 132, None) == EALIGN
    assert lens(_lays(_lay(B=0, n_rows=0)), 1, None, None, None) == 0                # no sequence: nothing to do

    # the lengths of an unjoin
    sizes, adds = _ptrs(0x200, None), (ctypes.c_int64 * 2)(0, 3)
    assert unlens(None, sizes, adds, 2, 64, None, None) == EINVAL
    for bad in bad_layouts:
        assert unlens(bad, sizes, adds, 2, 64, None, None) == EINVAL
    for n in (0, 9, -1):
        assert unlens(a, sizes, adds, n, 64, None, None) == EINVAL
    assert unlens(a, None, adds, 2, 64, None, None) == EINVAL
    assert unlens(a, sizes, None, 2, 64, None, None) == EINVAL
    assert unlens(a, sizes, adds, 2, None, None, None) == EINVAL
    assert unlens(a, sizes, adds, 2, 0x200, None, None) == EINVAL                          # out_lens is one of the sizes
    assert unlens(a, sizes, adds, 2, 64, 64, None) == EINVAL                         # one place for both outputs
    assert unlens(a, sizes, adds, 2, 64, 0x200, None) == EINVAL                      # own_lens is one of the sizes
    assert unlens(a, sizes, adds, 2, 68, None, None) == EALIGN
    assert unlens(a, sizes, adds, 2, 64, 132, None) == EALIGN
    assert unlens(a, _ptrs(0x204, None), adds, 2, 64, None, None) == EALIGN
    assert unlens(_lay(B=0, n_rows=0), sizes, adds, 2, None, None, None) == 0

    # the move: the joined layout, n_parts, the parts, B, nothing-to-do, then the pointers
    joined = _lay(n_rows=16, len_add=8)
    data = _ptrs(0x2000, 0x3000)
    for unjoin in (0, 1):
        assert move(None, two, 2, 0x1000, data, 4, unjoin, None) == EINVAL
        assert move(joined, None, 2, 0x1000, data, 4, unjoin, None) == EINVAL
        for n in (0, 9, -1):
            assert move(joined, two, n, 0x1000, data, 4, unjoin, None) == EINVAL
        for bad in bad_layouts:
            assert move(bad, two, 2, 0x1000, data, 4, unjoin, None) == EINVAL
            assert move(joined, _lays(a, bad), 2, 0x1000, data, 4, unjoin, None) == EINVAL
        assert move(joined, two, 2, 0x1000, data, -4, unjoin, None) == EINVAL        # a negative row width
        assert move(joined, _lays(a, _lay(B=3, n_rows=12)), 2, 0x1000, data, 4, unjoin, None) == EINVAL
        assert move(_lay(B=3, n_rows=12), two, 2, 0x1000, data, 4, unjoin, None) == EINVAL
        assert move(joined, two, 2, None, data, 4, unjoin, None) == EINVAL           # null payloads where rows exist
        assert move(joined, two, 2, 0x1000, None, 4, unjoin, None) == EINVAL
        assert move(joined, two, 2, 0x1000, _ptrs(0x2000, None), 4, unjoin, None) == EINVAL
        assert move(joined, two, 2, 0x1000, _ptrs(0x2000, 0x1000), 4, unjoin, None) == EINVAL    # the output aliases an input
        assert move(joined, two, 2, 0x1000, data, 0, unjoin, None) == 0              # rows of no bytes
        empty = _lay(B=0, n_rows=0)
        assert move(empty, _lays(empty, empty), 2, None, None, 4, unjoin, None) == 0
    assert move(joined, two, 2, 0x1000, _ptrs(0x2000, 0x2000), 4, 1, None) == EINVAL            # two outputs in one place
    # a destination without rows: an empty joined side (join), parts without rows (unjoin)
    none = _lay(n_rows=0, len_add=0)
    assert move(none, _lays(none, none), 2, None, _ptrs(None, None), 4, 0, None) == 0
    assert move(joined, _lays(none, none), 2, 0x1000, _ptrs(None, None), 4, 1, None) == 0
    # a part without rows needs no payload; the checks go on to the next one
    assert move(joined, _lays(none, a), 2, 0x1000, _ptrs(None, None), 4, 0, None) == EINVAL


def test_host_plan_under_host_sanitizers(tmp_path):
    """rua_join_plan.h is plain host C++: tests/c/join_plan_host.cpp includes it (and rua_seg_plan.h) alone and walks
    the form, the thread groups, the access width and the grid over B up to 2^40, bounds up to 2^36 and rows up to 2^33
    bytes, every kind, under ASan + UBSan, as its own process; it fails on a report and on a plan the launcher could not
    launch as computed."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    flags = ['-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    # can the sanitizer runtime start at all here?  Asked of an empty program, BEFORE the one under test runs: a failure
    # of that one is then never taken for the machine's
    empty = tmp_path / 'empty.cpp'
    empty.write_text('int main() { return 0; }\n')
    subprocess.run(['g++'] + flags + [str(empty), '-o', str(tmp_path / 'empty')], check=True)
    if subprocess.run([str(tmp_path / 'empty')], capture_output=True, text=True, timeout=60).returncode != 0:
        pytest.skip('the sanitizer runtime cannot start an empty program in this address-space layout')
    exe = str(tmp_path / 'join_plan_host')
    subprocess.run(['g++'] + flags + [
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'join_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]


def test_the_yardstick_is_the_definition():
    g = torch.Generator().manual_seed(11)
    la, lb = torch.tensor([0, 1, 4, 0, 7]), torch.tensor([2, 0, 3, 0, 1])
    for a, b in ((torch.randn(12, 3, generator=g), torch.randn(6, 3, generator=g)), (torch.arange(12), -torch.arange(6)),
                 (torch.randn(12, 2, 2, generator=g).bfloat16(), torch.randn(6, 2, 2, generator=g).bfloat16())):
        if a.is_floating_point():
            a.view(-1)[3] = float('nan')
        bos = a[:5] * 2                                            # one token per sequence
        parts = [as_seqs(bos), as_seqs(a, la), as_seqs(b, lb)]
        assert [s.shape[0] for s in parts[0]] == [1] * 5 and [s.shape[0] for s in parts[1]] == la.tolist()
        fast, slow = join_seqs(parts), join_by_loop(parts)
        assert len(fast) == len(slow) == 5
        for x, y in zip(fast, slow):
            assert same_bits(x, y)
        data, lens = cat(fast, a)
        assert lens.dtype == torch.int64 and lens.tolist() == (1 + la + lb).tolist()
        assert same_bits(cat(join_seqs([as_seqs(a, la)]), a)[0], a)                     # one part: a copy
        # unjoin at the parts' lengths is the inverse; short sizes drop the tail, long ones are clamped
        back = unjoin_seqs(split(data, lens), [1, la.tolist(), lb.tolist()])
        for want, got in zip(parts, back):
            assert all(same_bits(x, y) for x, y in zip(want, got))
        cut = unjoin_seqs(split(data, lens), [2, [100, 0, 1, 5, 2]])
        assert [s.shape[0] for s in cut[0]] == [2, 2, 2, 1, 2]
        assert [s.shape[0] for s in cut[1]] == [1, 0, 1, 0, 2]
        for b_, s in enumerate(split(data, lens)):
            assert same_bits(torch.cat([cut[0][b_], cut[1][b_]]), s[:cut[0][b_].shape[0] + cut[1][b_].shape[0]])
        left, right = padded(fast, a), padded(fast, a, right=True)
        T = int(lens.max())
        assert left.shape == right.shape == (5, T) + tuple(a.shape[1:])
        for b_, s in enumerate(fast):
            n = s.shape[0]
            assert same_bits(left[b_, :n], s) and same_bits(right[b_, T - n:], s)
            assert not bool(left[b_, n:].any()) and not bool(right[b_, :T - n].any())
