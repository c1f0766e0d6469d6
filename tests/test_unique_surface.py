"""Per-sequence unique_consecutive (run-length encode): what can be checked without a GPU — the public surface, the
Python-side refusals, the C ABI's argument checks (none of them touches a device), the workspace rule, and the
yardstick of tests/runs_util.py against a written-out loop.  (The operator has no host plan header of its own: its
geometry is seg_make_scan_plan, which tests/c/compress_plan_host.cpp walks.)"""
import importlib
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from runs_util import runs, runs_by_loop, runs_cat, runs_padded, same_bits, split
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_segment_runs_heads', 'rua_segment_runs_inverse', 'rua_segment_runs_counts')
EINVAL, EALIGN, ERANGE = -1, -2, -3
BITS = _lib.RUNS_BITS


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.unique')
    assert sorted(mod.__all__) == ['SeqRuns', 'segment_unique_consecutive', 'unique_consecutive']
    for name in mod.__all__:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
    assert ta.SeqRuns._fields == ('values', 'inverse', 'counts')
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.unique_consecutive is ta.unique_consecutive, cls
    from torchrua_amd import _ops
    assert callable(_ops.launch_runs_heads) and callable(_ops.launch_runs_inverse) and callable(_ops.launch_runs_counts)
    assert 'unique_consecutive' in importlib.import_module('torchrua_amd.compress').__doc__


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.unique"); '
            'from torchrua import unique_consecutive, segment_unique_consecutive, SeqRuns; '
            'from torchrua.unique import segment_unique_consecutive as s2; '
            'assert unique_consecutive is ta.unique_consecutive and s2 is ta.segment_unique_consecutive; '
            'assert m.unique_consecutive is ta.unique_consecutive and SeqRuns is ta.SeqRuns; '
            'assert torchrua.C.unique_consecutive is ta.unique_consecutive; '
            'assert torchrua.P.unique_consecutive is ta.unique_consecutive; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers(dtype=torch.float32):
    sizes = torch.tensor([3, 2])
    p = torch.nn.utils.rnn.pack_sequence([torch.zeros(3, 2, dtype=dtype), torch.zeros(2, 2, dtype=dtype)])
    return (ta.C(torch.zeros(5, 2, dtype=dtype), sizes), ta.L(torch.zeros(2, 4, 2, dtype=dtype), sizes),
            ta.R(torch.zeros(2, 4, 2, dtype=dtype), sizes), p)


def test_no_cpu_fallback():
    for dtype in (torch.float32, torch.int64, torch.bool):
        for z in _containers(dtype):
            for flags in ((False, False), (True, True)):
                with pytest.raises(ta.RuaError, match='no CPU fallback'):
                    z.unique_consecutive(*flags)
                with pytest.raises(ta.RuaError, match='no CPU fallback'):
                    ta.unique_consecutive(z, return_counts=flags[1])
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_unique_consecutive(torch.randn(5, 2), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_unique_consecutive(torch.arange(5), torch.tensor([3, 2]), True, True)      # 1-D int64


def test_python_refuses_unfit_payloads_before_any_launch():
    """Raised before the device check (the tensors are host tensors: the message tells them apart)."""
    for dtype in (torch.complex64, torch.complex128):
        for z in _containers(dtype):
            with pytest.raises(ta.RuaError, match='complex payloads are refused'):
                z.unique_consecutive()
        with pytest.raises(ta.RuaError, match='complex payloads are refused'):
            ta.segment_unique_consecutive(torch.zeros(5, dtype=dtype), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='takes a container'):
        ta.unique_consecutive(torch.zeros(5))
    from torchrua_amd import unique
    unique._check_dtype(torch.zeros(3, dtype=torch.uint8), 'x')
    unique._check_dtype(torch.zeros(3, dtype=torch.float64), 'x')

    class Wide:                                                  # (no stock real dtype has another element size)
        def is_complex(self):
            return False

        def element_size(self):
            return 16
        dtype = 'a 16-byte element'

    with pytest.raises(ta.RuaError, match='1, 2, 4 or 8 bytes'):
        unique._check_dtype(Wide(), 'x')


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_RUNS_BITS\s+0x100\b', header) and BITS == 0x100
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    assert lib.rua_abi_version() == 6 and _lib.ABI_VERSION == 6
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    assert 'rua_runs.hip' in open(os.path.join(ROOT, 'torchrua_amd', 'csrc', 'Makefile')).read()


def _lay(kind=_lib.CAT, **kw):
    if kind == _lib.CAT:
        kw = dict(dict(n_rows=8, B=2, len_add=4), **kw)
    elif kind == _lib.PACK:
        kw = dict(dict(n_rows=8, B=2, T=4, boff=0x1000), **kw)
    else:
        kw = dict(dict(n_rows=8, B=2, T_phys=4, T_log=4), **kw)
    return _lib.RuaLayout(kind=kind, **kw)


BAD_LAYOUTS = (lambda: None, lambda: _lib.RuaLayout(kind=7, n_rows=8, B=2), lambda: _lib.RuaLayout(kind=_lib.LIST, n_rows=8, B=2),
               lambda: _lay(n_rows=-1), lambda: _lay(B=-1), lambda: _lay(_lib.PACK, boff=None),
               lambda: _lay(_lib.LEFT, T_phys=-1))
TOO_LONG = ((_lib.CAT, dict(n_rows=1 << 31, B=2, len_add=0)), (_lib.CAT, dict(n_rows=1 << 40, B=2, T_log=1 << 31)),
            (_lib.LEFT, dict(n_rows=1 << 32, B=2, T_phys=1 << 31, T_log=1 << 31)),
            (_lib.RIGHT, dict(n_rows=1 << 32, B=2, T_phys=1 << 31, T_log=1 << 31)),
            (_lib.PACK, dict(n_rows=1 << 32, B=2, T=1 << 31)))


def test_argument_checks_need_no_device():
    """Made-up addresses (multiples of 64), never dereferenced by a check.  Every call here returns before a launch."""
    lib = _lib.load()
    heads, inverse, counts = lib.rua_segment_runs_heads, lib.rua_segment_runs_inverse, lib.rua_segment_runs_counts
    lay = _lay()
    # the layout comes first: null, a bad kind, negative sizes, PACK without boff
    for bad in BAD_LAYOUTS:
        assert heads(bad(), 64, 8, BITS, 128, None) == EINVAL
        assert inverse(bad(), 64, 128, 192, None, None) == EINVAL
        assert counts(bad(), lay, 64, 128, 192, None) == EINVAL
        assert counts(lay, bad(), 64, 128, 192, None) == EINVAL
    assert heads(lay, 64, -8, BITS, 128, None) == EINVAL                       # a negative row width
    # the equality rule: a float dtype code (rows of whole elements) or RUA_RUNS_BITS
    for eq in (-1, _lib.I64, _lib.U8, 0x101, 9):
        assert heads(lay, 64, 8, eq, 128, None) == EINVAL, eq
    assert heads(lay, 64, 6, _lib.F32, 128, None) == EINVAL and heads(lay, 64, 4, _lib.F64, 128, None) == EINVAL
    assert heads(lay, 64, 3, _lib.BF16, 128, None) == EINVAL and heads(lay, 64, 3, _lib.F16, 128, None) == EINVAL
    # null pointers and aliasing
    assert heads(lay, None, 8, BITS, 128, None) == EINVAL
    assert heads(lay, 64, 8, BITS, None, None) == EINVAL
    assert heads(lay, 64, 8, _lib.F64, 64, None) == EINVAL
    assert inverse(lay, None, 128, 192, None, None) == EINVAL
    assert inverse(lay, 64, None, 192, None, None) == EINVAL
    assert inverse(lay, 64, 128, None, None, None) == EINVAL
    assert inverse(lay, 64, 64, 192, None, None) == EINVAL
    assert inverse(lay, 64, 128, 64, None, None) == EINVAL
    assert inverse(lay, 64, 128, 128, None, None) == EINVAL
    assert inverse(lay, 64, 132, 192, None, None) == EALIGN and inverse(lay, 64, 128, 196, None, None) == EALIGN
    small = _lay(n_rows=4, len_add=2)
    assert counts(small, lay, None, 128, 192, None) == EINVAL
    assert counts(small, lay, 64, None, 192, None) == EINVAL
    assert counts(small, lay, 64, 128, None, None) == EINVAL
    assert counts(small, lay, 64, 64, 192, None) == EINVAL
    assert counts(small, lay, 64, 128, 128, None) == EINVAL
    assert counts(small, lay, 64, 128, 64, None) == EINVAL
    assert counts(small, lay, 66, 128, 192, None) == EALIGN and counts(small, lay, 64, 128, 196, None) == EALIGN
    assert counts(_lay(n_rows=4, B=3, len_add=1), lay, 64, 128, 192, None) == EINVAL          # another B
    # nothing to do
    empty = _lay(B=0, n_rows=0)
    assert heads(empty, None, 8, BITS, None, None) == 0 and heads(_lay(n_rows=0, len_add=0), None, 8, _lib.F32, None, None) == 0
    assert inverse(empty, None, None, None, None, None) == 0
    assert counts(empty, empty, None, None, None, None) == 0
    assert counts(_lay(n_rows=0, len_add=0), lay, None, None, None, None) == 0                 # (cannot happen: all empty)
    # a length bound of 2^31 or more: a rank, a start and a count of heads are int32
    for kind, kw in TOO_LONG:
        assert heads(_lay(kind, **kw), 64, 8, BITS, 128, None) == ERANGE, (kind, kw)
        assert inverse(_lay(kind, **kw), 64, 128, 192, 256, None) == ERANGE, (kind, kw)
        assert counts(lay, _lay(kind, **kw), 64, 128, 192, None) == ERANGE, (kind, kw)
        assert counts(_lay(kind, **kw), lay, 64, 128, 192, None) == ERANGE, (kind, kw)
    # one token below the bound is no range error (null pointers: the next check answers)
    below = _lay(n_rows=(1 << 40), T_log=(1 << 31) - 1, len_add=0)
    assert heads(below, 64, 8, BITS, None, None) == EINVAL and inverse(below, None, 128, 192, None, None) == EINVAL


def test_workspace_rule_is_the_compress_plans():
    """The inverse scan keeps one int32 count per (sequence, block), as the compress plan does: rua_compress_ws_bytes,
    B * ceil(bound / 2 048) * 4 bytes when fewer than 1 024 sequences have a bound of at least 8 192.  The other entry
    points take no workspace."""
    ws = _lib.load().rua_compress_ws_bytes
    assert ws(_lay(n_rows=40000, B=2, len_add=20000)) == 2 * 20 * 4
    assert ws(_lay(n_rows=8191, B=1, len_add=8191)) == 0 and ws(_lay(n_rows=8192, B=1, len_add=8192)) == 4 * 4
    assert ws(_lay(_lib.LEFT, n_rows=1023 * 8192, B=1023, T_phys=8192, T_log=8192)) == 1023 * 4 * 4
    assert ws(_lay(_lib.PACK, n_rows=1024 * 8192, B=1024, T=8192)) == 0
    from torchrua_amd import _ops
    import inspect
    assert "'rua_compress_ws_bytes'" in inspect.getsource(_ops.launch_runs_inverse)


CASES = (
    lambda g: torch.randint(0, 3, (12,), generator=g),
    lambda g: torch.randint(0, 2, (12, 2), generator=g).float(),
    lambda g: torch.tensor([float('nan'), float('nan'), 1., 1., -0.0, 0.0, 0.0, -0.0, 2., float('nan'), 2., 2.]),
    lambda g: torch.tensor([[0.0, 1.0], [-0.0, 1.0], [0.0, float('nan')], [0.0, float('nan')]] * 3),
    lambda g: torch.randint(0, 2, (12,), generator=g).bool(),
    lambda g: torch.randint(0, 2, (12, 3), generator=g).bool(),
    lambda g: torch.randint(0, 2, (12, 2, 2), generator=g).bfloat16(),
    lambda g: torch.tensor([1., 1., float('nan'), -0.0, 0.0, 3., 3., 3., 3., 3., 3., 0.5]).bfloat16(),
    lambda g: torch.randint(0, 2, (12,), generator=g).to(torch.float16),
    lambda g: torch.randint(0, 2, (12,), generator=g).to(torch.uint8),
)


def test_the_yardstick_is_the_definition():
    g = torch.Generator().manual_seed(7)
    lens = torch.tensor([0, 1, 4, 0, 7])
    for make in CASES:
        data = make(g)
        for seq in split(data, lens):
            fast, slow = runs(seq), runs_by_loop(seq)
            assert same_bits(fast[0], slow[0]), (data.dtype, seq)
            assert fast[1].dtype == fast[2].dtype == torch.int64
            assert torch.equal(fast[1], slow[1]) and torch.equal(fast[2], slow[2]), (data.dtype, seq)
            assert int(fast[2].sum()) == seq.shape[0] and fast[0].shape[0] == fast[2].shape[0]
        values, new, inverse, counts, parts = runs_cat(data, lens)
        assert new.dtype == torch.int64 and new.tolist() == [p[0].shape[0] for p in parts] and new[0] == new[3] == 0
        assert values.shape == (int(new.sum()),) + tuple(data.shape[1:]) and values.dtype == data.dtype
        assert inverse.shape == (12,) and counts.shape == (int(new.sum()),)
        assert same_bits(values, runs_cat(data, lens, runs_by_loop)[0])
        for right in (False, True):
            v, i, c = runs_padded(data, lens, right=right)
            T2 = int(new.max())
            assert v.shape == (5, T2) + tuple(data.shape[1:]) and i.shape == (5, 7) and c.shape == (5, T2)
            for b, p in enumerate(parts):
                n2, n = p[0].shape[0], p[1].shape[0]
                assert same_bits(v[b, T2 - n2:] if right else v[b, :n2], p[0])
                assert torch.equal(c[b, T2 - n2:] if right else c[b, :n2], p[2])
                assert torch.equal(i[b, 7 - n:] if right else i[b, :n], p[1])
                assert not bool((c[b, :T2 - n2] if right else c[b, n2:]).any())
    # a NaN row is a run of one; -0.0 and +0.0 merge and the value keeps the FIRST one's bits
    v, i, c = runs(torch.tensor([float('nan'), float('nan'), -0.0, 0.0, 0.0]))
    assert c.tolist() == [1, 1, 3] and i.tolist() == [0, 1, 2, 2, 2] and bool(torch.signbit(v[2]))
    # a global call merges across the border; the per-sequence definition does not
    ids, two = torch.tensor([5, 5, 5, 5]), torch.tensor([2, 2])
    assert torch.unique_consecutive(ids).tolist() == [5] and runs_cat(ids, two)[0].tolist() == [5, 5]
