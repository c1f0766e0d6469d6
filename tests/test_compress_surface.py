"""Per-sequence compress (keep tokens by mask): what can be checked without a GPU — the public surface, the Python-side
refusals, the C ABI's argument checks (none of them touches a device), the workspace formula of include/rua.h, the host
plan under the sanitizers, and the yardstick of tests/compress_util.py against a plain loop."""
import importlib
import os
import re
import shutil
import subprocess

import pytest
import torch

import torchrua_amd as ta
from compress_util import compress_cat, keep, keep_by_loop, padded, same_bits, split
from torchrua_amd import _lib
from torchrua_amd import compress as _compress_attr          # (the package attribute is the FUNCTION, like softmax)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_compress_ws_bytes', 'rua_segment_compress_plan', 'rua_segment_compress_move')
EINVAL, ERANGE = -1, -3


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.compress')
    assert _compress_attr is mod.compress
    assert sorted(mod.__all__) == ['compress', 'segment_compress']
    for name in mod.__all__:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.compress is ta.compress, cls
    from torchrua_amd import _ops
    assert callable(_ops.launch_compress_plan) and callable(_ops.launch_compress_move) and callable(_ops.compress)
    assert issubclass(_ops._Compress, torch.autograd.Function) and issubclass(_ops._Expand, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua, importlib; '
            'm = importlib.import_module("torchrua.compress"); '
            'from torchrua import compress, segment_compress; '
            'from torchrua.compress import segment_compress as s2; '
            'assert compress is ta.compress and s2 is ta.segment_compress and m.compress is ta.compress; '
            'assert torchrua.C.compress is ta.compress and torchrua.P.compress is ta.compress; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers():
    sizes = torch.tensor([3, 2])
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    return (ta.C(torch.randn(5, 2), sizes), ta.L(torch.randn(2, 4, 2), sizes), ta.R(torch.randn(2, 4, 2), sizes), p)


def _lead(z):
    return tuple(z.data.shape[:1]) if isinstance(z, (ta.C, ta.P)) else tuple(z.data.shape[:2])


def test_no_cpu_fallback():
    for z in _containers():
        mask = torch.ones(_lead(z), dtype=torch.bool)
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            z.compress(mask)
        with pytest.raises(ta.RuaError, match='no CPU fallback'):
            ta.compress(z, z._replace(data=mask))                 # the mask as a container of the same type
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_compress(torch.randn(5, 2), torch.ones(5, dtype=torch.bool), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_compress(torch.arange(5), torch.ones(5, dtype=torch.bool), torch.tensor([3, 2]))   # 1-D int64


def test_python_refuses_unfit_masks_before_any_launch():
    """Each of these is raised before the device check (the tensors are host tensors: the message tells them apart)."""
    for z in _containers():
        lead = _lead(z)
        with pytest.raises(ta.RuaError, match='must be torch.bool'):
            z.compress(torch.ones(lead, dtype=torch.uint8))
        with pytest.raises(ta.RuaError, match='must be torch.bool'):
            z.compress(torch.ones(lead))
        with pytest.raises(ta.RuaError, match='hidden dimensions'):
            z.compress(torch.ones(lead + (2,), dtype=torch.bool))
        with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
            z.compress(torch.ones((lead[0] + 1,) + lead[1:], dtype=torch.bool))
        with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
            z.compress(torch.ones(lead, dtype=torch.bool).reshape(-1)[:-1])
        with pytest.raises(ta.RuaError, match='the mask lives on meta'):
            z.compress(torch.ones(lead, dtype=torch.bool, device='meta'))
        with pytest.raises(ta.RuaError, match='torch.bool tensor'):
            z.compress([True] * lead[0])
    c, l = _containers()[:2]
    with pytest.raises(ta.RuaError, match='must be a CattedSequence'):
        c.compress(ta.L(torch.ones(2, 4, dtype=torch.bool), l.token_sizes))
    with pytest.raises(ta.RuaError, match='must be torch.bool'):
        ta.segment_compress(torch.randn(5, 2), torch.ones(5), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='hidden dimensions'):
        ta.segment_compress(torch.randn(5, 2), torch.ones(5, 2, dtype=torch.bool), torch.tensor([3, 2]))
    with pytest.raises(ta.RuaError, match='the token dimensions of the storage are'):
        ta.segment_compress(torch.randn(5, 2), torch.ones(4, dtype=torch.bool), torch.tensor([3, 2]))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
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


def test_argument_checks_need_no_device():
    """(mask, rank, new_lens, ws) = (8, 16, 32, 64) and (rank, small, big) = (16, 32, 64): made-up addresses, never
    dereferenced by a check.  Every call here returns before a launch."""
    lib = _lib.load()
    plan, move = lib.rua_segment_compress_plan, lib.rua_segment_compress_move
    lay = _lay()
    # a null layout, a negative size, a bad kind, an inconsistent layout
    assert plan(None, 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(n_rows=-1), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(B=-1), 8, 16, 32, None, None) == EINVAL
    assert plan(_lib.RuaLayout(kind=7, n_rows=8, B=2), 8, 16, 32, None, None) == EINVAL
    assert plan(_lib.RuaLayout(kind=_lib.LIST, n_rows=8, B=2), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(_lib.PACK, boff=None), 8, 16, 32, None, None) == EINVAL
    assert plan(_lay(_lib.LEFT, T_phys=-1), 8, 16, 32, None, None) == EINVAL
    # null pointers and aliasing
    assert plan(lay, None, 16, 32, None, None) == EINVAL
    assert plan(lay, 8, None, 32, None, None) == EINVAL
    assert plan(lay, 8, 16, None, None, None) == EINVAL
    assert plan(lay, 16, 16, 32, None, None) == EINVAL
    assert plan(lay, 8, 32, 32, None, None) == EINVAL
    # nothing to do: no sequence
    assert plan(_lay(B=0, n_rows=0), None, None, None, None, None) == 0
    # a length bound of 2^31 or more: a rank is an int32
    for kind, kw in ((_lib.CAT, dict(n_rows=1 << 31, B=2, len_add=0)), (_lib.CAT, dict(n_rows=1 << 40, B=2, T_log=1 << 31)),
                     (_lib.LEFT, dict(n_rows=1 << 32, B=2, T_phys=1 << 31, T_log=1 << 31)),
                     (_lib.RIGHT, dict(n_rows=1 << 32, B=2, T_phys=1 << 31, T_log=1 << 31)),
                     (_lib.PACK, dict(n_rows=1 << 32, B=2, T=1 << 31))):
        assert plan(_lay(kind, **kw), 8, 16, 32, 64, None) == ERANGE, (kind, kw)
        assert move(lay, _lay(kind, **kw), 16, 32, 64, 4, 0, None) == ERANGE, (kind, kw)
        assert move(_lay(kind, **kw), lay, 16, 32, 64, 4, 1, None) == ERANGE, (kind, kw)
        assert lib.rua_compress_ws_bytes(_lay(kind, **kw)) == 0
    assert plan(None, 8, 16, 32, 64, None) == EINVAL                              # the layout comes first
    # one token below the bound is no range error (null pointers: the next check answers)
    assert plan(_lay(n_rows=(1 << 40), T_log=(1 << 31) - 1, len_add=0), None, 16, 32, None, None) == EINVAL

    # the move: big's checks, then small's, then B, then nothing-to-do, then the pointers
    small = _lay(n_rows=4, len_add=2)
    for expand in (0, 1):
        assert move(None, lay, 16, 32, 64, 4, expand, None) == EINVAL
        assert move(small, None, 16, 32, 64, 4, expand, None) == EINVAL
        assert move(small, _lay(n_rows=-1), 16, 32, 64, 4, expand, None) == EINVAL
        assert move(_lay(n_rows=-1), lay, 16, 32, 64, 4, expand, None) == EINVAL
        assert move(_lib.RuaLayout(kind=9, n_rows=4, B=2), lay, 16, 32, 64, 4, expand, None) == EINVAL
        assert move(small, _lib.RuaLayout(kind=9, n_rows=4, B=2), 16, 32, 64, 4, expand, None) == EINVAL
        assert move(small, lay, 16, 32, 64, -4, expand, None) == EINVAL          # a negative row width
        assert move(_lay(n_rows=4, B=3, len_add=1), lay, 16, 32, 64, 4, expand, None) == EINVAL     # another B
        assert move(small, lay, None, 32, 64, 4, expand, None) == EINVAL
        assert move(small, lay, 16, None, 64, 4, expand, None) == EINVAL
        assert move(small, lay, 16, 32, None, 4, expand, None) == EINVAL
        assert move(small, lay, 16, 64, 64, 4, expand, None) == EINVAL           # small_data == big_data
        assert move(small, lay, 16, 32, 64, 0, expand, None) == 0                # rows of no bytes
        assert move(_lay(B=0, n_rows=0), _lay(B=0, n_rows=0), None, None, None, 4, expand, None) == 0
    assert move(_lay(n_rows=0, len_add=0), lay, None, None, None, 4, 0, None) == 0      # nothing was kept
    assert move(small, _lay(n_rows=0, len_add=0), None, None, None, 4, 1, None) == 0    # nothing to expand into


def _bound(lay):
    if lay.kind == _lib.CAT:
        return lay.T_log if 0 < lay.T_log < lay.n_rows else lay.n_rows
    return lay.T if lay.kind == _lib.PACK else lay.T_phys


def _documented(lay):
    """include/rua.h: B * ceil(bound / 2 048) * 4 bytes when fewer than 1 024 sequences have a bound of at least 8 192."""
    if not lay.B < 1024 or not _bound(lay) >= 8192:
        return 0
    return lay.B * -(-_bound(lay) // 2048) * 4


def test_workspace_formula():
    ws = _lib.load().rua_compress_ws_bytes
    cut = 0
    for kind in (_lib.CAT, _lib.LEFT, _lib.PACK, _lib.RIGHT):
        for B in (1, 2, 1023, 1024, 65536):
            for bound in (0, 1, 64, 2048, 8191, 8192, 8193, 40000, 200000):
                if kind == _lib.CAT:
                    lays = [_lay(kind, n_rows=bound, B=B, len_add=0), _lay(kind, n_rows=10 * bound + 1, B=B, len_add=0, T_log=bound)]
                elif kind == _lib.PACK:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T=bound)]
                else:
                    lays = [_lay(kind, n_rows=B * bound, B=B, T_phys=bound, T_log=bound)]
                for lay in lays:
                    assert ws(lay) == _documented(lay), (kind, B, bound)
                    cut += ws(lay) > 0
    assert cut >= 30                                             # (the edges do exercise the cut side)
    assert ws(_lay(n_rows=40000, B=2, len_add=20000)) == 2 * 20 * 4          # by hand: ceil(40000 / 2048) = 20 blocks
    assert ws(_lay(n_rows=40000, B=2, len_add=20000, T_log=20000)) == 2 * 10 * 4
    assert ws(_lay(n_rows=8191, B=1, len_add=8191)) == 0 and ws(_lay(n_rows=8192, B=1, len_add=8192)) == 4 * 4
    assert ws(None) == 0 and ws(_lay(n_rows=-1)) == 0 and ws(_lay(B=0, n_rows=0)) == 0
    assert ws(_lay(_lib.PACK, n_rows=40000, B=2, T=20000, boff=None)) == 0   # PACK without boff: not a layout


def test_host_plan_under_host_sanitizers(tmp_path):
    """rua_compress_plan.h is plain host C++: tests/c/compress_plan_host.cpp includes it (and rua_seg_plan.h) alone and
    walks the choice of form, the grid and the workspace over B up to 2^40 and bounds up to 2^36, every kind, under
    ASan + UBSan, as its own process; it fails on a report and on a plan the launcher could not launch as computed."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'compress_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'compress_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]


def test_the_yardstick_is_the_definition():
    g = torch.Generator().manual_seed(7)
    lens = torch.tensor([0, 1, 4, 0, 7])
    for data in (torch.randn(12, 3, generator=g), torch.arange(12), torch.randn(12, 2, 2, generator=g).bfloat16()):
        if data.is_floating_point():
            data.view(-1)[3] = float('nan')
        mask = torch.rand(12, generator=g) < 0.5
        seqs, masks = split(data, lens), split(mask, lens)
        assert [s.shape[0] for s in seqs] == lens.tolist()
        fast, slow = keep(seqs, masks), keep_by_loop(seqs, masks)
        assert len(fast) == len(slow) == 5
        for a, b in zip(fast, slow):
            assert same_bits(a, b)
        out, new = compress_cat(data, mask, lens)
        assert new.dtype == torch.int64 and new.tolist() == [int(m.sum()) for m in masks]
        assert same_bits(out, data[mask])
        assert same_bits(compress_cat(data, torch.ones(12, dtype=torch.bool), lens)[0], data)
        assert compress_cat(data, torch.zeros(12, dtype=torch.bool), lens)[0].shape == (0,) + tuple(data.shape[1:])
        left, right = padded(fast, data), padded(fast, data, right=True)
        T = int(new.max())
        assert left.shape == right.shape == (5, T) + tuple(data.shape[1:])
        for b, s in enumerate(fast):
            n = s.shape[0]
            assert same_bits(left[b, :n], s) and same_bits(right[b, T - n:], s)
            assert not bool(left[b, n:].any()) and not bool(right[b, :T - n].any())
