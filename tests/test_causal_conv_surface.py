"""Per-sequence causal depthwise convolution: what can be checked without a GPU — the public surface, the C ABI's
argument checks (none of them touches a device), the workspace formula of include/rua.h and the Python-side refusals.
The numerical bounds live in tests/conv_util.py; the yardstick itself is checked here against a plain loop."""
import importlib
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from conv_util import F32, F64, batch_lengths, conv64, draw, weight_grads64
from torchrua_amd import _lib
from torchrua_amd import conv as conv_module          # (the module under test: nothing here runs without it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('rua_causal_conv_ws_bytes', 'rua_segment_causal_conv', 'rua_segment_causal_conv_backward')
EINVAL, ERANGE = -1, -3


def test_public_names_exist():
    mod = importlib.import_module('torchrua_amd.conv')
    assert mod is conv_module and ta.conv is mod
    for name in ('segment_causal_conv', 'causal_conv'):
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.causal_conv is ta.causal_conv, cls
    from torchrua_amd import _ops
    assert callable(_ops.launch_causal_conv) and callable(_ops.launch_causal_conv_backward)
    assert callable(_ops.causal_conv)
    assert issubclass(_ops._CausalConv, torch.autograd.Function)
    assert issubclass(_ops._ConvWeightGrad, torch.autograd.Function)
    assert _lib.CONV_MAX_TAPS == 8


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; import torchrua.conv; '
            'from torchrua import causal_conv, segment_causal_conv; '
            'from torchrua.conv import segment_causal_conv as s2; '
            'assert causal_conv is ta.causal_conv and s2 is ta.segment_causal_conv; '
            'assert torchrua.conv is ta.conv and torchrua.C.causal_conv is ta.causal_conv; '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def _containers():
    sizes = torch.tensor([3, 4])
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    return (ta.C(torch.randn(7, 2), sizes), ta.L(torch.randn(2, 4, 2), sizes), ta.R(torch.randn(2, 4, 2), sizes), p)


def test_no_cpu_fallback():
    w, b = torch.randn(3, 2), torch.randn(2)
    for z in _containers():
        for reverse in (False, True):
            with pytest.raises(ta.RuaError, match='no CPU fallback'):
                z.causal_conv(w, b, reverse=reverse)
            with pytest.raises(ta.RuaError, match='no CPU fallback'):
                ta.causal_conv(z, w, reverse=reverse)
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_causal_conv(torch.randn(7, 2), w, torch.tensor([3, 4]), bias=b)
    with pytest.raises(ta.RuaError, match='no CPU fallback'):
        ta.segment_causal_conv(torch.randn(7), torch.randn(4), torch.tensor([3, 4]))         # a 1-D payload


def test_python_refuses_shapes_dtypes_and_filter_lengths_before_any_launch():
    """Each of these is raised before the device check (the tensors are host tensors: the message tells them apart)."""
    for z in _containers():
        with pytest.raises(ta.RuaError, match=r'\[K, \*hidden\]'):
            z.causal_conv(torch.randn(3, 5))                                   # hidden mismatch
        with pytest.raises(ta.RuaError, match=r'\[K, \*hidden\]'):
            z.causal_conv(torch.randn(3))                                      # no hidden dimension
        with pytest.raises(ta.RuaError, match=r'\[K, \*hidden\]'):
            z.causal_conv(torch.randn(3, 2, 1))
        with pytest.raises(ta.RuaError, match='the bias has shape'):
            z.causal_conv(torch.randn(3, 2), torch.randn(3))
        with pytest.raises(ta.RuaError, match='the bias has shape'):
            z.causal_conv(torch.randn(3, 2), torch.randn(1, 2))
        with pytest.raises(ta.RuaError, match='1 <= K <= 8'):
            z.causal_conv(torch.randn(0, 2))
        with pytest.raises(ta.RuaError, match='1 <= K <= 8'):
            z.causal_conv(torch.randn(9, 2))
        with pytest.raises(ta.RuaError, match='the weight has dtype'):
            z.causal_conv(torch.randn(3, 2, dtype=torch.float64))
        with pytest.raises(ta.RuaError, match='the bias has dtype'):
            z.causal_conv(torch.randn(3, 2), torch.randn(2).half())
    with pytest.raises(ta.RuaError, match='1 <= K <= 8'):
        ta.segment_causal_conv(torch.randn(7, 2), torch.randn(9, 2), torch.tensor([3, 4]))
    with pytest.raises(ta.RuaError, match=r'\[K, \*hidden\]'):
        ta.segment_causal_conv(torch.randn(7), torch.randn(3, 1), torch.tensor([3, 4]))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    assert re.search(r'#define\s+RUA_CONV_MAX_TAPS\s+8\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    assert lib.rua_abi_version() == 6
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def test_argument_checks_need_no_device():
    """(data, weight, bias, out) = (8, 16, 24, 32) and so on: made-up addresses, never dereferenced by a check."""
    lib = _lib.load()
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    fwd, bwd = lib.rua_segment_causal_conv, lib.rua_segment_causal_conv_backward
    # the layout, then H, the dtype and K
    assert fwd(None, 8, 16, 24, 32, 1, 3, _lib.F32, 0, None) == EINVAL
    assert fwd(_lib.RuaLayout(kind=_lib.CAT, n_rows=-1, B=1), 8, 16, 24, 32, 1, 3, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, 32, -1, 3, _lib.F32, 0, None) == EINVAL
    for code in (_lib.I64, _lib.I32, _lib.U8, 99):
        assert fwd(lay, 8, 16, 24, 32, 1, 3, code, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, 32, 1, 0, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, 32, 1, -2, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, 32, 1, 9, _lib.F32, 0, None) == ERANGE
    assert fwd(None, 8, 16, 24, 32, 1, 9, _lib.F32, 0, None) == EINVAL          # the layout comes first
    assert fwd(lay, 8, 16, 24, 32, 1, 9, _lib.I64, 0, None) == EINVAL           # the dtype before K
    # null pointers and aliasing
    assert fwd(lay, None, 16, 24, 32, 1, 3, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, None, 24, 32, 1, 3, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, None, 1, 3, _lib.F32, 0, None) == EINVAL
    assert fwd(lay, 8, 16, 24, 16, 1, 3, _lib.F32, 0, None) == EINVAL           # out == weight
    assert fwd(lay, 8, 16, 24, 24, 1, 3, _lib.F32, 0, None) == EINVAL           # out == bias
    # nothing to do: 0 without a launch (B == 0, n_rows == 0, H == 0), whatever the pointers
    for empty in (_lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0), _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=3),
                  _lib.RuaLayout(kind=_lib.LEFT, n_rows=0, B=0, T_phys=5, T_log=5)):
        assert fwd(empty, None, None, None, None, 4, 3, _lib.F32, 0, None) == 0
        assert bwd(empty, None, None, None, None, None, None, 4, 3, _lib.F32, 0, None, None) == 0
    assert fwd(lay, None, None, None, None, 0, 3, _lib.F32, 0, None) == 0
    assert bwd(lay, None, None, None, None, None, None, 0, 3, _lib.F32, 0, None, None) == 0
    assert bwd(lay, 8, 16, 24, None, None, None, 1, 3, _lib.F32, 0, None, None) == 0    # no output wanted
    # the backward: (grad_out, data, weight, grad_in, grad_weight, grad_bias) = (8, 16, 24, 32, 40, 48), ws = 56
    assert bwd(None, 8, 16, 24, 32, 40, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL
    assert bwd(lay, 8, 16, 24, 32, 40, 48, 1, 3, _lib.I64, 0, 56, None) == EINVAL
    assert bwd(lay, 8, 16, 24, 32, 40, 48, 1, 0, _lib.F32, 0, 56, None) == EINVAL
    assert bwd(lay, 8, 16, 24, 32, 40, 48, 1, 9, _lib.F32, 0, 56, None) == ERANGE
    assert bwd(lay, None, 16, 24, 32, 40, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL
    assert bwd(lay, 8, None, 24, 32, 40, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL     # grad_weight needs data
    assert bwd(lay, 8, 16, None, 32, 40, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL     # grad_in needs the weight
    for aliased in (8, 16, 24):                                    # grad_in == grad_out / data / weight
        assert bwd(lay, 8, 16, 24, aliased, 40, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL
    for aliased in (8, 16, 24, 32, 48):                            # grad_weight == an input / grad_in / grad_bias
        assert bwd(lay, 8, 16, 24, 32, aliased, 48, 1, 3, _lib.F32, 0, 56, None) == EINVAL
    for aliased in (8, 16, 24, 32, 40):                            # grad_bias likewise
        assert bwd(lay, 8, 16, 24, 32, 40, aliased, 1, 3, _lib.F32, 0, 56, None) == EINVAL
    # a missing workspace, when a [K, H] or [H] sum is wanted
    assert bwd(lay, 8, 16, 24, 32, 40, 48, 1, 3, _lib.F32, 0, None, None) == EINVAL
    assert bwd(lay, 8, 16, 24, None, 40, None, 1, 3, _lib.F32, 0, None, None) == EINVAL
    assert bwd(lay, 8, None, None, None, None, 48, 1, 3, _lib.F32, 0, None, None) == EINVAL


def _formula(parts, H, K, esize):
    """include/rua.h: parts * n_chunks * (128 / esize) * (K + 1) * sizeof(acc)"""
    return parts * -(-H * esize // 128) * (128 // esize) * (K + 1) * (8 if esize == 8 else 4)


def test_workspace_formula():
    ws = _lib.load().rua_causal_conv_ws_bytes
    esize = {_lib.F32: 4, _lib.F64: 8, _lib.BF16: 2, _lib.F16: 2}
    # a short batch: a part per sequence (rows of one vector: per group of 8 sequences)
    short = _lib.RuaLayout(kind=_lib.CAT, n_rows=700, B=37, len_add=0, T_log=40)
    for code, es in esize.items():
        for H in (5, 40, 64, 250):
            for K in (1, 4, 8):
                parts = 37 if H * es > 16 else -(-(-(-37 // 2)) // 4)
                assert ws(short, H, K, code) == _formula(parts, H, K, es), (code, H, K)
    # B = 2 x 20 000 tokens: the cut rule applies (fewer than 1 024 units, the bound at least 8 192): a part per block
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)                        # a CAT layout without T_log: the bound is n_rows
    for code, es in esize.items():
        assert ws(long_lay, 64, 4, code) == _formula(2 * blocks, 64, 4, es)
    assert ws(long_lay, 2, 4, _lib.F64) == _formula(1, 2, 4, 8)                # rows of one vector are never cut
    bounded = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000, T_log=20000)
    assert ws(bounded, 64, 4, _lib.F32) == _formula(2 * -(-20000 // 2048), 64, 4, 4)
    padded = _lib.RuaLayout(kind=_lib.LEFT, n_rows=40000, B=2, T_phys=20000, T_log=20000)
    assert ws(padded, 64, 4, _lib.F32) == _formula(2 * -(-20000 // 2048), 64, 4, 4)
    # a large batch: the size does not grow with B beyond the cap of 1 024 parts (nor with the number of tokens)
    for B, n in ((10 ** 6, 260 * 10 ** 6), (10 ** 7, 10 ** 10), (1024, 10 ** 6), (1025, 10 ** 6)):
        big = _lib.RuaLayout(kind=_lib.CAT, n_rows=n, B=B, len_add=0, T_log=512)
        assert ws(big, 512, 4, _lib.BF16) == _formula(1024, 512, 4, 2) == 1024 * 8 * 64 * 5 * 4
        assert ws(big, 8, 4, _lib.BF16) == _formula(min(1024, -(-(-(-B // 2)) // 4)), 8, 4, 2)
    # refused arguments and nothing to do: 0
    assert ws(None, 64, 4, _lib.F32) == 0 and ws(short, 64, 4, _lib.I64) == 0
    assert ws(short, 64, 0, _lib.F32) == 0 and ws(short, 64, 9, _lib.F32) == 0
    assert ws(short, 0, 4, _lib.F32) == 0 and ws(_lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0), 64, 4, _lib.F32) == 0


def test_the_yardstick_is_the_definition():
    """conv64 (F.conv1d per sequence) against the sums of the module docstring written as loops, both directions; and
    weight_grads64 against autograd through conv64."""
    K, H = 3, 2
    lens = torch.tensor([0, 1, 2, 5])
    x, w, b = draw((8, H), F64, 1), draw((K, H), F64, 2), draw((H,), F64, 3)
    for reverse in (False, True):
        want = torch.zeros_like(x)
        off = 0
        for n in lens.tolist():
            for t in range(n):
                acc = b.clone()
                for k in range(K):
                    src = t + (K - 1) - k if reverse else t - (K - 1) + k
                    if 0 <= src < n:
                        acc = acc + w[k] * x[off + src]
                want[off + t] = acc
            off += n
        assert torch.allclose(conv64(x, w, b, lens, reverse), want, rtol=1e-13, atol=1e-13)
        xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
        g = draw((8, H), F64, 4)
        (conv64(xr, wr, br, lens, reverse) * g).sum().backward()
        gw, gb, n_terms = weight_grads64(g, x, K, lens, reverse)
        assert torch.allclose(gw, wr.grad, rtol=1e-12, atol=1e-12) and torch.allclose(gb, br.grad, rtol=1e-12, atol=1e-12)
        assert torch.allclose(conv64(g, w, None, lens, not reverse), xr.grad, rtol=1e-12, atol=1e-12)
        assert n_terms == [0 + 0 + 0 + 3, 0 + 0 + 1 + 4, 8, 8]
    assert sorted(batch_lengths(4).tolist()) == [0, 1, 3, 4, 5, 31, 32, 33, 2047, 2048, 2049]
    assert batch_lengths(4).tolist() != sorted(batch_lengths(4).tolist())
    assert conv64(x.to(F32), w.to(F32), None, lens, False).dtype == F64
