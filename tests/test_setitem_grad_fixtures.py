"""The gradient fixtures of an autograd-visible `__setitem__` (tests/golden/r6_setitem_grad.npz, made by
scripts/gen_golden_setitem_grad.py from the reference's CPU autograd) and the C entry point behind its backward
(rua_setitem_backward), as far as they can be checked without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r6_setitem_grad.npz')


def load_cases():
    z = np.load(GOLDEN)
    out = {}
    for key in z.files:
        case, name = key.rsplit('/', 1)
        out.setdefault(case, {})[name] = z[key]
    return out


CASES = load_cases()


def widen(a: np.ndarray, dtype: str) -> np.ndarray:
    """A fixture array as float64 (bf16 travels as its uint16 bit pattern)."""
    if dtype == 'bf16':
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def narrow(a: np.ndarray, dtype: str) -> np.ndarray:
    """... and back: every number in these fixtures is an integer the dtype holds exactly."""
    if dtype == 'bf16':
        bits = a.astype(np.float32).view(np.uint32)
        assert not (bits & 0xffff).any(), 'not exactly representable in bf16'
        return (bits >> 16).astype(np.uint16)
    return a.astype({'fp32': np.float32, 'fp64': np.float64, 'fp16': np.float16}[dtype])


def restate(f):
    """The backward of `rows_of(raw)[flat] = value` under the cotangent `cot`, with raw = base * 2: gather, zero, row sum."""
    dtype = str(f['dtype'])
    lead_dims = 2 if str(f['kind']) in 'LR' else 1
    cot = widen(f['cot'], dtype)
    hidden = cot.shape[lead_dims:]
    rows = cot.reshape((-1,) + hidden)
    flat = f['flat']
    g_value = rows[flat.reshape(-1)].reshape(flat.shape + hidden)            # gather
    g_raw = rows.copy()
    g_raw[flat.reshape(-1)] = 0                                              # zero
    vshape = f['value'].shape
    pad = (1,) * (g_value.ndim - len(vshape)) + vshape
    axes = tuple(i for i, (a, b) in enumerate(zip(g_value.shape, pad)) if b == 1 and a != 1)
    g_value = g_value.sum(axis=axes, keepdims=True).reshape(vshape)          # row sum (and the sum inside a row)
    return narrow(g_value, dtype), narrow(g_raw.reshape(cot.shape) * 2.0, dtype)


def test_fixture_file_is_data_only_and_small():
    assert os.path.getsize(GOLDEN) < 1_000_000
    assert len(CASES) >= 100
    kinds = {str(f['kind']) for f in CASES.values()}
    forms = {str(f['form']) for f in CASES.values()}
    dtypes = {str(f['dtype']) for f in CASES.values()}
    assert kinds == set('CLPR') and dtypes == {'fp32', 'fp64', 'bf16', 'fp16'}
    assert forms == {'pair', 'pair2d', 'zkey', 'zkeyL', 'flat', 'int32', 'mask', 'tensorZ'}
    widths = {int(np.prod(f['base'].shape[2 if str(f['kind']) in 'LR' else 1:], dtype=np.int64)) * f['base'].dtype.itemsize
              for f in CASES.values()}
    assert {4, 8, 20, 24, 500, 1024} <= widths
    assert any(f['base'].ndim == 1 for f in CASES.values())                  # a 1-D payload
    assert any((f['lens'] == 0).any() for f in CASES.values())               # a batch with an empty sequence
    assert any(str(f['form']) == 'flat' and (f['idx'] < 0).any() for f in CASES.values())
    assert any(not int(f['unique']) for f in CASES.values())                 # repeated rows in the gradient cases


@pytest.mark.parametrize('case', sorted(CASES))
def test_numpy_restatement_reproduces_the_reference(case):
    f = CASES[case]
    g_value, g_base = restate(f)
    assert g_value.dtype == f['grad_value'].dtype and g_value.shape == f['grad_value'].shape
    assert g_value.tobytes() == f['grad_value'].tobytes(), 'gradient w.r.t. the value'
    assert g_base.tobytes() == f['grad_base'].tobytes() or np.array_equal(g_base, f['grad_base']), 'gradient w.r.t. the base'
    if int(f['unique']):                                                     # the written storage, where it is defined
        dtype = str(f['dtype'])
        lead_dims = 2 if str(f['kind']) in 'LR' else 1
        out = widen(f['base'], dtype) * 2.0
        hidden = out.shape[lead_dims:]
        rows = out.reshape((-1,) + hidden)
        rows[f['flat'].reshape(-1)] = np.broadcast_to(widen(f['value'], dtype), f['flat'].shape + hidden).reshape((-1,) + hidden)
        assert np.array_equal(narrow(rows.reshape(out.shape), dtype), f['out'])


# ---- the C ABI
def test_header_table_and_library_agree_on_the_new_symbol():
    text = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+rua_setitem_backward\s*\(', text), 'include/rua.h does not declare rua_setitem_backward'
    assert 'rua_setitem_backward' in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'rua_setitem_backward'), 'librua_hip.so does not export it'
    assert _lib.load().rua_abi_version() == 6                                # additive: the ABI number did not move


def _layouts(m=3, n=8):
    keys = (ctypes.c_int64 * max(m, 1))(*range(max(m, 1)))                   # never dereferenced: the calls below are refused first
    lst = _lib.RuaLayout(kind=_lib.LIST, n_rows=m, B=0, tptr=ctypes.addressof(keys))
    src = _lib.RuaLayout(kind=_lib.LEFT, n_rows=n, B=1, T_phys=n, T_log=n, len_add=n)
    return keys, lst, src


def test_bad_arguments_come_back_without_touching_a_gpu():
    lib = _lib.load()
    EINVAL = -1
    keys, lst, src = _layouts()
    grad, gv, gr = 0x1000, 0x2000, 0x3000                                    # stand-ins for device pointers

    def call(l, s, g, v, r, rb=16, flags=0):
        return lib.rua_setitem_backward(ctypes.byref(l) if l is not None else None, ctypes.byref(s) if s is not None else None,
                                        g, v, r, rb, flags, None)

    assert call(lst, src, grad, gv, grad) == EINVAL                          # grad_raw aliases grad
    assert call(lst, src, None, gv, gr) == EINVAL                            # no grad, M > 0
    assert call(lst, src, None, gv, None) == EINVAL
    assert call(lst, src, grad, gv, gr, rb=-16) == EINVAL                    # negative row size
    not_list = _lib.RuaLayout(kind=_lib.CAT, n_rows=3, B=1, len_add=3)
    assert call(not_list, src, grad, gv, gr) == EINVAL                       # `list` must be a LIST layout
    assert call(src, src, grad, gv, gr) == EINVAL
    assert call(lst, lst, grad, gv, gr) == EINVAL                            # ... and `src` must not be one
    assert call(None, src, grad, gv, gr) == EINVAL and call(lst, None, grad, gv, gr) == EINVAL
    no_keys = _lib.RuaLayout(kind=_lib.LIST, n_rows=3, B=0)
    assert call(no_keys, src, grad, gv, gr) == EINVAL                        # a LIST of 3 entries without token pointers
    assert call(lst, src, grad, gv, gr, flags=1 << 20) == EINVAL             # an unknown flag
    # nothing to do is not an error: no outputs asked for, rows of no bytes
    assert call(lst, src, grad, None, None) == 0
    assert call(lst, src, grad, gv, gr, rb=0) == 0
    del keys
