"""The surface of pack(keep_sums=...) that needs no GPU: the argument is validated before anything touches a device,
the mover's plan still answers as before for the north-star call (the routing sits above it), the new entry points refuse
null and misaligned pointers with the documented codes before any launch, and their host-side plan header survives a
walk under ASan + UBSan as a stand-alone program."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
THERE = 0x1000                       # a stand-in device pointer: never dereferenced by a refused call


@pytest.mark.parametrize('bad', [1, 0, 'yes', 1.0, [True]])
def test_keep_sums_is_none_true_or_false(bad):
    c = ta.C(torch.zeros(3, 8), torch.tensor([1, 2]))
    with pytest.raises(TypeError, match='keep_sums'):
        c.pack(keep_sums=bad)


@pytest.mark.parametrize('ok', [None, True, False])
def test_a_valid_keep_sums_reaches_the_device_check(ok):
    c = ta.C(torch.zeros(3, 8), torch.tensor([1, 2]))
    with pytest.raises(K.RuaError, match='MI355X'):          # a host tensor: there is no CPU path, with or without sums
        c.pack(keep_sums=ok)


def test_the_header_declares_what_the_binding_loads():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    for name in ('rua_pack_sums', 'rua_pack_sums_backward', 'rua_sums_cast'):
        assert re.search(r'\bint\s+%s\(' % name, header) and name in K.SYMBOLS
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header) and K.load().rua_abi_version() == 6      # additive


def test_the_movers_plan_answers_as_before_at_the_north_star():
    """The routing sits above the mover's plan: asked for the north-star pack (65 536 sequences, 17 046 960 rows of
    1 KiB, C -> P) rua_debug_move_plan still names the kernel bench.py's roofline names, in the XCD-span geometry."""
    dst, src = K.RuaLayout(), K.RuaLayout()
    n, B, T = 17046960, 65536, 512
    dst.kind, dst.n_rows, dst.B, dst.T = K.PACK, n, B, T
    dst.lens = dst.boff = dst.sorted = dst.unsorted = dst.bsz = THERE
    src.kind, src.n_rows, src.B = K.CAT, n, B
    src.lens = src.off = THERE
    buf = ctypes.create_string_buffer(512)
    rc = K.load().rua_debug_move_plan(dst, src, 0, 0, 1 << 20, 1 << 21, 1024, -1, 0, buf, 512)
    assert rc > 0, rc
    tiles = -(-n // 16)
    per_xcd = -(-tiles // 8)
    assert buf.raw[:rc].decode() == (f'move_rows_kernel VEC=16 SCATTER=0 NT=1 RPT=1 TROWS=16 TAIL8=0 grid={per_xcd * 8} '
                                     f'per_xcd={per_xcd} lpr=64 lp_log2=6 cpr=1')


def _layouts(B=4):
    src, pack = K.RuaLayout(), K.RuaLayout()
    src.kind, src.B, src.n_rows, src.len_add = K.CAT, B, 10, 1
    pack.kind, pack.B, pack.n_rows, pack.T, pack.boff = K.PACK, B, 10, 3, THERE
    return src, pack


def test_pack_sums_refuses_before_launching():
    lib = K.load()
    src, pack = _layouts()
    bf16, f32, f64 = K.DTYPES[torch.bfloat16], K.DTYPES[torch.float32], K.DTYPES[torch.float64]
    s, p = ctypes.byref(src), ctypes.byref(pack)
    call = lib.rua_pack_sums
    assert call(None, p, THERE, THERE, THERE, 64, bf16, 0, None, None) == EINVAL
    assert call(s, None, THERE, THERE, THERE, 64, bf16, 0, None, None) == EINVAL
    for null in range(3):
        ptrs = [THERE] * 3
        ptrs[null] = None
        assert call(s, p, *ptrs, 64, bf16, 0, None, None) == EINVAL
    assert call(s, p, THERE, THERE, THERE, 64, f64, 0, None, None) == EINVAL        # fp32 accumulators only
    assert call(s, p, THERE, THERE, THERE, -1, bf16, 0, None, None) == EINVAL
    for off in range(3):                                                            # a pointer off 16 bytes
        ptrs = [THERE] * 3
        ptrs[off] = THERE + 8
        assert call(s, p, *ptrs, 64, bf16, 0, None, None) == EALIGN
    assert call(s, p, THERE, THERE, THERE, 68, bf16, 0, None, None) == EALIGN       # 136-byte rows
    assert call(s, p, THERE, THERE, THERE, 6, f32, 0, None, None) == EALIGN
    other = _layouts(5)[1]
    assert call(s, ctypes.byref(other), THERE, THERE, THERE, 64, bf16, 0, None, None) == EINVAL
    src.kind = K.PACK
    assert call(s, p, THERE, THERE, THERE, 64, bf16, 0, None, None) == EINVAL


def test_pack_sums_backward_and_cast_refuse_before_launching():
    lib = K.load()
    src, pack = _layouts()
    s, p = ctypes.byref(src), ctypes.byref(pack)
    f32, bf16 = K.DTYPES[torch.float32], K.DTYPES[torch.bfloat16]
    bwd = lib.rua_pack_sums_backward
    for null in range(3):
        ptrs = [THERE] * 3
        ptrs[null] = None
        assert bwd(s, p, *ptrs, 64, f32, None) == EINVAL
    for off in range(3):
        ptrs = [THERE] * 3
        ptrs[off] = THERE + 4
        assert bwd(s, p, *ptrs, 64, f32, None) == EALIGN
    assert bwd(s, p, THERE, THERE, THERE, 6, f32, None) == EALIGN
    assert bwd(s, p, THERE, THERE, THERE, 64, K.DTYPES[torch.float64], None) == EINVAL
    cast = lib.rua_sums_cast
    assert cast(None, THERE, 8, bf16, 0, None) == EINVAL and cast(THERE, None, 8, bf16, 0, None) == EINVAL
    assert cast(THERE, THERE, 8, bf16, 0, None) == EINVAL and cast(THERE, THERE + 64, -1, bf16, 0, None) == EINVAL
    assert cast(THERE + 2, THERE + 64, 8, bf16, 0, None) == EALIGN                 # the fp32 side off 4 bytes
    assert cast(THERE, THERE + 65, 8, bf16, 0, None) == EALIGN                     # the bf16 side off 2 bytes
    assert cast(THERE, THERE + 64, 0, bf16, 0, None) == 0                          # nothing to do


def test_the_plan_header_under_host_sanitizers(tmp_path):
    """rua_pack_sums_plan.h is plain host C++: tests/c/pack_sums_plan_host.cpp includes it alone and walks the checks
    and the adjoint's grid up to B = 2^40 and H = 2^24 under ASan + UBSan, as its own program."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'pack_sums_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'pack_sums_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]
