"""The cut plan every per-sequence operator shares (csrc/rua_seg_plan.h), through the `*_ws_bytes` entry points the
family exports.  include/rua.h documents the workspace as

    B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * bytes per (block, padded column)

when FEWER than 1 024 (sequence x 128-byte chunk) units have a length bound (CAT: T_log where it is given and below
n_rows, else n_rows; LEFT / RIGHT: T_phys; PACK: T) of AT LEAST 8 192 and a row is wider than one 16-byte vector; 0
otherwise.  `_documented` below is that sentence and nothing else; the entry points must agree with it on every edge of
the rule.  Layout structs only: no device memory, no launch.  The second test builds tests/c/seg_plan_host.cpp with the
host sanitizers and lets it walk the plan and the launch geometry over sizes no test could allocate."""
import os
import shutil
import subprocess

import pytest

from torchrua_amd import _lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESIZE = {K.F32: 4, K.BF16: 2, K.F16: 2, K.F64: 8, K.I64: 8}
FLOATS = (K.F32, K.BF16, K.F16, K.F64)
# operator -> (entry point, the dtypes it takes, accumulators per (block, padded column), extra bytes per column)
OPS = {
    'softmax': ('rua_softmax_ws_bytes', FLOATS, 2, 0),                 # (max, sum)
    'cumsum': ('rua_cumsum_ws_bytes', FLOATS + (K.I64,), 1, 0),        # a block's total
    'argreduce': ('rua_argreduce_ws_bytes', FLOATS + (K.I64,), 1, 8),  # a value and a 64-bit position
    'linear_scan': ('rua_linear_scan_ws_bytes', FLOATS, 2, 0),         # an (A, B) pair
    'norm': ('rua_norm_ws_bytes', FLOATS, 2, 0),                       # (mean, M2)
}
DUMMY = 0x1000        # a non-null pointer the plan never follows (PACK layouts must name their boff)


def _layout(kind, B, bound, t_log=0):
    """A layout of B sequences whose length bound is `bound` (CAT: through n_rows, or through T_log when given)."""
    if kind == K.CAT:
        return K.RuaLayout(kind=K.CAT, n_rows=bound if not t_log else 10 * bound, B=B, len_add=1, T_log=t_log)
    if kind == K.PACK:
        return K.RuaLayout(kind=K.PACK, n_rows=B * bound, B=B, T=bound, boff=DUMMY)
    return K.RuaLayout(kind=kind, n_rows=B * bound, B=B, T_phys=bound, T_log=bound)


def _bound(lay):
    if lay.kind == K.CAT:
        return lay.T_log if 0 < lay.T_log < lay.n_rows else lay.n_rows
    return lay.T if lay.kind == K.PACK else lay.T_phys


def _documented(lay, H, dtype, accs, extra):
    es = ESIZE[dtype]
    chunks = -(-H * es // 128)
    if H * es <= 16 or not lay.B * chunks < 1024 or not _bound(lay) >= 8192:
        return 0
    return lay.B * -(-_bound(lay) // 2048) * chunks * (128 // es) * (accs * (8 if es == 8 else 4) + extra)


def _edges():
    """(layout, H, label) — every edge of the rule, on fp32-sized reasoning but checked for every dtype."""
    cases = []
    for kind in (K.CAT, K.LEFT, K.PACK, K.RIGHT):
        for bound in (8191, 8192, 8193, 40000):                  # the length bound around 4 blocks
            cases.append((_layout(kind, 2, bound), 64, f'kind={kind} bound={bound}'))
        for B in (1023, 1024):                                   # B * n_chunks around 1 024, one chunk per row
            cases.append((_layout(kind, B, 8192), 8, f'kind={kind} B={B} one chunk'))
        for B in (511, 512):                                     # ... and with two chunks per row (fp32: 33 columns)
            cases.append((_layout(kind, B, 8192), 33, f'kind={kind} B={B} two chunks'))
    # a CAT layout with and without T_log: the bound is T_log only where it is given and below n_rows
    cases.append((_layout(K.CAT, 3, 9000, t_log=9000), 40, 'CAT T_log=9000 of 90000 rows'))
    cases.append((_layout(K.CAT, 3, 9000, t_log=8191), 40, 'CAT T_log=8191: below the threshold'))
    cases.append((K.RuaLayout(kind=K.CAT, n_rows=9000, B=3, len_add=1, T_log=20000), 40, 'CAT T_log above n_rows'))
    cases.append((_layout(K.CAT, 3, 9000), 40, 'CAT no T_log'))
    return cases


@pytest.mark.parametrize('op', sorted(OPS))
def test_ws_bytes_is_the_documented_formula(op):
    lib = K.load()
    symbol, dtypes, accs, extra = OPS[op]
    fn = getattr(lib, symbol)
    cut = 0
    for lay, H, label in _edges():
        for dtype in dtypes:
            es = ESIZE[dtype]
            # the row widths around the rule's own edges, in elements of this dtype: 16 and 20 bytes (one vector or
            # more; 24 for 8-byte elements), 128 and 129+ bytes (one chunk and two), and the case's own H
            for h in {16 // es, 16 // es + 1, 128 // es, 128 // es + 1, H}:
                want = _documented(lay, h, dtype, accs, extra)
                assert fn(lay, h, dtype) == want, (op, label, dtype, h)
                cut += want > 0
        refused = K.I64 if K.I64 not in dtypes else K.I32
        assert fn(lay, H, refused) == 0, (op, label, 'a dtype the operator refuses')
        assert fn(lay, 0, K.F32) == 0 and fn(lay, -1, K.F32) == 0
    assert cut > 50                                              # (the edges do exercise the cut side)
    assert fn(None, 64, K.F32) == 0                              # a null layout
    bad = K.RuaLayout(kind=K.PACK, n_rows=40000, B=2, T=20000)   # PACK without boff: not a layout
    assert fn(bad, 64, K.F32) == 0
    assert fn(K.RuaLayout(kind=K.CAT, n_rows=40000, B=0, len_add=1), 64, K.F32) == 0


def test_row_byte_edges_by_hand():
    """The edges spelled out once, so that a slip shared by the formula above and the header cannot hide."""
    lib = K.load()
    lay = _layout(K.CAT, 2, 40000)
    blocks = 20                                                  # ceil(40000 / 2048)
    assert lib.rua_cumsum_ws_bytes(lay, 4, K.F32) == 0                           # 16 bytes: one vector, never cut
    assert lib.rua_cumsum_ws_bytes(lay, 5, K.F32) == 2 * blocks * 1 * 32 * 4     # 20 bytes: one chunk
    assert lib.rua_cumsum_ws_bytes(lay, 32, K.F32) == 2 * blocks * 1 * 32 * 4    # 128 bytes: one chunk
    assert lib.rua_cumsum_ws_bytes(lay, 33, K.F32) == 2 * blocks * 2 * 32 * 4    # 132 bytes: two
    assert lib.rua_norm_ws_bytes(lay, 33, K.BF16) == 2 * blocks * 1 * 64 * 2 * 4
    assert lib.rua_norm_ws_bytes(lay, 33, K.BF16 | K.NORM_MEAN_ACC) == 2 * blocks * 1 * 64 * 2 * 4
    assert lib.rua_cumsum_ws_bytes(_layout(K.LEFT, 2, 8191), 64, K.F32) == 0
    assert lib.rua_cumsum_ws_bytes(_layout(K.LEFT, 2, 8192), 64, K.F32) == 2 * 4 * 2 * 32 * 4
    assert lib.rua_cumsum_ws_bytes(_layout(K.PACK, 1023, 8192), 32, K.F32) == 1023 * 4 * 1 * 32 * 4
    assert lib.rua_cumsum_ws_bytes(_layout(K.PACK, 1024, 8192), 32, K.F32) == 0


def test_relations_between_the_operators():
    lib = K.load()
    for lay, H, label in _edges():
        for dtype in FLOATS + (K.I64,):
            acc = 8 if ESIZE[dtype] == 8 else 4
            cs = lib.rua_cumsum_ws_bytes(lay, H, dtype)
            assert lib.rua_argreduce_ws_bytes(lay, H, dtype) * acc == cs * (8 + acc), (label, dtype)
            if dtype == K.I64:
                continue
            sm = lib.rua_softmax_ws_bytes(lay, H, dtype)
            assert lib.rua_norm_ws_bytes(lay, H, dtype) == sm, (label, dtype)
            assert sm == 2 * cs, (label, dtype)
            assert lib.rua_linear_scan_ws_bytes(lay, H, dtype) == 2 * cs, (label, dtype)


def test_plan_and_launch_geometry_under_host_sanitizers(tmp_path):
    """rua_seg_plan.h is plain host C++: tests/c/seg_plan_host.cpp includes it alone and walks seg_make_plan, the rows
    grid and the lanes geometry up to n_rows = 2^40, H = 2^20 and B = 2^31, every kind, under ASan + UBSan; it fails on a
    report and on a plan whose workgroups would not fit the grid the launchers compute."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'seg_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'seg_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]
