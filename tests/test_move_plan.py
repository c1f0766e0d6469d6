"""The row mover's decision (csrc/rua_move_plan.h) through rua_debug_move_plan: layout structs and payload ADDRESSES only,
no device memory, no launch — safe on any machine.

tests/golden/move_plan_records.json is a fixed battery of rua_move_rows arguments — hand-listed ones (every conversion
the package asks for, at every width the host builds a tile table for, on both sides of every span threshold, every
refusal) and seeded ones picked so that every kernel instantiation occurs — with what the commit BEFORE the plan was
split out of rua_move.hip answered for each: the return code, and the record of the launch it went on to make, taken
from a copy of that commit with one record line in front of every launch (never from the tree under test).  A change of
routing or of a threshold shows up here as a changed line; an intended one re-records the battery the same way.

The second test builds tests/c/move_plan_host.cpp with the host sanitizers: the header alone, walked over sizes no test
could allocate, against the invariants the kernels and the launcher rely on."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from torchrua_amd import _lib as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'move_plan_records.json')
KERNELS = ('move_rows_kernel', 'move_rows_narrow_kernel', 'move_rows_span_kernel', 'seq_copy_kernel', 'pack_tile_lds_kernel',
           'pack_tile_vec_kernel', 'pack_roll_tile_kernel', 'pack_roll_steps_kernel')


def move_plan(dst, src, tmap, tmap_arg, dst_addr, src_addr, row_bytes, pad_row=-1, flags=0):
    """(return code, record) of rua_debug_move_plan; the code is 0 where a record came back."""
    buf = ctypes.create_string_buffer(512)
    rc = K.load().rua_debug_move_plan(dst, src, tmap, tmap_arg, dst_addr, src_addr, row_bytes, pad_row, flags, buf, 512)
    return (0, buf.raw[:rc].decode()) if rc > 0 else (rc, '')


def _battery():
    with open(FIXTURE) as f:
        doc = json.load(f)
    fields = [name for name, _ in K.RuaLayout._fields_]
    assert doc['layout'] == fields
    return [([K.RuaLayout(**dict(zip(fields, lay))) for lay in case[:2]], case[2:9], case[9], case[10]) for case in doc['cases']]


def test_records_are_the_recorded_ones():
    battery = _battery()
    assert len(battery) >= 200
    for n, (lays, args, want_rc, want_rec) in enumerate(battery):
        assert move_plan(*lays, *args) == (want_rc, want_rec), f'case {n}: {args}'


def test_the_battery_covers_every_form_and_every_refusal():
    seen, variants, codes = set(), set(), set()
    for _, _, rc, rec in _battery():
        codes.add(rc if not rec else 'record')
        if rec:
            seen.add(rec.split(' ', 1)[0])
            variants |= {w for w in rec.split() if w in ('RPT=4', 'TAIL8=1', 'SCATTER=1', 'NT=1', 'TO_PACK=0', 'TO_PACK=1', 'R=2', 'R=4', 'R=8')}
            variants.add('span' if ' per_xcd=0' not in rec and 'per_xcd=' in rec else 'plain')
    assert seen == set(KERNELS)
    assert variants == {'RPT=4', 'TAIL8=1', 'SCATTER=1', 'NT=1', 'TO_PACK=0', 'TO_PACK=1', 'R=2', 'R=4', 'R=8', 'span', 'plain'}
    assert codes == {'record', 0, -1, -3}              # nothing to launch, RUA_EINVAL, RUA_ERANGE


def test_the_buffer_is_the_callers():
    lay = K.RuaLayout(kind=K.LEFT, n_rows=4096, B=1, T_phys=4096, T_log=4096, len_add=4096)
    lib = K.load()
    rc, rec = move_plan(lay, lay, K.T_SHIFT, 0, 0x1000, 0x2000, 1024)
    assert rc == 0 and rec.startswith('move_rows_kernel VEC=16 SCATTER=0 NT=0 RPT=1 TROWS=16 TAIL8=0 grid=256 per_xcd=0 ')
    small = ctypes.create_string_buffer(8)
    assert lib.rua_debug_move_plan(lay, lay, K.T_SHIFT, 0, 0x1000, 0x2000, 1024, -1, 0, small, 8) == -3
    assert lib.rua_debug_move_plan(lay, lay, K.T_SHIFT, 0, 0x1000, 0x2000, 1024, -1, 0, None, 0) == -3
    assert small.raw == b'\0' * 8


def test_plan_under_host_sanitizers(tmp_path):
    """rua_move_plan.h is plain host C++: tests/c/move_plan_host.cpp includes it alone and walks plan_move_rows and
    plan_setitem_backward under ASan + UBSan; it fails on a report, on a plan that breaks an invariant (grid within
    1 .. 2^31 - 1, the XCD-span geometry, LDS within 48 KiB, tile rows, R / phase, a (vec, ttl, trl) the launcher has no
    kernel for) and on a form the walk never reached."""
    if not shutil.which('g++'):
        pytest.skip('no g++')
    exe = str(tmp_path / 'move_plan_host')
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                    '-I', os.path.join(ROOT, 'include'), '-I', os.path.join(ROOT, 'torchrua_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'c', 'move_plan_host.cpp'), '-o', exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    if 'unexpected memory mapping' in out.stderr:
        pytest.skip('this kernel\'s address-space layout is one the sanitizer runtime cannot run under')
    assert out.returncode == 0 and 'violations 0' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'ERROR: AddressSanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-4000:]
