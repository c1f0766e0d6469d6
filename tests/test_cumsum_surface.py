"""Per-sequence cumsum: what can be checked without a GPU — the public surface, the C ABI, and the fixture file itself
(tests/golden/r8_cumsum.npz, written by scripts/gen_golden_cumsum.py from the reference).

The GPU tests hold the kernels to 1e-5 * sum_{s<=t} |x_s| against the reference's stored results.  That bar is reachable
only if the reference itself sits well inside it, so every stored float result is re-checked HERE against a float64
per-sequence torch.cumsum, within 5e-6 of the same sum (half the bar; the kernels have the other half); int64 results
are exact."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r8_cumsum.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16,
          'int64': torch.int64}
ENTRY_POINTS = ('rua_segment_cumsum', 'rua_cumsum_ws_bytes')
HALF_BAR = 5e-6


def draw(seed, n, H, dtype_name):
    """(x, cot) of a fixture case — the definition of scripts/gen_golden_cumsum.py, repeated."""
    g = torch.Generator().manual_seed(int(seed))
    shape = (n,) if H == 0 else (n, H)
    if dtype_name == 'int64':
        return torch.randint(-1000, 1001, shape, generator=g, dtype=torch.int64), None
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    x = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    cot = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    return x, cot


def seg_cumsum(v, lens, reverse):
    """per-sequence torch.cumsum of a cat-form payload, in the dtype of `v` (the suffix sums with `reverse`)."""
    out = []
    for piece in torch.split(v, lens.tolist(), dim=0):
        out.append(piece.flip(0).cumsum(0).flip(0) if reverse else piece.cumsum(0))
    return torch.cat(out) if out else v.clone()


_CASES = None


def load_cases():
    """The fixtures, loaded once and shared (nobody modifies them)."""
    global _CASES
    if _CASES is not None:
        return _CASES
    z = np.load(GOLDEN)
    out = {}
    for name in sorted(set(k.split('/')[0] for k in z.files)):
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['H'], c['seed'], c['dtype'] = int(c['H']), int(c['seed']), str(c['dtype'])
        c['lens'] = torch.from_numpy(c['lens'].astype(np.int64))
        c['x'], c['cot'] = draw(c['seed'], int(c['lens'].sum()), c['H'], c['dtype'])
        for k in ('y', 'yrev', 'gx', 'gxrev'):
            if k in c:
                c[k] = torch.from_numpy(c[k])
        out[name] = c
    _CASES = out
    return out


def test_public_names_exist():
    """The two free functions, from the package and from its module, and the method on each of C / L / P / R."""
    import importlib
    mod = importlib.import_module('torchrua_amd.cumsum')
    for name in ('segment_cumsum', 'cumsum'):
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.cumsum is ta.cumsum, cls
    from torchrua_amd import _ops
    assert callable(_ops.launch_cumsum) and issubclass(_ops._Cumsum, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import cumsum, segment_cumsum; '
            'from torchrua.cumsum import segment_cumsum as s2; '
            'assert cumsum is ta.cumsum and s2 is ta.segment_cumsum and callable(torchrua.cumsum); print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    x, sizes = torch.randn(7, 3), torch.tensor([3, 4])
    for reverse in (False, True):
        with pytest.raises(ta.RuaError):
            ta.segment_cumsum(x, sizes, reverse=reverse)
    with pytest.raises(ta.RuaError):
        ta.segment_cumsum(torch.arange(7), sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        with pytest.raises(ta.RuaError):
            z.cumsum()
        with pytest.raises(ta.RuaError):
            ta.cumsum(z, reverse=True)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    # argument checks need no device: a null layout, a dtype the scan does not take
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    assert lib.rua_segment_cumsum(None, 8, 8, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_cumsum(lay, 8, 8, 1, _lib.I32, 0, None, None) == -1
    assert lib.rua_cumsum_ws_bytes(lay, 1, _lib.F32) == 0
    assert lib.rua_cumsum_ws_bytes(lay, 64, _lib.F32) == 0
    # few but long sequences of wide rows: the cut form's workspace — one accumulator per block and padded column:
    # B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * accumulator bytes
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_cumsum_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * 4
    assert lib.rua_cumsum_ws_bytes(long_lay, 64, _lib.I64) == 2 * blocks * 4 * 16 * 8
    assert lib.rua_cumsum_ws_bytes(long_lay, 2, _lib.I64) == 0           # rows of one vector are never cut


def test_fixture_file_loads():
    assert os.path.getsize(GOLDEN) < 1_000_000
    cases = load_cases()
    assert {c['H'] for c in cases.values()} >= {0, 1, 3, 8, 64, 250, 512}
    assert {c['dtype'] for c in cases.values()} == set(DTYPES)
    lengths = set()
    for c in cases.values():
        lengths |= set(c['lens'].tolist())
    assert lengths >= {0, 1, 31, 32, 33, 63, 64, 65, 255, 257, 2047, 2048, 2049}
    assert any(c['lens'].numel() == 2 and int(c['lens'].min()) > 4 * 2048 for c in cases.values())
    for name, c in cases.items():
        for k in ('y', 'yrev') + (() if c['dtype'] == 'int64' else ('gx', 'gxrev')):
            assert c[k].shape == c['x'].shape, (name, k)
            if c['dtype'] != 'int64':
                assert bool(torch.isfinite(c[k]).all()), (name, k)


def test_reference_results_are_within_half_the_bar_of_float64():
    worst = {'fwd': 0.0, 'grad': 0.0}
    for name, c in load_cases().items():
        lens, x = c['lens'], c['x']
        for reverse, ykey, gkey in ((False, 'y', 'gx'), (True, 'yrev', 'gxrev')):
            if c['dtype'] == 'int64':
                assert torch.equal(c[ykey], seg_cumsum(x, lens, reverse)), f'{name} {ykey}'
                continue
            if x.numel() == 0:
                continue
            cot = c['cot'].double()
            f = ((c[ykey].double() - seg_cumsum(x.double(), lens, reverse)).abs()
                 / seg_cumsum(x.double().abs(), lens, reverse).clamp_min(1e-300)).max().item()
            g = ((c[gkey].double() - seg_cumsum(cot, lens, not reverse)).abs()
                 / seg_cumsum(cot.abs(), lens, not reverse).clamp_min(1e-300)).max().item()
            assert f <= HALF_BAR, f'{name} {ykey}: reference off float64 by {f:.2e} of the prefix sum of |x|'
            assert g <= HALF_BAR, f'{name} {gkey}: reference off float64 by {g:.2e} of the suffix sum of |cot|'
            worst['fwd'], worst['grad'] = max(worst['fwd'], f), max(worst['grad'], g)
    print(f'reference vs float64: forward {worst["fwd"]:.2e}, gradient {worst["grad"]:.2e}')
