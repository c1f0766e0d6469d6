"""Per-sequence var_mean / standardize: what can be checked without a GPU — the public surface, the C ABI, and the
fixture file itself (tests/golden/r11_standardize.npz, written by scripts/gen_golden_standardize.py from the reference).

The GPU tests hold the kernels to the bounds of tests/norm_util.py against the reference's stored results.  That is
reachable only if the reference itself sits well inside them, so every stored result is re-checked HERE against a float64
per-sequence evaluation, within half of each bound (the kernels have the other half)."""
import os
import re
import subprocess

import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

import norm_util as U

ROOT = U.ROOT
FUNCTIONS = ('segment_var_mean', 'segment_var', 'segment_standardize', 'var_mean', 'var', 'standardize')
ENTRIES = ('rua_norm_ws_bytes', 'rua_segment_var_mean', 'rua_segment_var_mean_backward', 'rua_segment_standardize',
           'rua_segment_standardize_backward')


def test_public_names_exist():
    """The six free functions, from the package and from its module, and the three methods on each of C / L / P / R."""
    import importlib
    mod = importlib.import_module('torchrua_amd.norm')
    for name in FUNCTIONS:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.var_mean is ta.var_mean and cls.var is ta.var and cls.standardize is ta.standardize, cls


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import standardize, var_mean, var, segment_standardize, segment_var_mean, segment_var; '
            'from torchrua.norm import segment_standardize as s2; '
            'assert standardize is ta.standardize and s2 is ta.segment_standardize and var_mean is ta.var_mean; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    x, sizes = torch.randn(7, 3), torch.tensor([3, 4])
    for fn in (ta.segment_var_mean, ta.segment_var, ta.segment_standardize):
        with pytest.raises(ta.RuaError):
            fn(x, sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        for call in (lambda: z.standardize(), lambda: z.var_mean(), lambda: z.var(), lambda: ta.standardize(z, eps=0.0),
                     lambda: ta.var_mean(z, correction=0), lambda: ta.var(z)):
            with pytest.raises(ta.RuaError):
                call()


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header) and _lib.ABI_VERSION == 6
    for name in ENTRIES:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    assert lib.rua_abi_version() == 6
    for name in ENTRIES:
        assert getattr(lib, name) is not None


def test_argument_checks_need_no_device():
    lib = _lib.load()
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    EINVAL = -1
    # a null layout
    assert lib.rua_segment_var_mean(None, 8, 64, 128, 1, _lib.F32, 1, None, None) == EINVAL
    assert lib.rua_segment_var_mean_backward(None, 8, 64, 128, 192, 256, 1, _lib.F32, 1, None) == EINVAL
    assert lib.rua_segment_standardize(None, 8, 64, 128, 1, _lib.F32, 0, 1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize_backward(None, 8, 64, 128, 192, 1, _lib.F32, 0, None, None) == EINVAL
    # an integer dtype
    assert lib.rua_segment_var_mean(lay, 8, 64, 128, 1, _lib.I64, 1, None, None) == EINVAL
    assert lib.rua_segment_var_mean_backward(lay, 8, 64, 128, 192, 256, 1, _lib.I32, 1, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 8, 64, 128, 1, _lib.I64, 0, 1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize_backward(lay, 8, 64, 128, 192, 1, _lib.U8, 0, None, None) == EINVAL
    # a negative correction, a negative (or NaN) eps
    assert lib.rua_segment_var_mean(lay, 8, 64, 128, 1, _lib.F32, -1, None, None) == EINVAL
    assert lib.rua_segment_var_mean_backward(lay, 8, 64, 128, 192, 256, 1, _lib.F32, -1, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 8, 64, 128, 1, _lib.F32, -1, 1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 8, 64, 128, 1, _lib.F32, 0, -1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 8, 64, 128, 1, _lib.F32, 0, float('nan'), None, None) == EINVAL
    assert lib.rua_segment_standardize_backward(lay, 8, 64, 128, 192, 1, _lib.F32, -2, None, None) == EINVAL
    # aliasing: a [B, H] output on an input or on the other output; y or rstd on grad_in
    assert lib.rua_segment_var_mean(lay, 64, 64, 128, 1, _lib.F32, 1, None, None) == EINVAL
    assert lib.rua_segment_var_mean(lay, 64, 128, 64, 1, _lib.F32, 1, None, None) == EINVAL
    assert lib.rua_segment_var_mean(lay, 64, 128, 128, 1, _lib.F32, 1, None, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 64, 128, 64, 1, _lib.F32, 0, 1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize(lay, 64, 128, 128, 1, _lib.F32, 0, 1e-5, None, None) == EINVAL
    assert lib.rua_segment_standardize_backward(lay, 64, 128, 192, 64, 1, _lib.F32, 0, None, None) == EINVAL
    assert lib.rua_segment_standardize_backward(lay, 64, 128, 192, 128, 1, _lib.F32, 0, None, None) == EINVAL
    assert lib.rua_segment_var_mean_backward(lay, 8, 64, 128, 192, 64, 1, _lib.F32, 1, None) == EINVAL
    assert lib.rua_segment_var_mean_backward(lay, 8, 64, 128, 192, 128, 1, _lib.F32, 1, None) == EINVAL
    # nothing to do: no launch, no error
    none = _lib.RuaLayout(kind=_lib.CAT, n_rows=0, B=0)
    assert lib.rua_segment_standardize(none, None, None, None, 4, _lib.F32, 0, 1e-5, None, None) == 0
    assert lib.rua_segment_var_mean(lay, None, None, None, 0, _lib.F32, 1, None, None) == 0
    assert lib.rua_segment_standardize_backward(lay, None, None, None, None, 0, _lib.BF16, 0, None, None) == 0


def test_workspace_size():
    lib = _lib.load()
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    assert lib.rua_norm_ws_bytes(lay, 1, _lib.F32) == 0 and lib.rua_norm_ws_bytes(lay, 64, _lib.F32) == 0
    assert lib.rua_norm_ws_bytes(None, 64, _lib.F32) == 0
    # few but long sequences of wide rows: the header's formula —
    # B * ceil(bound / 2048) * ceil(H * esize / 128) * (128 / esize) * 2 * sizeof(accumulator)
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_norm_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * 2 * 4
    assert lib.rua_norm_ws_bytes(long_lay, 33, _lib.BF16) == 2 * blocks * 1 * 64 * 2 * 4
    assert lib.rua_norm_ws_bytes(long_lay, 2, _lib.F32) == 0            # rows of one vector are never cut


def test_fixture_file_loads():
    assert os.path.getsize(U.GOLDEN) < 1_000_000
    cases = U.load_cases()
    assert len(cases) >= 23                                             # (the generator's grid has 25: at most 10 % dropped)
    assert {0, 3, 8, 64, 250, 512} <= {c['H'] for c in cases.values()}
    assert {c['dtype'] for c in cases.values()} == set(U.DTYPES)
    assert any((c['lens'] == 0).any() for c in cases.values())
    assert any((c['lens'] == 1).any() for c in cases.values())
    assert any(int(c['lens'].max()) >= 1024 for c in cases.values())
    assert any(c['offset'] != 0 for c in cases.values())
    for name, c in cases.items():
        assert abs(c['offset']) <= 10 * c['scale'], name
        B = c['lens'].numel()
        for k in ('y00', 'y01', 'y10', 'y11', 'gy00', 'gy11', 'gvm0', 'gvm1'):
            assert c[k].shape == c['x'].shape, (name, k)
        for k in ('mean', 'var0', 'var1'):
            assert c[k].shape == (B,) + tuple(c['x'].shape[1:]), (name, k)
        single = torch.repeat_interleave(c['lens'] == 1, c['lens'])
        assert bool(torch.isnan(c['y11'][single]).all()) and bool(torch.isnan(c['gvm1'][single]).all()), name
        assert bool(torch.isnan(c['var1'][c['lens'] <= 1]).all()) and bool(torch.isnan(c['mean'][c['lens'] == 0]).all())


def _ratio(got, want, bound, what):
    """max |got - want| / (bound / 2) where float64 is finite; the NaN masks must agree."""
    fin = torch.isfinite(bound)
    assert torch.equal(torch.isnan(got) | ~fin, ~fin), f'{what}: NaN positions'
    if not bool(fin.any()):
        return 0.0
    e, b = (got.double() - want).abs()[fin], bound[fin] / 2
    assert bool((e[b == 0] == 0).all()), f'{what}: must be exact'
    return float((e / b.clamp_min(1e-300)).max())


def test_reference_results_are_within_half_the_bounds_of_float64():
    worst = {}
    for name, c in U.load_cases().items():
        if int(c['lens'].sum()) == 0:
            continue
        lens, dt = c['lens'], U.DTYPES[c['dtype']]
        ex = U.Exact(c['x'], lens)
        r = {'mean': _ratio(c['mean'], ex.mean, ex.mean_bound(dt), name)}
        for cr in (0, 1):
            r[f'var{cr}'] = _ratio(c[f'var{cr}'], ex.var(cr), ex.var_bound(cr, dt), name)
            want, absdev, kv, km = U.vm_grad(c['x'], ex.mean, c['cv'], c['cm'], lens, cr)
            bound = U.vm_grad_bound(want, absdev, kv, km, ex.mean.abs()[ex.ids], dt, independent=True)
            r[f'gvm{cr}'] = _ratio(c[f'gvm{cr}'], want, bound, name)
        for key, (cr, eps) in U.COMBOS.items():
            r['y' + key] = _ratio(c['y' + key], ex.y(cr, eps), ex.y_bound(cr, eps, dt), name)
        for key in U.GRAD_COMBOS:
            cr, eps = U.COMBOS[key]
            want, norm = U.std_grad(ex.y(cr, eps), ex.rstd(cr, eps), c['cot'], lens, cr)
            rho = (ex.mean.abs() / torch.sqrt(ex.var(0) + eps))[ex.ids]
            r['gy' + key] = _ratio(c['gy' + key], want, U.std_grad_bound(want, norm, dt, rho), name)
        for k, v in r.items():
            assert v <= 1.0, f'{name}: reference {k} at {v:.2f} x half its bound'
            worst[k] = max(worst.get(k, 0.0), v)
    print('reference vs float64, worst error / half bound: ' + ', '.join(f'{k} {v:.2f}' for k, v in sorted(worst.items())))
