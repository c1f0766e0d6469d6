"""Per-sequence softmax / log_softmax: what can be checked without a GPU — the public surface, the C ABI, and the
fixture file itself (tests/golden/r7_softmax.npz, written by scripts/gen_golden_softmax.py from the reference).

The GPU tests hold the kernels to 1e-5 against the reference's stored results.  That bar is reachable only if the
reference itself sits well inside it, so every stored result is re-checked HERE against a float64 per-sequence
torch.softmax / torch.log_softmax, within 5e-6 (half the bar; the kernels have the other half)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r7_softmax.npz')
FUNCTIONS = ('segment_softmax', 'segment_log_softmax', 'softmax', 'log_softmax')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
HALF_BAR = 5e-6


def draw(seed, n, H, dtype_name, scale):
    """(x, cot) of a fixture case — the definition of scripts/gen_golden_softmax.py, repeated (stored inputs, where a
    case has them, must agree with it)."""
    g = torch.Generator().manual_seed(int(seed))
    shape = (n,) if H == 0 else (n, H)
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    x = (torch.randn(shape, generator=g, dtype=work) * scale).to(DTYPES[dtype_name]).to(work)
    cot = torch.randn(shape, generator=g, dtype=work).to(DTYPES[dtype_name]).to(work)
    return x, cot


def load_cases():
    z = np.load(GOLDEN)
    names = sorted(set(k.split('/')[0] for k in z.files))
    out = {}
    for name in names:
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['H'], c['seed'], c['scale'], c['dtype'] = int(c['H']), int(c['seed']), float(c['scale']), str(c['dtype'])
        c['lens'] = torch.from_numpy(c['lens'].astype(np.int64))
        x, cot = draw(c['seed'], int(c['lens'].sum()), c['H'], c['dtype'], c['scale'])
        if 'x' in c:
            assert np.array_equal(c['x'], x.numpy()) and np.array_equal(c['cot'], cot.numpy()), \
                f'{name}: the generator of this torch build does not reproduce the stored inputs'
        c['x'], c['cot'] = x, cot
        for k in ('y', 'ylog', 'gx', 'gxlog'):
            c[k] = torch.from_numpy(c[k])
        out[name] = c
    return out


def test_public_names_exist():
    """The four free functions, from the package and from its module, and the two methods on each of C / L / P / R."""
    import importlib
    mod = importlib.import_module('torchrua_amd.softmax')
    for name in FUNCTIONS:
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.softmax is ta.softmax and cls.log_softmax is ta.log_softmax, cls


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import softmax, log_softmax, segment_softmax, segment_log_softmax; '
            'from torchrua.softmax import segment_softmax as s2; '
            'assert softmax is ta.softmax and s2 is ta.segment_softmax; print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    x, sizes = torch.randn(7, 3), torch.tensor([3, 4])
    with pytest.raises(ta.RuaError):
        ta.segment_softmax(x, sizes)
    with pytest.raises(ta.RuaError):
        ta.segment_log_softmax(x, sizes)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        with pytest.raises(ta.RuaError):
            z.softmax()
        with pytest.raises(ta.RuaError):
            ta.log_softmax(z)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ('rua_segment_softmax', 'rua_segment_softmax_backward', 'rua_softmax_ws_bytes'):
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    for name in ('rua_segment_softmax', 'rua_segment_softmax_backward', 'rua_softmax_ws_bytes'):
        assert getattr(lib, name) is not None
    # argument checks need no device: a null layout, an integer dtype, y aliasing grad_in
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    assert lib.rua_segment_softmax(None, 8, 8, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_softmax(lay, 8, 8, 1, _lib.I64, 0, None, None) == -1
    assert lib.rua_segment_softmax_backward(lay, 64, 128, 64, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_softmax_ws_bytes(lay, 1, _lib.F32) == 0
    # few but long sequences of wide rows: the cut form's workspace — (max, sum) fp32 per block and padded column
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_softmax_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 64 * 2 * 4


def test_fixture_file_loads():
    assert os.path.getsize(GOLDEN) < 1_000_000
    cases = load_cases()
    assert len(cases) >= 24
    hs = {c['H'] for c in cases.values()}
    assert {0, 3, 8, 64, 250, 512} <= hs
    assert {c['dtype'] for c in cases.values()} == set(DTYPES)
    assert any((c['lens'] == 0).any() for c in cases.values())
    assert any(int(c['lens'].max()) > 512 for c in cases.values())
    for name, c in cases.items():
        assert c['scale'] <= 3.0
        for k in ('y', 'ylog', 'gx', 'gxlog'):
            assert c[k].shape == c['x'].shape and bool(torch.isfinite(c[k]).all()), (name, k)


def _seg_sum(v, lens):
    pieces = [p.sum(dim=0) for p in torch.split(v, lens.tolist(), dim=0)]
    return torch.repeat_interleave(torch.stack(pieces), lens, dim=0)


def test_reference_results_are_within_half_the_bar_of_float64():
    worst = {'fwd': 0.0, 'grad': 0.0}
    for name, c in load_cases().items():
        lens, cot = c['lens'], c['cot'].double()
        x64 = c['x'].double().clone().requires_grad_(True)
        ys, yl = [], []
        for piece in torch.split(x64, lens.tolist(), dim=0):
            ys.append(torch.softmax(piece, dim=0))
            yl.append(torch.log_softmax(piece, dim=0))
        y, ylog = torch.cat(ys), torch.cat(yl)
        gx, = torch.autograd.grad((y * cot).sum(), x64, retain_graph=True)
        gxl, = torch.autograd.grad((ylog * cot).sum(), x64)
        y, ylog = y.detach(), ylog.detach()
        f1 = ((c['y'].double() - y).abs() / y).max().item()
        f2 = ((c['ylog'].double() - ylog).abs() / ylog.abs().clamp_min(1.0)).max().item()
        n1 = y * (cot.abs() + _seg_sum((cot * y).abs(), lens))
        n2 = cot.abs() + ylog.exp() * _seg_sum(cot.abs(), lens)
        g1 = ((c['gx'].double() - gx).abs() / n1).max().item()
        g2 = ((c['gxlog'].double() - gxl).abs() / n2).max().item()
        assert max(f1, f2) <= HALF_BAR, f'{name}: reference forward off float64 by {max(f1, f2):.2e}'
        assert max(g1, g2) <= HALF_BAR, f'{name}: reference gradient off float64 by {max(g1, g2):.2e}'
        worst['fwd'], worst['grad'] = max(worst['fwd'], f1, f2), max(worst['grad'], g1, g2)
    print(f'reference vs float64: forward {worst["fwd"]:.2e}, gradient {worst["grad"]:.2e}')
