"""Per-sequence gated linear recurrence: what can be checked without a GPU — the public surface, the C ABI, and the
fixture file itself (tests/golden/r9_linear_scan.npz, written by scripts/gen_golden_linear_scan.py from the reference).

The error bar (shared with tests/test_gpu_linear_scan.py; none of it comes from what the kernels give).  With M_t the
same recurrence evaluated in float64 on (|a|, |x|):

    |got_t - want64_t| <= BAR * M_t          (+ one ulp of the payload dtype for bf16 / f16),   BAR = K * 2^-24

K counts the roundings on the longest path from any x_s to any h_t in the blocked order (rua.h): every combine
(A2 * A1, A2 * B1 + B2) the contribution of x_s passes through rounds three times (the gate product, the product with
the earlier value, the addition).  At the longest sequence tested (8 211 tokens = 5 blocks) the longest path runs from a
token of the first group of the first tile of block 0 to a token of the last block:
      3   doubling steps inside its group
    + 3   group totals of its tile (g0.g1, .g2, .g3)
    + 64  tile totals joining the block's carry, one after the other (the first one joins the identity)
    + 4   block totals joining the base, one after the other
    + 1   base . carry of the last block
    + 1   . the groups before the token
    + 1   . the prefix inside the token's group
    = 77 combines, K = 3 * 77 = 231, BAR = 231 * 2^-24 = 1.38e-5 (the issue's condition: at most 1e-4).
A wrong or lost carry is off by a fraction of M_t, orders of magnitude above that.  float64 is held to the same BAR.
Gradients: dx against the reversed recurrence of (|a|, |cot|) (Mdx); da_t = dx_t * h_(t-1) against
2 * BAR * Mdx_t * Mh_(t-1), plus the ulp term.

Every stored float result of the fixture file is re-checked HERE against an independent float64 per-sequence loop,
within HALF the bar (the kernels have the other half)."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import torchrua_amd as ta
from torchrua_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'r9_linear_scan.npz')
DTYPES = {'fp32': torch.float32, 'fp64': torch.float64, 'bf16': torch.bfloat16, 'fp16': torch.float16}
ENTRY_POINTS = ('rua_linear_scan_ws_bytes', 'rua_segment_linear_scan', 'rua_segment_linear_scan_backward')
K_ROUNDINGS = 3 * (3 + 3 + 64 + 4 + 1 + 1 + 1)
BAR = K_ROUNDINGS * 2.0 ** -24
assert K_ROUNDINGS == 231 and BAR <= 1e-4


def draw(seed, n, H, dtype_name):
    """(x, gate, cot) of a fixture case — the ONE definition (scripts/gen_golden_linear_scan.py imports it): randn
    payload and cotangent, gates +-exp(0.02 * randn) with about a quarter negative, all rounded to the case's dtype and
    held in the reference's working dtype."""
    g = torch.Generator().manual_seed(int(seed))
    shape = (n,) if H == 0 else (n, H)
    work = torch.float64 if dtype_name == 'fp64' else torch.float32
    x = torch.randn(shape, generator=g, dtype=work)
    mag = torch.exp(0.02 * torch.randn(shape, generator=g, dtype=work))
    sign = torch.where(torch.rand(shape, generator=g, dtype=work) < 0.25, -1.0, 1.0).to(work)
    cot = torch.randn(shape, generator=g, dtype=work)
    return tuple(v.to(DTYPES[dtype_name]).to(work) for v in (x, sign * mag, cot))


def _pieces(lens):
    off = 0
    for n in (lens.tolist() if hasattr(lens, 'tolist') else list(lens)):
        yield off, int(n)
        off += int(n)


def scan64(x, a, lens, reverse):
    """The recurrence of every sequence of a cat-form float64 numpy payload, one token after the other; `a` is an array
    of the same shape or a number.  h_0 = x_0 (the gate at scan position 0 is not looked at)."""
    x = np.asarray(x, dtype=np.float64)
    arr = isinstance(a, np.ndarray)
    out = np.empty_like(x)
    with np.errstate(all='ignore'):
        for off, n in _pieces(lens):
            if not n:
                continue
            xs = x[off:off + n][::-1] if reverse else x[off:off + n]
            gs = (a[off:off + n][::-1] if reverse else a[off:off + n]) if arr else None
            h = np.empty_like(xs)
            h[0] = xs[0]
            for t in range(1, n):
                h[t] = (gs[t] if arr else a) * h[t - 1] + xs[t]
            out[off:off + n] = h[::-1] if reverse else h
    return out


def _shift(v, lens, step):
    """out[t] = v[t + step] inside every sequence (what wraps around is never used by the callers: set to 0)."""
    out = np.zeros_like(v)
    for off, n in _pieces(lens):
        if n > 1:
            if step > 0:
                out[off:off + n - step] = v[off + step:off + n]
            else:
                out[off - step:off + n] = v[off:off + n + step]
    return out


def grads64(a, cot, h, lens, reverse):
    """(dx, da) of sum(h * cot) in float64 from the closed form: dx is the recurrence run the other way with the gate
    of the neighbouring token, da = dx * the neighbouring h (0 at the ignored gate).  `a` a number: da is None."""
    step = -1 if reverse else 1                       # the token the forward scan visits next
    if not isinstance(a, np.ndarray):
        return scan64(cot, a, lens, not reverse), None
    dx = scan64(cot, _shift(a, lens, step), lens, not reverse)
    with np.errstate(all='ignore'):
        da = dx * _shift(h, lens, -step)
    for off, n in _pieces(lens):                      # the ignored gate: exactly 0, whatever dx and h hold
        if n:
            da[off + (n - 1 if reverse else 0)] = 0.0
    return dx, da


def scales64(x, a, cot, lens, reverse):
    """(M, Mdx, Mda): the recurrences on absolute values that the bounds scale with."""
    aa = np.abs(a) if isinstance(a, np.ndarray) else abs(a)
    M = scan64(np.abs(x), aa, lens, reverse)
    step = -1 if reverse else 1
    Mdx = scan64(np.abs(cot), _shift(aa, lens, step) if isinstance(a, np.ndarray) else aa, lens, not reverse)
    return M, Mdx, Mdx * _shift(M, lens, -step)


_CASES = None


def load_cases():
    """The fixtures, loaded once and shared (nobody modifies them); float64 references are added lazily by want64()."""
    global _CASES
    if _CASES is not None:
        return _CASES
    z = np.load(GOLDEN)
    out = {}
    for name in sorted(set(k.split('/')[0] for k in z.files)):
        c = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
        c['H'], c['seed'], c['dtype'] = int(c['H']), int(c['seed']), str(c['dtype'])
        c['gamma'] = None if np.isnan(c['gamma']) else float(c['gamma'])
        c['lens'] = torch.from_numpy(c['lens'].astype(np.int64))
        c['x'], c['a'], c['cot'] = draw(c['seed'], int(c['lens'].sum()), c['H'], c['dtype'])
        out[name] = c
    _CASES = out
    return out


def want64(c, reverse):
    """(y, dx, da, M, Mdx, Mda) of a fixture case in float64, computed once per direction and kept."""
    key = f'want64.{int(reverse)}'
    if key not in c:
        x, cot = c['x'].double().numpy(), c['cot'].double().numpy()
        a = c['a'].double().numpy() if c['gamma'] is None else c['gamma']
        y = scan64(x, a, c['lens'], reverse)
        c[key] = (y,) + grads64(a, cot, y, c['lens'], reverse) + scales64(x, a, cot, c['lens'], reverse)
    return c[key]


def test_public_names_exist():
    """The two free functions, from the package and from its module, and the method on each of C / L / P / R."""
    import importlib
    mod = importlib.import_module('torchrua_amd.linear_scan')
    for name in ('segment_linear_scan', 'linear_scan'):
        assert callable(getattr(ta, name)), name
        assert getattr(mod, name) is getattr(ta, name)
        assert name in mod.__all__
    for cls in (ta.C, ta.L, ta.P, ta.R):
        assert cls.linear_scan is ta.linear_scan, cls
    from torchrua_amd import _ops
    assert callable(_ops.launch_linear_scan) and callable(_ops.launch_linear_scan_backward)
    assert callable(_ops.linear_scan) and issubclass(_ops._LinearScan, torch.autograd.Function)


def test_names_resolve_under_the_torchrua_alias():
    code = ('import torchrua_amd as ta; ta.install_as_torchrua(); import torchrua; '
            'from torchrua import linear_scan, segment_linear_scan; '
            'from torchrua.linear_scan import segment_linear_scan as s2; '
            'assert linear_scan is ta.linear_scan and s2 is ta.segment_linear_scan and callable(torchrua.linear_scan); '
            'print("ok")')
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    out = subprocess.run([os.sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


def test_no_cpu_fallback():
    x, a, sizes = torch.randn(7, 3), torch.rand(7, 3), torch.tensor([3, 4])
    for reverse in (False, True):
        with pytest.raises(ta.RuaError):
            ta.segment_linear_scan(x, a, sizes, reverse=reverse)
        with pytest.raises(ta.RuaError):
            ta.segment_linear_scan(x, 0.5, sizes, reverse=reverse)
    p = torch.nn.utils.rnn.pack_sequence([torch.randn(3, 2), torch.randn(2, 2)])
    for z in (ta.C(x, sizes), ta.L(torch.randn(2, 4, 3), sizes), ta.R(torch.randn(2, 4, 3), sizes), p):
        with pytest.raises(ta.RuaError):
            z.linear_scan(0.9)
        with pytest.raises(ta.RuaError):
            z.linear_scan(torch.ones_like(z.data))
        with pytest.raises(ta.RuaError):
            ta.linear_scan(z, z, reverse=True)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'rua.h')).read()
    assert re.search(r'#define\s+RUA_ABI_VERSION\s+6\b', header)
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/rua.h'
        assert name in _lib.SYMBOLS
    lib = _lib.load()                   # (the cross-compiled library; load() resolves every name of the table)
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None
    # argument checks need no device: a null layout, a dtype the scan does not take (no integers), null payloads,
    # an output that aliases the gate, a grad_gate that aliases something that is read
    lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=4, B=1, len_add=4)
    assert lib.rua_segment_linear_scan(None, 8, 16, 0.0, 24, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, 8, 16, 0.0, 24, 1, _lib.I64, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, 8, 16, 0.0, 24, 1, _lib.I32, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, None, 16, 0.0, 24, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, 8, 16, 0.0, None, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, 8, 16, 0.0, 16, 1, _lib.F32, 0, None, None) == -1
    assert lib.rua_segment_linear_scan(lay, 8, 16, 0.0, 24, -1, _lib.F32, 0, None, None) == -1
    bwd = lib.rua_segment_linear_scan_backward
    assert bwd(None, 8, 16, 0.0, 24, 32, 40, 1, _lib.F32, 0, None, None) == -1
    assert bwd(lay, 8, 16, 0.0, 24, 32, 40, 1, _lib.I64, 0, None, None) == -1
    assert bwd(lay, None, 16, 0.0, 24, 32, 40, 1, _lib.F32, 0, None, None) == -1
    for aliased in (8, 16, 24, 32):                    # grad_gate == grad_out / gate / h / grad_x
        assert bwd(lay, 8, 16, 0.0, 24, 32, aliased, 1, _lib.F32, 0, None, None) == -1
    assert bwd(lay, 8, None, 0.5, 24, 32, 40, 1, _lib.F32, 0, None, None) == -1      # a scalar gate has no gradient
    # the cut form's workspace holds an (A, B) PAIR per block and column: twice the cumsum's, on the same layouts
    for H, code in ((1, _lib.F32), (64, _lib.F32)):
        assert lib.rua_linear_scan_ws_bytes(lay, H, code) == 2 * lib.rua_cumsum_ws_bytes(lay, H, code) == 0
    long_lay = _lib.RuaLayout(kind=_lib.CAT, n_rows=40000, B=2, len_add=20000)
    blocks = -(-40000 // 2048)
    assert lib.rua_cumsum_ws_bytes(long_lay, 64, _lib.F32) == 2 * blocks * 2 * 32 * 4
    for H, code in ((64, _lib.F32), (64, _lib.F64), (64, _lib.BF16), (250, _lib.F16), (5, _lib.F32)):
        want = 2 * lib.rua_cumsum_ws_bytes(long_lay, H, code)
        assert want > 0 and lib.rua_linear_scan_ws_bytes(long_lay, H, code) == want, (H, code)
    assert lib.rua_linear_scan_ws_bytes(long_lay, 2, _lib.F64) == 0           # rows of one vector are never cut
    assert lib.rua_linear_scan_ws_bytes(long_lay, 8, _lib.BF16) == 0
    assert lib.rua_linear_scan_ws_bytes(long_lay, 64, _lib.I64) == 0          # no integer types


def test_fixture_file_loads():
    assert os.path.getsize(GOLDEN) < 1_000_000
    cases = load_cases()
    assert {c['H'] for c in cases.values()} >= {0, 1, 3, 8, 64, 250}
    assert {c['dtype'] for c in cases.values()} == set(DTYPES)
    lengths = set()
    for c in cases.values():
        lengths |= set(c['lens'].tolist())
    assert lengths >= {0, 1, 7, 8, 9, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049}
    assert any(int(c['lens'].max()) > 4 * 2048 for c in cases.values())
    assert sum(c['gamma'] is not None for c in cases.values()) >= 3
    for name, c in cases.items():
        keys = ('y', 'yrev', 'gx', 'gxrev') + (('ga', 'garev') if c['gamma'] is None else ())
        for k in keys:
            assert c[k].shape == tuple(c['x'].shape), (name, k)
            assert bool(np.isfinite(c[k]).all()), (name, k)
        assert ('ga' in c) == (c['gamma'] is None)


def test_reference_results_are_within_half_the_bar_of_float64():
    worst = {'fwd': 0.0, 'gx': 0.0, 'ga': 0.0}
    for name, c in load_cases().items():
        if c['x'].numel() == 0:
            continue
        for reverse, ykey, gxkey, gakey in ((False, 'y', 'gx', 'ga'), (True, 'yrev', 'gxrev', 'garev')):
            y, dx, da, M, Mdx, Mda = want64(c, reverse)
            f = (np.abs(c[ykey].astype(np.float64) - y) / np.maximum(BAR * M, 1e-300)).max()
            g = (np.abs(c[gxkey].astype(np.float64) - dx) / np.maximum(BAR * Mdx, 1e-300)).max()
            assert f <= 0.5, f'{name} {ykey}: reference off float64 by {f:.3f} of the bar'
            assert g <= 0.5, f'{name} {gxkey}: reference off float64 by {g:.3f} of the bar'
            worst['fwd'], worst['gx'] = max(worst['fwd'], f), max(worst['gx'], g)
            if c['gamma'] is None:
                h = (np.abs(c[gakey].astype(np.float64) - da) / np.maximum(2 * BAR * Mda, 1e-300)).max()
                assert h <= 0.5, f'{name} {gakey}: reference off float64 by {h:.3f} of the bar'
                worst['ga'] = max(worst['ga'], h)
    print(f'reference vs float64, as a fraction of the bar: forward {worst["fwd"]:.3f}, grad_x {worst["gx"]:.3f}, '
          f'grad_gate {worst["ga"]:.3f}')
