"""attention_decode over a float8_e4m3fn cache on the GPU, against the float64 yardsticks of attention_decode fed the
DEQUANTISED cache (k8.double() * k_scale, v8.double() * v_scale) with q's dtype.  `run`, the masks' keywords, the draws
and the QL / KL edge lists are test_gpu_attention_decode.py's; draws are quantised on the CPU with scale = amax / 448 per
kv head, so nothing overflows to NaN.

BOUNDS.  Dequantisation is exact, so with power-of-two scales (both folds exact) the bound is attention_decode's own:
b_out + merge_term(n_split) A, and lse_reference's.  With other scales (`exact=False`) the kernel rounds the score scale
twice more — fl(k_scale[hk] * by_value), then fl(scale * that) — and the merged accumulator once more:
  * every score of one (sequence, head) is off by the SAME factor 1 + d, |d| <= 2 e (1.01 covers e^2).  A normalised
    weight exp(s_s) / sum_j exp(s_j) then moves by exp(d s_s) / sum_j p_j exp(d s_j), which lies within exp(+-2 |d| smax)
    for smax >= every |s|: numerator and normaliser each move by at most exp(|d| smax).  So out moves by at most
    (exp(4 e smax) - 1) A, and lse — 1-Lipschitz in the scores — by at most 2 e smax;
  * the v_scale multiply is one fp32 rounding of a sum of magnitude at most A: e A.
smax is taken as the largest |scaled score| over ALL (query, key) pairs of the case, hidden ones included: an upper bound
that needs no mask."""
import math

import pytest
import torch

from torchrua_amd import _meta, _ops
import attention_band_util as U
import attention_decode_util as DU
from test_gpu_attention import KINDS
from test_gpu_attention_decode import KL, QL, draw_case, kw, run

pytestmark = pytest.mark.gpu
E4M3, DEV = torch.float8_e4m3fn, 'cuda'


def quantise(x, pow2):
    """(codes [N, heads_kv, D], scale float32 [heads_kv]) with scale = amax / 448, rounded up to a power of two or as is."""
    s = x.float().abs().amax((0, 2)) / 448
    s = torch.exp2(torch.ceil(torch.log2(s))) if pow2 else s
    return (x.float() / s[None, :, None]).to(E4M3), s


def deq(x8, s):
    """float64 [N, heads_kv, D]: float(code) * scale[hk]; `s` is None, a number or a [heads_kv] tensor."""
    s = torch.ones(x8.size(1)) if s is None else torch.as_tensor(s, dtype=torch.float32).expand(x8.size(1))
    return x8.float().double() * s.double()[None, :, None]


def on_dev(s):
    return s.to(DEV) if isinstance(s, torch.Tensor) else s


def check(key, got, q, qlens, k8, ks, v8, vs, klens, mask, dtype, kv_chunk, exact=True):
    """out and lse within the bounds of the module docstring; dead queries: exact zeros and -inf.  Returns `dead`."""
    kd, vd = deq(k8, ks), deq(v8, vs)
    n_split = _ops.attention_decode_plan(len(qlens), q.size(1), k8.size(1), q.size(2), max(qlens), max(klens), kv_chunk)[1]
    (want, *_), (b_out, *_), A = U.reference(q, qlens, kd, vd, klens, torch.zeros_like(q), mask, None, dtype)
    b_out = b_out + DU.merge_term(n_split) * A * (b_out > 0)
    lse, b_lse = DU.lse_reference(q, qlens, kd, klens, mask, None, n_split)
    dead = torch.isinf(lse)
    if not exact:
        smax = q.size(2) ** -0.5 * max(float(torch.einsum('thd,shd->ths', a.double().abs(), b.abs().repeat_interleave(q.size(1) // b.size(1), 1)).max())
                                       for a, b in zip(q.split(qlens), kd.split(klens)) if a.numel() and b.numel())
        b_out = b_out + 1.01 * (math.expm1(4 * U.E * smax) + U.E) * A * (b_out > 0)
        b_lse = b_lse + 1.01 * 2 * U.E * smax * ~dead
    U.check(f'decode fp8 {key} out', got[0], want, b_out)
    assert bool((got[1][dead] == -float('inf')).all()) and not got[0][dead.any(1)].any()
    U.check(f'decode fp8 {key} lse', got[1].masked_fill(dead, 0.0), lse.masked_fill(dead, 0.0), b_lse)
    return dead


def case(qlens, klens, heads, D, dtype, seed, pow2=True):
    q, k, v = draw_case(qlens, klens, heads, D, dtype, seed)
    return (q, *quantise(k, pow2), *quantise(v, pow2))


def go(kinds, q, qlens, k8, ks, v8, vs, klens, **kwargs):
    return run(kinds, q, qlens, k8, v8, klens, k_scale=on_dev(ks), v_scale=on_dev(vs), **kwargs)


@pytest.mark.parametrize('kv_chunk', [None, 128])
@pytest.mark.parametrize('mask', [('end', 40, 0), ('start', 33, 7)], ids=str)
@pytest.mark.parametrize('heads', [(4, 2), (8, 1)], ids=str)
@pytest.mark.parametrize('dtype', [U.BF16, U.F16], ids=str)
@pytest.mark.parametrize('D', [32, 64, 128])
def test_tile_and_split_edges(D, dtype, heads, mask, kv_chunk):
    q, k8, ks, v8, vs = case(QL, KL, heads, D, dtype, 10 * D)
    got = go('LC' if D == 32 else 'CC', q, QL, k8, ks, v8, vs, KL, kv_chunk=kv_chunk, **kw(*mask))
    key = f'{str(dtype)[6:]} D={D} heads={heads[0]}/{heads[1]} {mask[0]} {mask[1]} {mask[2]} chunk={kv_chunk}'
    assert bool(check(key, got, q, QL, k8, ks, v8, vs, KL, mask, dtype, kv_chunk).any())


@pytest.mark.parametrize('dtype', [U.BF16, U.F16], ids=str)
@pytest.mark.parametrize('D', [32, 64, 128])
def test_all_256_codes(D, dtype):
    """Every code in every byte position of a load, in K and in V; the reference is torch's CPU decode of the same bytes.
    An fnuz decode is off by a factor 2 and by its NaN code."""
    T, S = 2, 256
    codes = ((torch.arange(S)[:, None] + torch.arange(D)[None, :]) % 256).to(torch.uint8)
    codes[(codes == 0x7F) | (codes == 0xFF)] = 0
    k8 = codes[:, None, :].contiguous().view(E4M3)
    q = U.draw([T], 2, D, dtype, 256 + D)
    got = go('CC', q, [T], k8, 2.0 ** -9, k8.clone(), 2.0 ** -4, [S], kv_chunk=128)
    check(f'codes {str(dtype)[6:]} D={D}', got, q, [T], k8, 2.0 ** -9, k8, 2.0 ** -4, [S], ('end', None, 0), dtype, 128)


def test_all_sixteen_pairs_of_layouts_give_the_same_bits(monkeypatch):
    PQ, PK = [30, 0, 5, 32], [131, 3, 0, 129]
    q, k8, ks, v8, vs = case(PQ, PK, (4, 2), 32, U.F16, 7)
    calls, real = [], _meta._read_back
    monkeypatch.setattr(_meta, '_read_back', lambda t: (calls.append(tuple(t.shape)), real(t))[1])
    base = go('CC', q, PQ, k8, ks, v8, vs, PK, kv_chunk=128)
    check('pairs', base, q, PQ, k8, ks, v8, vs, PK, ('end', None, 0), U.F16, 128)
    for pair in [a + b for a in KINDS for b in KINDS]:           # run() asserts the zero padding rows of every L / R
        for got, exp, what in zip(go(pair, q, PQ, k8, ks, v8, vs, PK, kv_chunk=128), base, ('out', 'lse')):
            assert torch.equal(got, exp), (pair, what)
    assert calls == [], calls                                   # host lengths: nothing is read back


def test_scale_forms():
    ql, kl, dtype = [1, 3], [200, 131], U.BF16
    q, k8, ks, v8, vs = case(ql, kl, (4, 2), 64, dtype, 21, pow2=False)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))    # noqa: E731
    one = lambda s: go('CC', q, ql, k8, s, v8, s, kl, kv_chunk=128)     # noqa: E731
    assert same(one(None), one(1.0)) and same(one(None), one(torch.ones(2)))
    assert same(one(0.37), one(torch.full((2,), 0.37)))
    assert not same(one(None), one(0.37))
    got = go('CC', q, ql, k8, ks, v8, vs, kl, kv_chunk=128)
    check('amax / 448 as it comes', got, q, ql, k8, ks, v8, vs, kl, ('end', None, 0), dtype, 128, exact=False)
    got = go('CC', q, ql, k8, 0.37, v8, torch.tensor([0.6, 1.7]), kl, kv_chunk=128)
    check('a number and a tensor', got, q, ql, k8, 0.37, v8, torch.tensor([0.6, 1.7]), kl, ('end', None, 0), dtype, 128, exact=False)


def test_a_split_walks_several_steps():
    ql, kl = [4, 1, 2], [700, 385, 5]
    q, k8, ks, v8, vs = case(ql, kl, (8, 2), 64, U.BF16, 33)
    got = go('CC', q, ql, k8, ks, v8, vs, kl, kv_chunk=384)
    check('walk chunk=384', got, q, ql, k8, ks, v8, vs, kl, ('end', None, 0), U.BF16, 384)


def test_a_bf16_cache_through_the_new_signature_keeps_its_bits():
    q, k, v = draw_case(QL, KL, (4, 2), 64, U.BF16, 640)
    old = run('CC', q, QL, k, v, KL, kv_chunk=128)
    new = run('CC', q, QL, k, v, KL, kv_chunk=128, k_scale=None, v_scale=None)
    assert all(torch.equal(a, b) for a, b in zip(old, new))
