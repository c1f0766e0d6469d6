"""Per-sequence causal depthwise convolution: the case builders, the float64 yardstick and the bounds shared by
tests/test_causal_conv_surface.py and tests/test_gpu_causal_conv.py.

The reference library has no convolution: the yardstick is stock torch on the CPU in float64, every sequence on its
own,

    F.conv1d(x_seq.T[None], weight.reshape(K, H).T[:, None, :], bias, padding=K-1, groups=H)[..., :len]

(`reverse`: the sequence flipped, convolved, flipped back).  For bf16 / f16 the wanted value is computed from the
ROUNDED inputs the kernel actually receives.

The bounds are derived, none comes from what the kernels give.  u = 2^-24 is the rounding of the fp32 accumulator
(2^-53 for float64 payloads), and r |y| stands for half a unit in the last place of the output dtype at the wanted
value: 2^-24 |y| for fp32, 2^-53 |y| for fp64, and for bf16 / f16 the exact half ulp at y, 2^(floor(log2 |y|) - 8) and
2^(floor(log2 |y|) - 11) (never below half the smallest subnormal's spacing).  (As a multiple of |y| half an ulp of
bf16 lies between 2^-9 — just below a power of two — and 2^-8 — at one; 2^-12 and 2^-11 for f16.  The flat factors
2^-9 and 2^-12 are half an ulp only at the top of a binade: the CORRECTLY ROUNDED exact result misses them by up to
2 x — 1 + 2^-8 lies 2^-8 from both of its bf16 neighbours — so no kernel could be held to them.)

    forward, grad_input:     |err| <= (K + 1) u (|bias| + sum_k |w_k x|) + r |y|
        the accumulator starts at the bias and takes K fused multiply-adds, each rounded once: K roundings of partial
        sums that are bounded by the sum of absolute values (one more for slack), then the output rounding.
    grad_weight, grad_bias:  |err| <= (n_terms + K) u sum |g x| + r |result|
        the summation bound that holds for ANY order of adding n_terms products (each product and each addition rounds
        once); n_terms = the number of tokens that contribute to the element.
"""
import numpy as np
import torch
import torch.nn.functional as F

F32, BF16, F16, F64 = torch.float32, torch.bfloat16, torch.float16, torch.float64
HALF_ULP = {F32: 2.0 ** -24, F64: 2.0 ** -53}           # as a multiple of |y|; bf16 / f16: half_ulp() below, exact


def acc_u(dtype) -> float:
    return 2.0 ** -53 if dtype == F64 else 2.0 ** -24


def half_ulp(want64: torch.Tensor, dtype) -> torch.Tensor:
    """The r |y| term: half a unit in the last place of `dtype` at the float64 values `want64`."""
    if dtype in HALF_ULP:
        return HALF_ULP[dtype] * want64.abs()
    bits, lowest = (7, -133) if dtype == BF16 else (10, -24)        # explicit significand bits, log2 of the subnormal spacing
    _, e = torch.frexp(want64.abs().clamp_min(2.0 ** -140))         # |y| = m * 2^e, 0.5 <= m < 1
    return torch.ldexp(torch.ones_like(want64), (e - 1 - bits).clamp_min(lowest) - 1)


def batch_lengths(K: int, seed: int = 0) -> torch.Tensor:
    """The lengths every layout test uses, shuffled so that a PackedSequence's sort matters: empty, single, around the
    filter length, around a tile of 32, around a block of 2 048."""
    lens = [0, 1, max(K - 1, 0), K, K + 1, 31, 32, 33, 2047, 2048, 2049]
    order = np.random.RandomState(seed).permutation(len(lens))
    return torch.tensor([lens[i] for i in order], dtype=torch.long)


def draw(shape, dtype, seed: int) -> torch.Tensor:
    """randn rounded to `dtype` (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=F64 if dtype == F64 else F32).to(dtype)


def _pieces(lens):
    off = 0
    for n in (lens.tolist() if hasattr(lens, 'tolist') else list(lens)):
        yield off, int(n)
        off += int(n)


def conv64(x: torch.Tensor, w: torch.Tensor, b, lens, reverse: bool) -> torch.Tensor:
    """The yardstick: a cat-form payload [N, *hidden] (any float dtype, CPU), the filter [K, *hidden] and the bias
    [*hidden] or None -> float64 [N, *hidden]."""
    N, K = x.shape[0], w.shape[0]
    x2, w2 = x.double().reshape(N, -1), w.double().reshape(K, -1)
    H = x2.shape[1]
    b2 = None if b is None else b.double().reshape(H)
    out = torch.zeros_like(x2)
    for off, n in _pieces(lens):
        if not n:
            continue
        seq = x2[off:off + n]
        if reverse:
            seq = seq.flip(0)
        y = F.conv1d(seq.T[None], w2.T[:, None, :], b2, padding=K - 1, groups=H)[0, :, :n].T
        out[off:off + n] = y.flip(0) if reverse else y
    return out.reshape(x.shape)


def conv_bound(x, w, b, lens, reverse: bool, want64: torch.Tensor, dtype) -> torch.Tensor:
    """(K + 1) u (|bias| + sum_k |w_k x|) + r |y|"""
    K = w.shape[0]
    scale = conv64(x.double().abs(), w.double().abs(), None if b is None else b.double().abs(), lens, reverse)
    return (K + 1) * acc_u(dtype) * scale + half_ulp(want64, dtype)


def weight_grads64(g: torch.Tensor, x: torch.Tensor, K: int, lens, reverse: bool):
    """(grad_weight [K, *hidden], grad_bias [*hidden], n_terms [K + 1]) in float64 of sum(y * g) for the convolution
    whose direction is `reverse`: gw[k] = sum_t g[t] * x[the token tap k read]; n_terms[k] counts the tokens that
    contribute (n_terms[K]: the bias, every token)."""
    N = x.shape[0]
    g2, x2 = g.double().reshape(N, -1), x.double().reshape(N, -1)
    gw = torch.zeros((K,) + tuple(x2.shape[1:]), dtype=F64)
    n_terms = [0] * (K + 1)
    for off, n in _pieces(lens):
        if not n:
            continue
        gs, xs = g2[off:off + n], x2[off:off + n]
        if reverse:
            gs, xs = gs.flip(0), xs.flip(0)
        for k in range(K):
            j = K - 1 - k                                   # tap k of token u reads token u - j
            if n > j:
                gw[k] += (gs[j:] * xs[:n - j]).sum(0)
                n_terms[k] += n - j
        n_terms[K] += n
    gb = torch.zeros_like(g2[0]) if N == 0 else sum((g2[off:off + n].sum(0) for off, n in _pieces(lens)),
                                                    torch.zeros_like(g2[0]))
    hidden = tuple(x.shape[1:])
    return gw.reshape((K,) + hidden), gb.reshape(hidden), n_terms


def weight_grad_bounds(g, x, K: int, lens, reverse: bool, gw64, gb64, dtype):
    """(n_terms + K) u sum |g x| + r |result| for grad_weight and grad_bias."""
    aw, ab, n_terms = weight_grads64(g.double().abs(), x.double().abs(), K, lens, reverse)      # sum |g x|, sum |g|
    u = acc_u(dtype)
    terms = torch.tensor(n_terms[:K], dtype=F64).reshape((K,) + (1,) * (gw64.dim() - 1))
    return (terms + K) * u * aw + half_ulp(gw64, dtype), (n_terms[K] + K) * u * ab + half_ulp(gb64, dtype)


def ratio(got: torch.Tensor, want64: torch.Tensor, bound: torch.Tensor) -> float:
    """The worst error over its bound (0 for nothing to compare).  Where the bound is 0 the result must be exact."""
    if got.numel() == 0:
        return 0.0
    err = (got.detach().cpu().double().reshape(want64.shape) - want64).abs()
    if bool(((bound == 0) & (err > 0)).any()):
        return float('inf')
    return float((err / bound.clamp_min(1e-300)).max())
