"""ctypes binding of librua_hip.so (the C ABI declared in include/rua.h).

The product path has no CPU fallback: if the shared library is missing, or an op is handed a
tensor that does not live on a HIP device, we raise.  PyTorch is used only for device memory and
streams; every kernel is launched through the plain-pointer C ABI on torch's current stream.
"""
import ctypes
import os
import threading
from ctypes import POINTER, Structure, c_char_p, c_double, c_int, c_int32, c_int64, c_uint64, c_void_p

import torch  # noqa: F401  (must be imported first: maps the HIP runtime our library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('RUA_LIB_PATH') or os.path.join(_HERE, 'librua_hip.so')   # env: developer A/B of builds

ABI_VERSION = 6
# enum rua_kind
CAT, LEFT, PACK, RIGHT, LIST = 0, 1, 2, 3, 4
# enum rua_tmap
T_SHIFT, T_ROLL, T_REV_S, T_REV_D, T_ZERO = 0, 1, 2, 3, 4
TIES_FINAL = 2      # rua_segment_reduce_backward include_self: `ties` came complete from the forward
BWD_FILL_PADDING = 0x100   # ... OR-ed in: the call itself zeroes the padding rows of a padded layout
BWD_TIES_POSITIVE = 0x200  # ... OR-ed in (max/min): torch.segment_reduce's tie rule — ties share g only where g > 0
MOVE_SCATTER = 1
MOVE_NT_ON, MOVE_NT_OFF = 2, 4       # rua.h: force / forbid non-temporal payload accesses
MOVE_XCD_SPAN_ON, MOVE_XCD_SPAN_OFF = 256, 512      # rua.h: force / forbid one contiguous span of tiles per XCD
MOVE_NO_NARROW = 2048               # rua.h: developer A/B — rows of one vector through the generic kernel
OP_SCRATCH_CLEAN, OP_NO_EMPTY = 0x100, 0x200      # rua.h: bits OR-ed into `op` (persistent zeroed extreme scratch; no sequence is empty: proven)
EXTREME_WORDS = 1027                               # rua.h: RUA_EXTREME_WORDS
POOL_OUT_ACC = 0x100       # rua.h: RUA_POOL_OUT_ACC, OR-ed into the dtype of rua_segment_softmax_pool[_backward]
NORM_MEAN_ACC = 0x100      # rua.h: RUA_NORM_MEAN_ACC, OR-ed into the dtype of rua_segment_var_mean[_backward]
OP_SHORT_SEQS = 0x400      # rua.h: a CattedSequence of short sequences, none far above the average (a hint)
CONV_MAX_TAPS = 8          # rua.h: RUA_CONV_MAX_TAPS, the longest filter of rua_segment_causal_conv
JOIN_MAX_PARTS = 8         # rua.h: RUA_JOIN_MAX_PARTS, the most parts of one rua_segment_join
RUNS_BITS = 0x100          # rua.h: RUA_RUNS_BITS, the `eq` of rua_segment_runs_heads that compares bits
WINDOW_MAX_K = 64          # rua.h: RUA_WINDOW_MAX_K, the longest window of rua_segment_window_pool
CRF_MAX_TAGS = 64          # rua.h: RUA_CRF_MAX_TAGS, the most tags of the linear-chain CRF (a lane per tag)
CRF_LOG, CRF_MAX = 0, 1    # rua.h: RUA_CRF_LOG / RUA_CRF_MAX, the semiring of rua_segment_crf_forward
CTC_MAX_TARGET = 1023      # rua.h: RUA_CTC_MAX_TARGET, the longest target of the CTC operators (2 S + 1 <= 2 047 states)
EDIT_MAX_REF = 2048       # rua.h: RUA_EDIT_MAX_REF, the longest reference of the edit-distance operators (hyp is unbounded)
WINDOW_TAKE = 6            # rua.h: RUA_WINDOW_TAKE, the fourth mode of rua_segment_window_pool / _spread (next to SUM, MEAN, MAX)
# enum rua_dtype / rua_op
F32, BF16, F16, F64 = 0, 1, 2, 3
SUM, MEAN, MAX, MIN, PROD, LOGSUMEXP = 0, 1, 2, 3, 4, 5

I64, I32, I16, I8, U8 = 4, 5, 6, 7, 8

DTYPES = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.float64: F64}
# integer element types: rua_segment_reduce over a CAT layout only (scatter_* on integer tensors, reduce.py:6-23)
INT_DTYPES = {torch.int64: I64, torch.int32: I32, torch.int16: I16, torch.int8: I8, torch.uint8: U8}
# per-sequence cumsum (rua_segment_cumsum): the float types and int64
SCAN_DTYPES = {**DTYPES, torch.int64: I64}


class RuaLayout(Structure):
    """struct rua_layout (include/rua.h)."""
    _fields_ = [
        ('kind', c_int32), ('tile_t_log2', c_int32),
        ('n_rows', c_int64), ('B', c_int64), ('T_phys', c_int64), ('T_log', c_int64),
        ('lens', c_void_p), ('len_add', c_int64), ('off', c_void_p),
        ('boff', c_void_p), ('T', c_int64), ('sorted', c_void_p), ('unsorted', c_void_p),
        ('bptr', c_void_p), ('tptr', c_void_p),
        ('bsz', c_void_p), ('tile_start', c_void_p), ('n_tchunks', c_int64), ('n_tiles', c_int64),
    ]


class RuaError(RuntimeError):
    pass


# every symbol include/rua.h declares: name -> (restype, argtypes)
SYMBOLS = {
    'rua_scan_ws_elems': (c_int64, [c_int64]),
    'rua_exclusive_scan_i64': (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    'rua_pack_meta': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    'rua_pack_prepare': (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p]),
    'rua_lens_from_pack': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    'rua_enum_rows': (c_int, [POINTER(RuaLayout), c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_mask': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int32, c_uint64, c_uint64, c_void_p]),
    'rua_move_rows': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_int32, c_int64, c_void_p, c_void_p,
                              c_int64, c_void_p, c_int64, c_int32, c_void_p]),
    'rua_setitem_backward': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64,
                                     c_int32, c_void_p]),
    'rua_reduce_ws_bytes': (c_int64, [c_int64, c_int64, c_int32, c_int64]),
    'rua_reduce_team_waves': (c_int, [c_int64, c_int64, c_int64]),
    'rua_segment_reduce': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                   c_int32, c_uint64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    'rua_pack_reduce': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                c_int32, c_uint64, c_void_p, c_int64, c_void_p, c_void_p]),
    'rua_pack_sums': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                              c_int64, c_void_p, c_void_p]),
    'rua_pack_sums_backward': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64,
                                       c_int32, c_void_p]),
    'rua_sums_cast': (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p]),
    'rua_segment_reduce_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_int32, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    'rua_scatter_self_grad': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_int32, c_int32, c_void_p]),
    'rua_softmax_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_softmax': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                    c_void_p]),
    'rua_segment_softmax_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                             c_int32, c_void_p, c_void_p]),
    'rua_softmax_pool_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int64, c_int32]),
    'rua_segment_softmax_pool': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                         c_int32, c_void_p, c_void_p]),
    'rua_segment_softmax_pool_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    'rua_norm_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_var_mean': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64,
                                     c_void_p, c_void_p]),
    'rua_segment_var_mean_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_int64, c_int32, c_int64, c_void_p]),
    'rua_segment_standardize': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int64,
                                        c_double, c_void_p, c_void_p]),
    'rua_segment_standardize_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                                 c_int32, c_int64, c_void_p, c_void_p]),
    'rua_cumsum_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_cumsum': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    'rua_cumextreme_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_cumextreme': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32,
                                       c_int32, c_void_p, c_void_p]),
    'rua_segment_cumextreme_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                                c_int32, c_void_p, c_void_p]),
    'rua_logcumsumexp_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_logcumsumexp': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                         c_void_p]),
    'rua_segment_logcumsumexp_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                                  c_int32, c_int32, c_void_p, c_void_p]),
    'rua_crf_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int32, c_int32]),
    'rua_segment_crf_forward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    'rua_segment_crf_backtrace': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    'rua_segment_crf_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    'rua_segment_ctc_forward': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                        c_void_p]),
    'rua_segment_ctc_backtrace': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    'rua_segment_ctc_backward': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'rua_segment_edit_forward': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int32, c_void_p]),
    'rua_segment_edit_backtrace': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int32, c_void_p]),
    'rua_linear_scan_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_linear_scan': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_double, c_void_p, c_int64, c_int32,
                                        c_int32, c_void_p, c_void_p]),
    'rua_segment_linear_scan_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_double, c_void_p, c_void_p,
                                                 c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    'rua_causal_conv_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32, c_int32]),
    'rua_segment_causal_conv': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int32,
                                        c_int32, c_int32, c_void_p]),
    'rua_segment_causal_conv_backward': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                 c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    'rua_compress_ws_bytes': (c_int64, [POINTER(RuaLayout)]),
    'rua_segment_compress_plan': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_segment_compress_move': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64,
                                          c_int32, c_void_p]),
    'rua_segment_runs_heads': (c_int, [POINTER(RuaLayout), c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    'rua_segment_runs_inverse': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_segment_runs_counts': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_window_lens': (c_int, [POINTER(RuaLayout), c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    'rua_segment_window_pool': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64,
                                        c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'rua_segment_window_spread': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64,
                                          c_int32, c_int32, c_int32, c_int32, c_void_p]),
    'rua_segment_join_lens': (c_int, [POINTER(RuaLayout), c_int32, c_void_p, c_void_p, c_void_p]),
    'rua_segment_unjoin_lens': (c_int, [POINTER(RuaLayout), POINTER(c_void_p), POINTER(c_int64), c_int32, c_void_p,
                                        c_void_p, c_void_p]),
    'rua_segment_join': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_int32, c_void_p, POINTER(c_void_p), c_int64,
                                 c_int32, c_void_p]),
    'rua_repeat_ws_bytes': (c_int64, [POINTER(RuaLayout)]),
    'rua_segment_repeat_plan': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_segment_repeat_move': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_int64, c_void_p, c_void_p,
                                        c_int64, c_void_p]),
    'rua_segment_repeat_sum': (c_int, [POINTER(RuaLayout), POINTER(RuaLayout), c_void_p, c_void_p, c_int64, c_void_p,
                                       c_void_p, c_int64, c_int32, c_void_p]),
    'rua_sort_block_len': (c_int64, []),
    'rua_sort_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_sort': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                 c_void_p]),
    'rua_segment_reorder': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int32,
                                    c_void_p]),
    'rua_argreduce_ws_bytes': (c_int64, [POINTER(RuaLayout), c_int64, c_int32]),
    'rua_segment_argreduce': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p,
                                      c_void_p]),
    'rua_segment_take': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    'rua_segment_put': (c_int, [POINTER(RuaLayout), c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    'rua_fill_empty': (c_int, [POINTER(RuaLayout), c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    'rua_bucket_ws_elems': (c_int64, [c_int64, c_int64]),
    'rua_index_buckets': (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'rua_host_sort_desc': (c_int, [c_void_p, c_int64, c_void_p, c_int32]),
    'rua_host_sort_desc_begin': (c_int, [c_void_p, c_int64, c_void_p, c_int32]),
    'rua_host_sort_desc_end': (c_int, []),
    'rua_host_sort_heap_segments': (c_int64, []),
    'rua_host_batch_sizes': (c_int, [c_void_p, c_int64, c_int64, c_void_p]),
    'rua_host_pack_scans': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    'rua_debug_trace': (c_int, [c_int32]),
    'rua_debug_trace_take': (c_int64, [c_char_p, c_int64]),
    'rua_debug_reduce_plan': (c_int64, [c_int32, POINTER(RuaLayout), POINTER(RuaLayout), c_int64, c_int32, c_int32, c_int32,
                                        c_int64, c_int32, c_int32, c_char_p, c_int64]),
    'rua_debug_move_plan': (c_int64, [POINTER(RuaLayout), POINTER(RuaLayout), c_int32, c_int64, c_uint64, c_uint64, c_int64,
                                      c_int64, c_int32, c_char_p, c_int64]),
    'rua_abi_version': (c_int, []),
    'rua_build_target': (c_char_p, []),
}

_lib = None


def load():
    """Load librua_hip.so (once).  Raises RuaError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuaError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C torchrua_amd/csrc`. torchrua_amd has no CPU/eager fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table disagree
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.rua_abi_version() != ABI_VERSION:
        raise RuaError(f'ABI mismatch: library reports {lib.rua_abi_version()}, binding expects {ABI_VERSION}')
    _lib = lib
    return lib


_tls = threading.local()       # .prev: the device stream_ptr() switched away from for the launch in flight


def check(code: int, what: str) -> None:
    prev = getattr(_tls, 'prev', None)
    if prev is not None:           # stream_ptr() made another device current for this one launch: hand it back
        _tls.prev = None
        torch.cuda.set_device(prev)
    if code == 0:
        return
    if code < 0:
        names = {-1: 'RUA_EINVAL', -2: 'RUA_EALIGN', -3: 'RUA_ERANGE'}
        raise RuaError(f'{what}: rejected argument ({names.get(code, code)})')
    raise RuaError(f'{what}: HIP error {code}')


def stream_ptr(device) -> int:
    """torch's current stream on `device` — the device the TENSORS live on, whatever the thread's current device is,
    as with any torch op (and therefore with the reference: core/get.py:25-29 indexes on `self.data.device`).  A HIP
    launch goes to the calling thread's current device, so when that is another one it is switched for this ONE launch:
    every call site is `check(lib.rua_xxx(..., stream_ptr(dev)), name)`, the stream argument is evaluated last before
    the call and check() runs right after it and switches back.  (One process per GPU never takes this branch.)"""
    cur = torch.cuda.current_device()
    idx = cur if device.index is None else device.index
    if idx != cur:
        if getattr(_tls, 'prev', None) is None:
            _tls.prev = cur
        torch.cuda.set_device(idx)
    # the raw hipStream_t of torch's current stream; torch.cuda.current_stream() builds a Stream object (~6 us a call)
    return torch._C._cuda_getCurrentRawStream(idx)


def require_device(*tensors) -> torch.device:
    """All tensors must sit on one HIP device; there is no host path."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuaError(
                'torchrua_amd runs on MI355X only: got a tensor on '
                f'{t.device}; move it to a HIP device (there is no CPU fallback by design)')
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuaError(f'tensors on different devices: {dev} vs {t.device}')
    return dev


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()
