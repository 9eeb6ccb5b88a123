"""markov-huffman-coding_amd — MI355X-native Markov-Huffman codec (ctypes face of libmhc.so).

The product is the C-ABI library (include/mh.h) built from csrc/ — hand-written HIP kernels for
gfx950 plus the C++ host model.  This module only binds it for tests and bench.py; it contains no
codec logic and never falls back to a CPU implementation: if libmhc.so is missing it raises, and
every compute call needs a GPU (MH_ERR_NO_DEVICE otherwise).

The directory name carries a hyphen, so import it through `__graft_entry__.load_package()`
(which registers it as module `mhc_amd`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MH_LIB: an experimental build of the same library (csrc/Makefile `make exp TAG=x EXPFLAGS=-D...`), for A/B runs
LIB_PATH = os.environ.get("MH_LIB") or os.path.join(_HERE, "libmhc.so")

MH_OK = 0
MH_ERR_ARG, MH_ERR_NO_DEVICE, MH_ERR_HIP, MH_ERR_CORRUPT, MH_ERR_TYPE = -1, -2, -3, -4, -5
MH_ERR_BADTABLE, MH_ERR_CODE_TOO_LONG, MH_ERR_CAPACITY, MH_ERR_TIMEOUT, MH_ERR_NOMEM = -6, -7, -8, -9, -10
PREV0 = 0x20
CHUNK_DEFAULT = 1024
INDEX_BIT_MASK = 0x00FFFFFFFFFFFFFF
INDEX2_BIT_MASK = 0x0000FFFFFFFFFFFF      # order-2 models: two context bytes in bits 48..63

# every symbol include/mh.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "mh_strerror", "mh_last_hip_error", "mh_last_index_path", "mh_last_encode_retries", "mh_total_encode_retries", "mh_device_count", "mh_set_device",
    "mh_dev_malloc", "mh_dev_free", "mh_dev_upload", "mh_dev_download",
    "mh_model_from_counts", "mh_dev_model_from_counts", "mh_dev_model_workspace", "mh_dev_model_from_counts_ws",
    "mh_model_from_counts_limited", "mh_dev_model_from_counts_limited", "mh_dev_model_from_counts_limited_ws",
    "mh_model_from_table_bits", "mh_model_write_table",
    "mh_model_type", "mh_model_max_code_len", "mh_model_min_code_len", "mh_model_get_code", "mh_model_get_lut", "mh_model_decode_layout", "mh_model_tile_layout",
    "mh_model_image", "mh_model_free",
    "mh_set_input_residency", "mh_histogram_o1", "mh_histogram_o0", "mh_histogram_o2", "mh_dev_histogram_o2", "mh_dev_histogram_o2_ws", "mh_dev_histogram_o2_workspace", "mh_encode", "mh_encode_bound", "mh_stream_header",
    "mh_stream_parse_header", "mh_decode",
    "mh_dev_histogram_workspace", "mh_dev_histogram_o1", "mh_dev_histogram_o0",
    "mh_decode_to", "mh_model_payload_bits", "mh_dev_encode_workspace", "mh_dev_encode", "mh_dev_payload_bits", "mh_dev_encode_at", "mh_dev_encode_ctx", "mh_dev_encode_hist", "mh_dev_decode_workspace", "mh_dev_decode", "mh_dev_decode_dn",
    "mh_dev_build_index_workspace", "mh_dev_build_index", "mh_dev_status",
    "mh_dev_model2_workspace", "mh_dev_model2_array", "mh_dev_model2_build_slice", "mh_dev_model2_finish",
    "mh_dev_encode_fine", "mh_dev_encode_ctx_fine", "mh_dev_decode_fine", "mh_dev_build_index_fine", "mh_dev_decode_stream_states", "mh_dev_decode_stream_emit", "mh_dev_index_path", "mh_dev_encode_path", "mh_dev_decode_path", "mh_dev_decode_variant",
    "mh_batch_index_base", "mh_batch_index_capacity", "mh_dev_histogram_batch_workspace", "mh_dev_histogram_o1_batch", "mh_dev_histogram_o0_batch",
    "mh_encode_batch_bound", "mh_dev_encode_batch_workspace", "mh_dev_encode_batch", "mh_dev_decode_batch_workspace", "mh_dev_decode_batch",
    "mh_encode_batch", "mh_decode_batch",
    "mh_dev_model_set_train_workspace", "mh_dev_model_set_train", "mh_model_set_from_models", "mh_model_set_from_tables", "mh_model_set_free",
    "mh_model_set_size", "mh_model_set_slots", "mh_model_set_stream_info", "mh_model_set_code_lens", "mh_model_set_tables_bound",
    "mh_dev_model_set_tables_workspace", "mh_dev_model_set_tables", "mh_encode_each_bound", "mh_dev_encode_each_workspace", "mh_dev_encode_each",
    "mh_dev_decode_each_workspace", "mh_dev_decode_each", "mh_compress_each_bounds", "mh_compress_each", "mh_decompress_each",
    "mh_dev_decode_ranges_workspace", "mh_dev_decode_ranges", "mh_decode_ranges", "mh_last_range_upload_bytes",
    "mh_dev_decode_batch_ranges_workspace", "mh_dev_decode_batch_ranges", "mh_dev_decode_each_ranges", "mh_decode_batch_ranges",
    "mh_decompress_each_ranges", "mh_last_batch_range_upload_bytes",
    "mh_dev_bank_select_workspace", "mh_dev_bank_select", "mh_dev_model_set_pick", "mh_dev_bank_train_workspace", "mh_dev_bank_train",
    "mh_bank_train", "mh_encode_bank_bound", "mh_encode_bank", "mh_decode_bank",
    "mh_dev_batch_states_workspace", "mh_dev_batch_states", "mh_dev_each_states", "mh_dev_batch_index", "mh_dev_each_index",
    "mh_dev_batch_emit", "mh_dev_each_emit", "mh_index_batch", "mh_index_each",
    "mh_dev_histogram_o2_batch_workspace", "mh_dev_histogram_o2_batch", "mh_dev_encode_batch_o2_workspace", "mh_dev_encode_batch_o2",
    "mh_dev_decode_batch_o2_workspace", "mh_dev_decode_batch_o2", "mh_encode_batch_o2", "mh_decode_batch_o2",
    "mh_dev_decode_ranges_o2_workspace", "mh_dev_decode_ranges_o2", "mh_decode_ranges_o2",
    "mh_dev_decode_batch_o2_ranges_workspace", "mh_dev_decode_batch_o2_ranges", "mh_decode_batch_o2_ranges",
    "mh_pattern_set_create", "mh_pattern_set_size", "mh_pattern_set_max_len", "mh_pattern_set_free",
    "mh_dev_find_batch_workspace", "mh_dev_find_batch", "mh_dev_find_each", "mh_find_batch",
    "mh_dev_histogram_coded_workspace", "mh_dev_histogram_coded_batch", "mh_dev_histogram_coded_each",
    "mh_dev_recode_batch_workspace", "mh_dev_recode_batch", "mh_dev_recode_each", "mh_recode_batch",
    "mh_dev_find_batch_o2_workspace", "mh_dev_find_batch_o2", "mh_find_batch_o2", "mh_dev_histogram_coded_batch_o2_workspace",
    "mh_dev_histogram_coded_batch_o2", "mh_dev_recode_batch_o2_workspace", "mh_dev_recode_batch_o2", "mh_recode_batch_o2",
    "mh_dev_batch_states_o2_workspace", "mh_dev_batch_states_o2", "mh_dev_batch_index_o2", "mh_dev_batch_emit_o2", "mh_index_batch_o2",
    "mh_dev_batch_states_stats",
    "mh_dev_crc_batch_workspace", "mh_dev_crc_batch", "mh_dev_crc_each", "mh_dev_crc_batch_o2", "mh_crc_batch", "mh_crc_batch_o2",
    "mh_dev_crc_raw_batch_workspace", "mh_dev_crc_raw_batch", "mh_crc32_combine",
    "mh_dict_create", "mh_dict_free", "mh_dict_size", "mh_dict_max_len", "mh_dict_states", "mh_dict_classes", "mh_dict_device_bytes",
    "mh_dict_find_bytes", "mh_dev_find_dict_workspace", "mh_dev_find_dict_batch", "mh_dev_find_dict_each", "mh_dev_find_dict_batch_o2",
    "mh_find_dict_batch", "mh_find_dict_batch_o2",
    "mh_spans_from_hits", "mh_dev_spans_from_hits_workspace", "mh_dev_spans_from_hits", "mh_dev_recode_edit_workspace",
    "mh_dev_recode_edit_batch", "mh_dev_recode_edit_each", "mh_recode_edit_batch",
    "mh_dev_recode_splice_workspace", "mh_dev_recode_splice_batch", "mh_dev_recode_splice_each", "mh_recode_splice_batch",
    "mh_spans_from_hits_tagged", "mh_dev_spans_from_hits_tagged_workspace", "mh_dev_spans_from_hits_tagged",
    "mh_dev_recode_splice_table_workspace", "mh_dev_recode_splice_table_batch", "mh_dev_recode_splice_table_each",
    "mh_recode_splice_table_batch",
    "mh_dev_recode_edit_batch_o2_workspace", "mh_dev_recode_splice_table_batch_o2_workspace", "mh_dev_recode_edit_batch_o2",
    "mh_dev_recode_splice_table_batch_o2", "mh_recode_edit_batch_o2", "mh_recode_splice_table_batch_o2",
    "mh_dev_select_batch_workspace", "mh_dev_select_batch", "mh_dev_picks_from_hits_workspace", "mh_dev_picks_from_hits",
    "mh_select_batch", "mh_picks_from_hits",
    "mh_span_token_digest", "mh_dev_span_tokens_workspace", "mh_dev_span_tokens_batch", "mh_span_tokens_batch",
]
FIND_MAX_POSITIONS = 64                    # include/mh.h MH_FIND_MAX_POSITIONS
FIND_FOLD_ASCII = 1                        # include/mh.h MH_FIND_FOLD_ASCII
DICT_MAX_LEN = 255                         # include/mh.h MH_DICT_MAX_LEN
DICT_MAX_STATES = 32768                    # include/mh.h MH_DICT_MAX_STATES
DICT_MAX_PATTERNS = 65536                  # include/mh.h MH_DICT_MAX_PATTERNS
DICT_MAX_OUTPUTS = 1 << 20                 # include/mh.h MH_DICT_MAX_OUTPUTS
BANK_MAX = 64                              # include/mh.h MH_BANK_MAX
BANK_NONE = 0xFFFFFFFF                     # include/mh.h MH_BANK_NONE
BATCH_WALK_MAX_BITS = 1 << 23              # include/mh.h MH_BATCH_WALK_MAX_BITS
SELECT_MAX_SOURCES = 8                     # include/mh.h MH_SELECT_MAX_SOURCES
SELECT_NONE = 0xFFFFFFFFFFFFFFFF           # include/mh.h MH_SELECT_NONE
PICKS_WITHOUT_HITS = 1                     # include/mh.h MH_PICKS_WITHOUT_HITS
TOKEN_FOLD = 1                             # include/mh.h MH_TOKEN_FOLD
SPLICE_MAX_REP = 255                       # include/mh.h MH_SPLICE_MAX_REP


class MhError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().mh_strerror(status).decode() if _lib is not None else str(status)
        super().__init__("%s: %s (%d)" % (what, msg, status))


class CodedBatchArgs(C.Structure):
    """include/mh.h mh_coded_batch_args: the batch description inside the argument blocks below."""
    _fields_ = [("d_payload", C.c_void_p), ("d_pay_off", C.c_void_p), ("d_nbits", C.c_void_p), ("n_streams", C.c_size_t),
                ("pay_total", C.c_uint64), ("prev0", C.c_uint8), ("d_sym_off", C.c_void_p), ("sym_total", C.c_uint64),
                ("d_index", C.c_void_p), ("chunk_symbols", C.c_uint32)]


class RecodeEditO2Args(C.Structure):
    """include/mh.h mh_recode_edit_o2_args: the parameters of mh_dev_recode_edit_batch under the same names, in the same order."""
    _fields_ = [("struct_size", C.c_uint32), ("src", C.c_void_p), ("dst", C.c_void_p), ("batch", CodedBatchArgs),
                ("d_span_off", C.c_void_p), ("d_spans", C.c_void_p), ("d_map", C.c_void_p), ("d_out_payload", C.c_void_p),
                ("cap", C.c_size_t), ("d_out_off", C.c_void_p), ("d_out_nbits", C.c_void_p), ("d_out_index", C.c_void_p),
                ("d_dropped", C.c_void_p), ("d_stream_status", C.c_void_p), ("d_ws", C.c_void_p), ("ws_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class RecodeSpliceO2Args(C.Structure):
    """include/mh.h mh_recode_splice_o2_args: the parameters of mh_dev_recode_splice_table_batch, same names, same order."""
    _fields_ = [("struct_size", C.c_uint32), ("src", C.c_void_p), ("dst", C.c_void_p), ("batch", CodedBatchArgs),
                ("d_span_off", C.c_void_p), ("d_spans", C.c_void_p), ("d_span_tag", C.c_void_p), ("d_rep_off", C.c_void_p),
                ("d_rep_bytes", C.c_void_p), ("n_reps", C.c_size_t), ("d_out_payload", C.c_void_p), ("cap", C.c_size_t),
                ("d_out_off", C.c_void_p), ("d_out_nbits", C.c_void_p), ("d_out_sym_off", C.c_void_p), ("d_out_index", C.c_void_p),
                ("index_cap", C.c_uint64), ("d_dropped", C.c_void_p), ("d_stream_status", C.c_void_p), ("d_ws", C.c_void_p),
                ("ws_bytes", C.c_size_t), ("stream", C.c_void_p)]


class Launch(C.Structure):
    """include/mh.h mh_launch: the workspace and the stream of a call that takes a block."""
    _fields_ = [("d_ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("stream", C.c_void_p)]


class SelectArgs(C.Structure):
    """include/mh.h mh_select_args."""
    _fields_ = [("struct_size", C.c_uint32), ("sources", C.POINTER(CodedBatchArgs)), ("n_sources", C.c_uint32), ("d_picks", C.c_void_p),
                ("n_picks", C.c_size_t), ("d_out_payload", C.c_void_p), ("cap", C.c_size_t), ("d_out_off", C.c_void_p),
                ("d_out_nbits", C.c_void_p), ("d_out_sym_off", C.c_void_p), ("d_out_index", C.c_void_p), ("index_cap", C.c_uint64),
                ("chunk_symbols", C.c_uint32), ("d_pick_status", C.c_void_p), ("launch", Launch)]


class PicksArgs(C.Structure):
    """include/mh.h mh_picks_args."""
    _fields_ = [("struct_size", C.c_uint32), ("d_hit_off", C.c_void_p), ("d_stream_status", C.c_void_p), ("n_streams", C.c_size_t),
                ("source", C.c_uint32), ("flags", C.c_uint32), ("d_picks", C.c_void_p), ("d_n_kept", C.c_void_p), ("launch", Launch)]


class SpanTokensArgs(C.Structure):
    """include/mh.h mh_span_tokens_args."""
    _fields_ = [("struct_size", C.c_uint32), ("src", C.c_void_p), ("src_set", C.c_void_p), ("batch", CodedBatchArgs),
                ("d_span_off", C.c_void_p), ("d_spans", C.c_void_p), ("d_span_tag", C.c_void_p), ("key", C.c_uint8 * 16),
                ("flags", C.c_uint32), ("d_fmt_off", C.c_void_p), ("d_fmt_bytes", C.c_void_p), ("d_hex_digits", C.c_void_p),
                ("n_formats", C.c_size_t), ("n_reps", C.c_size_t), ("d_rep_off", C.c_void_p), ("d_rep_bytes", C.c_void_p),
                ("rep_cap", C.c_size_t), ("d_rep_tag", C.c_void_p), ("d_stream_status", C.c_void_p)]


def _addr(v):
    return v.value if isinstance(v, C.c_void_p) else v


def coded_batches(sources):
    """A ctypes array of mh_coded_batch_args from (payload, pay_off, nbits, n_streams, pay_total, sym_off, sym_total, index,
    chunk_symbols) tuples of addresses and numbers."""
    arr = (CodedBatchArgs * max(len(sources), 1))()
    for b, (payload, pay_off, nbits, n, pay_total, sym_off, sym_total, index, chunk) in zip(arr, sources):
        b.d_payload, b.d_pay_off, b.d_nbits, b.n_streams, b.pay_total = _addr(payload), _addr(pay_off), _addr(nbits), n, pay_total
        b.d_sym_off, b.sym_total, b.d_index, b.chunk_symbols = _addr(sym_off), sym_total, _addr(index), chunk
    return arr


def select_args(sources, n_sources, picks, n_picks, out_payload, cap, out_off, out_nbits, out_sym_off, out_index, index_cap, chunk_symbols,
                pick_status, ws, ws_bytes, stream):
    """An mh_select_args block (sources: a coded_batches array, which the block keeps alive)."""
    blk = SelectArgs(C.sizeof(SelectArgs), sources, n_sources, _addr(picks), n_picks, _addr(out_payload), cap, _addr(out_off), _addr(out_nbits),
                     _addr(out_sym_off), _addr(out_index), index_cap, chunk_symbols, _addr(pick_status), Launch(_addr(ws), ws_bytes, _addr(stream)))
    blk.keep = sources
    return blk


def picks_args(hit_off, stream_status, n_streams, source, flags, picks, n_kept, ws, ws_bytes, stream):
    """An mh_picks_args block."""
    return PicksArgs(C.sizeof(PicksArgs), _addr(hit_off), _addr(stream_status), n_streams, source, flags, _addr(picks), _addr(n_kept),
                     Launch(_addr(ws), ws_bytes, _addr(stream)))


def span_tokens_args(src, src_set, batch, span_off, spans, span_tag, key, flags, fmt_off, fmt_bytes, hex_digits, n_formats, n_reps,
                     rep_off, rep_bytes, rep_cap, rep_tag, stream_status):
    """An mh_span_tokens_args block.  batch: one coded_batches tuple (with prev0 appended: ten values); key: 16 bytes."""
    payload, pay_off, nbits, n, pay_total, sym_off, sym_total, index, chunk, prev0 = batch
    blk = SpanTokensArgs()
    blk.struct_size = C.sizeof(SpanTokensArgs)
    blk.src, blk.src_set = _addr(src), _addr(src_set)
    b = blk.batch
    b.d_payload, b.d_pay_off, b.d_nbits, b.n_streams, b.pay_total, b.prev0 = _addr(payload), _addr(pay_off), _addr(nbits), n, pay_total, prev0
    b.d_sym_off, b.sym_total, b.d_index, b.chunk_symbols = _addr(sym_off), sym_total, _addr(index), chunk
    blk.d_span_off, blk.d_spans, blk.d_span_tag = _addr(span_off), _addr(spans), _addr(span_tag)
    key = bytes(key)
    if len(key) != 16:
        raise ValueError("a token key has 16 bytes")
    blk.key = (C.c_uint8 * 16)(*key)
    blk.flags = flags
    blk.d_fmt_off, blk.d_fmt_bytes, blk.d_hex_digits, blk.n_formats = _addr(fmt_off), _addr(fmt_bytes), _addr(hex_digits), n_formats
    blk.n_reps, blk.d_rep_off, blk.d_rep_bytes, blk.rep_cap = n_reps, _addr(rep_off), _addr(rep_bytes), rep_cap
    blk.d_rep_tag, blk.d_stream_status = _addr(rep_tag), _addr(stream_status)
    return blk


def launch_args(ws, ws_bytes, stream):
    """An mh_launch: where a call that takes one runs."""
    return Launch(_addr(ws), ws_bytes, _addr(stream))


def args_block(cls, *a):
    """An argument block of class `cls` from the positional parameters of the order-0/1 twin call: struct_size set, the members
    filled in order, the batch's ten into the nested block."""
    want = sum(len(CodedBatchArgs._fields_) if typ is CodedBatchArgs else 1 for _, typ in cls._fields_[1:])
    if len(a) != want:
        raise TypeError("%s takes %d members behind struct_size, %d given" % (cls.__name__, want, len(a)))
    blk = cls()
    blk.struct_size = C.sizeof(cls)
    it = iter(a)
    for name, typ in cls._fields_[1:]:
        into, names = (blk.batch, [f[0] for f in CodedBatchArgs._fields_]) if typ is CodedBatchArgs else (blk, [name])
        for k in names:
            v = next(it)
            setattr(into, k, v.value if isinstance(v, C.c_void_p) else v)
    return blk


_lib = None


def lib():
    """Loads libmhc.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libmhc.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C markov-huffman-coding_amd/csrc`")
        l = C.CDLL(LIB_PATH)
        vp, sz, u8, u32, u64, i32 = C.c_void_p, C.c_size_t, C.c_uint8, C.c_uint32, C.c_uint64, C.c_int
        pi, pu64, psz = C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        l.mh_strerror.restype = C.c_char_p
        l.mh_strerror.argtypes = [i32]
        l.mh_total_encode_retries.restype = u64
        l.mh_dev_malloc.argtypes = [C.POINTER(vp), sz]
        l.mh_dev_free.argtypes = [vp]
        l.mh_dev_upload.argtypes = [vp, vp, sz]
        l.mh_dev_download.argtypes = [vp, vp, sz]
        l.mh_model_from_counts.argtypes = [vp, i32, C.POINTER(vp)]
        l.mh_dev_model_from_counts.argtypes = [vp, i32, vp, C.POINTER(vp)]
        l.mh_dev_model_workspace.argtypes = [i32]
        l.mh_dev_model_workspace.restype = sz
        l.mh_dev_model_from_counts_ws.argtypes = [vp, i32, vp, sz, vp, C.POINTER(vp)]
        l.mh_model_from_counts_limited.argtypes = [vp, i32, i32, C.POINTER(vp)]
        l.mh_dev_model_from_counts_limited.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
        l.mh_dev_model_from_counts_limited_ws.argtypes = [vp, i32, i32, vp, sz, vp, C.POINTER(vp)]
        l.mh_model_from_table_bits.argtypes = [vp, sz, C.POINTER(vp)]
        l.mh_model_write_table.argtypes = [vp, vp, sz, psz]
        l.mh_model_type.argtypes = [vp]
        l.mh_model_max_code_len.argtypes = [vp]
        l.mh_model_min_code_len.argtypes = [vp]
        l.mh_model_get_code.argtypes = [vp, i32, i32, pi, pu64]
        l.mh_model_get_lut.argtypes = [vp, i32, i32, pi, pi, pi, pi]
        l.mh_model_decode_layout.argtypes = [vp, pi, pi, pi]
        l.mh_model_tile_layout.argtypes = [vp, pi, pi, pi]
        l.mh_model_image.argtypes = [vp, i32, vp, sz, psz]
        l.mh_model_free.argtypes = [vp]
        l.mh_model_free.restype = None
        l.mh_histogram_o1.argtypes = [vp, sz, u8, vp]
        l.mh_histogram_o0.argtypes = [vp, sz, vp]
        l.mh_histogram_o2.argtypes = [vp, sz, vp]
        l.mh_dev_histogram_o2.argtypes = [vp, sz, C.c_uint16, vp, vp]
        l.mh_dev_histogram_o2_ws.argtypes = [vp, sz, C.c_uint16, vp, vp, sz, vp]
        l.mh_dev_histogram_o2_workspace.argtypes = [sz]
        l.mh_dev_histogram_o2_workspace.restype = sz
        l.mh_encode.argtypes = [vp, vp, sz, u8, vp, sz, pu64, vp, u32]
        l.mh_encode_bound.argtypes = [vp, sz]
        l.mh_encode_bound.restype = sz
        l.mh_stream_header.argtypes = [vp, u64]
        l.mh_stream_header.restype = u8
        l.mh_stream_parse_header.argtypes = [vp, u8, u64, pu64]
        l.mh_decode.argtypes = [vp, vp, u64, u8, vp, sz, psz, vp, u32, u64]
        l.mh_dev_histogram_workspace.argtypes = [sz]
        l.mh_dev_histogram_workspace.restype = sz
        l.mh_dev_histogram_o1.argtypes = [vp, sz, u8, vp, vp, sz, vp]
        l.mh_dev_histogram_o0.argtypes = [vp, sz, vp, vp, sz, vp]
        l.mh_dev_encode_workspace.argtypes = [sz]
        l.mh_dev_encode_workspace.restype = sz
        l.mh_dev_encode.argtypes = [vp, vp, sz, u8, vp, sz, vp, vp, u32, vp, sz, vp]
        l.mh_dev_payload_bits.argtypes = [vp, vp, vp, vp]
        l.mh_model_payload_bits.argtypes = [vp, vp, pu64]
        l.mh_dev_encode_at.argtypes = [vp, vp, sz, u8, vp, vp, sz, vp, vp, u32, vp, sz, vp]
        l.mh_dev_encode_ctx.argtypes = [vp, vp, sz, u32, vp, vp, sz, vp, vp, u32, vp, sz, vp]
        l.mh_dev_encode_hist.argtypes = [vp, vp, sz, u8, vp, vp, sz, vp, vp, u32, vp, sz, vp, sz, vp]
        l.mh_dev_decode_workspace.argtypes = [u64, u64, u32]
        l.mh_dev_decode_workspace.restype = sz
        l.mh_dev_decode.argtypes = [vp, vp, u64, vp, u64, vp, u32, vp, sz, vp]
        l.mh_dev_decode_dn.argtypes = [vp, vp, vp, u64, vp, u64, vp, u32, vp, sz, vp]
        l.mh_dev_build_index_workspace.argtypes = [u64]
        l.mh_dev_build_index_workspace.restype = sz
        l.mh_dev_build_index.argtypes = [vp, vp, u64, u8, vp, u64, u32, vp, vp, sz, vp]
        l.mh_dev_status.argtypes = [vp, vp]
        l.mh_dev_encode_fine.argtypes = [vp, vp, sz, u8, vp, vp, sz, vp, vp, u32, vp, vp, sz, vp, sz, vp]
        l.mh_dev_model2_workspace.argtypes = []
        l.mh_dev_model2_workspace.restype = sz
        l.mh_dev_model2_array.argtypes = [i32, psz, psz]
        l.mh_dev_model2_build_slice.argtypes = [vp, u32, u32, vp, sz, vp]
        l.mh_dev_model2_finish.argtypes = [vp, sz, vp, C.POINTER(vp)]
        l.mh_dev_encode_ctx_fine.argtypes = [vp, vp, sz, u32, vp, vp, sz, vp, vp, u32, vp, vp, sz, vp]
        l.mh_dev_decode_fine.argtypes = [vp, vp, u64, vp, vp, u64, vp, u32, vp, vp, sz, vp]
        l.mh_dev_build_index_fine.argtypes = [vp, vp, u64, u8, vp, u64, u32, vp, u64, vp, vp, sz, vp]
        l.mh_dev_decode_stream_states.argtypes = [vp, vp, u64, u8, vp, vp, sz, vp]
        l.mh_dev_decode_stream_emit.argtypes = [vp, vp, u64, u8, vp, u64, vp, sz, vp]
        l.mh_dev_index_path.argtypes = [vp, vp]
        l.mh_dev_decode_variant.argtypes = [vp, vp]
        l.mh_dev_encode_path.argtypes = [vp, vp]
        l.mh_dev_decode_path.argtypes = [vp, vp]
        l.mh_batch_index_base.argtypes = [u64, u64, u32]
        l.mh_batch_index_base.restype = u64
        l.mh_batch_index_capacity.argtypes = [u64, u64, u32]
        l.mh_batch_index_capacity.restype = u64
        l.mh_dev_histogram_batch_workspace.argtypes = [sz]
        l.mh_dev_histogram_batch_workspace.restype = sz
        l.mh_dev_histogram_o1_batch.argtypes = [vp, vp, sz, sz, u8, vp, vp, sz, vp]
        l.mh_dev_histogram_o0_batch.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp]
        l.mh_encode_batch_bound.argtypes = [vp, sz, sz]
        l.mh_encode_batch_bound.restype = sz
        l.mh_dev_encode_batch_workspace.argtypes = [sz, sz]
        l.mh_dev_encode_batch_workspace.restype = sz
        l.mh_dev_encode_batch.argtypes = [vp, vp, vp, sz, sz, u8, vp, sz, vp, vp, vp, u32, vp, sz, vp]
        l.mh_dev_decode_batch_workspace.argtypes = [sz]
        l.mh_dev_decode_batch_workspace.restype = sz
        l.mh_dev_decode_batch.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, u64, vp, u32, vp, vp, sz, vp]
        l.mh_encode_batch.argtypes = [vp, vp, vp, sz, u8, vp, sz, vp, vp, vp, u32]
        l.mh_decode_batch.argtypes = [vp, vp, vp, vp, sz, u8, vp, sz, vp, vp, u32, vp]
        l.mh_dev_histogram_o2_batch_workspace.argtypes = [sz]
        l.mh_dev_histogram_o2_batch_workspace.restype = sz
        l.mh_dev_histogram_o2_batch.argtypes = [vp, vp, sz, sz, u8, vp, vp, sz, vp]
        l.mh_dev_encode_batch_o2_workspace.argtypes = [sz, sz]
        l.mh_dev_encode_batch_o2_workspace.restype = sz
        l.mh_dev_encode_batch_o2.argtypes = l.mh_dev_encode_batch.argtypes
        l.mh_dev_decode_batch_o2_workspace.argtypes = [sz]
        l.mh_dev_decode_batch_o2_workspace.restype = sz
        l.mh_dev_decode_batch_o2.argtypes = l.mh_dev_decode_batch.argtypes
        l.mh_encode_batch_o2.argtypes = l.mh_encode_batch.argtypes
        l.mh_decode_batch_o2.argtypes = l.mh_decode_batch.argtypes
        l.mh_dev_model_set_train_workspace.argtypes = [sz]
        l.mh_dev_model_set_train_workspace.restype = sz
        l.mh_dev_model_set_train.argtypes = [vp, vp, sz, sz, i32, u8, vp, sz, vp, C.POINTER(vp)]
        l.mh_model_set_from_models.argtypes = [C.POINTER(vp), sz, C.POINTER(vp)]
        l.mh_model_set_from_tables.argtypes = [vp, vp, sz, C.POINTER(vp)]
        l.mh_model_set_free.argtypes = [vp]
        l.mh_model_set_free.restype = None
        l.mh_model_set_size.argtypes = [vp]
        l.mh_model_set_size.restype = sz
        l.mh_model_set_slots.argtypes = [vp]
        l.mh_model_set_slots.restype = sz
        l.mh_model_set_stream_info.argtypes = [vp, sz, pi, pi]
        l.mh_model_set_code_lens.argtypes = [vp, pi, pi]
        l.mh_model_set_tables_bound.argtypes = [vp]
        l.mh_model_set_tables_bound.restype = sz
        l.mh_dev_model_set_tables_workspace.argtypes = [vp]
        l.mh_dev_model_set_tables_workspace.restype = sz
        l.mh_dev_model_set_tables.argtypes = [vp, vp, sz, vp, vp, sz, vp]
        l.mh_encode_each_bound.argtypes = [vp, sz, sz]
        l.mh_encode_each_bound.restype = sz
        l.mh_dev_encode_each_workspace.argtypes = [sz, sz]
        l.mh_dev_encode_each_workspace.restype = sz
        l.mh_dev_encode_each.argtypes = [vp, vp, vp, sz, sz, u8, vp, sz, vp, vp, vp, u32, vp, sz, vp]
        l.mh_dev_decode_each_workspace.argtypes = [sz]
        l.mh_dev_decode_each_workspace.restype = sz
        l.mh_dev_decode_each.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, u64, vp, u32, vp, vp, sz, vp]
        l.mh_compress_each_bounds.argtypes = [vp, sz, psz, psz]
        l.mh_compress_each.argtypes = [vp, vp, sz, i32, u8, vp, sz, vp, vp, sz, vp, vp, vp, u32]
        l.mh_decompress_each.argtypes = [vp, vp, vp, vp, vp, sz, u8, vp, sz, vp, vp, u32, vp]
        l.mh_dev_decode_ranges_workspace.argtypes = [sz]
        l.mh_dev_decode_ranges_workspace.restype = sz
        l.mh_dev_decode_ranges.argtypes = [vp, vp, u64, u64, u64, vp, u32, u64, vp, vp, sz, vp, vp, u64, vp, vp, sz, vp]
        l.mh_decode_ranges.argtypes = [vp, vp, u64, vp, u32, u64, vp, sz, vp, sz, vp, vp]
        l.mh_last_range_upload_bytes.argtypes = []
        l.mh_last_range_upload_bytes.restype = u64
        l.mh_dev_decode_batch_ranges_workspace.argtypes = [sz]
        l.mh_dev_decode_batch_ranges_workspace.restype = sz
        l.mh_dev_decode_batch_ranges.argtypes = [vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, vp, u64, vp, vp, sz, vp]
        l.mh_dev_decode_each_ranges.argtypes = [vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, vp, u64, vp, vp, sz, vp]
        l.mh_decode_batch_ranges.argtypes = [vp, vp, u64, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, sz, vp, vp]
        l.mh_decompress_each_ranges.argtypes = [vp, u64, vp, vp, u64, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, sz, vp, vp]
        l.mh_last_batch_range_upload_bytes.argtypes = []
        l.mh_last_batch_range_upload_bytes.restype = u64
        l.mh_dev_decode_ranges_o2_workspace.argtypes = [sz]
        l.mh_dev_decode_ranges_o2_workspace.restype = sz
        l.mh_dev_decode_ranges_o2.argtypes = l.mh_dev_decode_ranges.argtypes
        l.mh_decode_ranges_o2.argtypes = l.mh_decode_ranges.argtypes
        l.mh_dev_decode_batch_o2_ranges_workspace.argtypes = [sz]
        l.mh_dev_decode_batch_o2_ranges_workspace.restype = sz
        l.mh_dev_decode_batch_o2_ranges.argtypes = l.mh_dev_decode_batch_ranges.argtypes
        l.mh_decode_batch_o2_ranges.argtypes = l.mh_decode_batch_ranges.argtypes
        l.mh_dev_bank_select_workspace.argtypes = [sz, sz, sz]
        l.mh_dev_bank_select_workspace.restype = sz
        l.mh_dev_bank_select.argtypes = [vp, vp, vp, sz, sz, u8, vp, vp, vp, sz, vp]
        l.mh_dev_model_set_pick.argtypes = [vp, vp, sz, vp, C.POINTER(vp)]
        l.mh_dev_bank_train_workspace.argtypes = [sz, sz, u32]
        l.mh_dev_bank_train_workspace.restype = sz
        l.mh_dev_bank_train.argtypes = [vp, vp, sz, sz, i32, u8, u32, u32, vp, pi, vp, sz, vp, C.POINTER(vp)]
        l.mh_bank_train.argtypes = [vp, vp, sz, i32, u8, u32, u32, vp, pi, C.POINTER(vp)]
        l.mh_encode_bank_bound.argtypes = [vp, vp, vp, sz]
        l.mh_encode_bank_bound.restype = sz
        l.mh_encode_bank.argtypes = [vp, vp, vp, sz, u8, vp, vp, sz, vp, vp, vp, u32]
        l.mh_decode_bank.argtypes = [vp, vp, vp, vp, vp, sz, u8, vp, sz, vp, vp, u32, vp]
        l.mh_dev_batch_states_workspace.argtypes = [sz, u64]
        l.mh_dev_batch_states_workspace.restype = sz
        for fn in (l.mh_dev_batch_states, l.mh_dev_each_states):
            fn.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, vp, vp, sz, vp]
        for fn in (l.mh_dev_batch_index, l.mh_dev_each_index):
            fn.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, u64, u32, vp, vp, sz, vp]
        for fn in (l.mh_dev_batch_emit, l.mh_dev_each_emit):
            fn.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, vp, sz, vp]
        l.mh_index_batch.argtypes = [vp, vp, vp, vp, sz, u8, u32, vp, vp, u64, vp]
        l.mh_index_each.argtypes = [vp, vp, vp, vp, vp, sz, u8, u32, vp, vp, u64, vp]
        l.mh_pattern_set_create.argtypes = [vp, vp, sz, u32, C.POINTER(vp)]
        l.mh_pattern_set_size.argtypes = [vp]
        l.mh_pattern_set_size.restype = sz
        l.mh_pattern_set_max_len.argtypes = [vp]
        l.mh_pattern_set_free.argtypes = [vp]
        l.mh_pattern_set_free.restype = None
        l.mh_dev_find_batch_workspace.argtypes = [sz, u64, u32]
        l.mh_dev_find_batch_workspace.restype = sz
        for fn in (l.mh_dev_find_batch, l.mh_dev_find_each):
            fn.argtypes = [vp, vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, u32, vp, vp, vp, u64, vp, vp, sz, vp]
        l.mh_find_batch.argtypes = [vp, vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, vp, vp, u64, vp]
        for fn in (l.mh_dev_histogram_coded_workspace, l.mh_dev_recode_batch_workspace):
            fn.argtypes = [sz, u64, u32]
            fn.restype = sz
        for fn in (l.mh_dev_histogram_coded_batch, l.mh_dev_histogram_coded_each):
            fn.argtypes = [vp, i32, vp, vp, vp, sz, u64, u8, vp, u64, vp, u32, vp, vp, vp, sz, vp]
        for fn in (l.mh_dev_recode_batch, l.mh_dev_recode_each):
            fn.argtypes = [vp, vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp]
        l.mh_recode_batch.argtypes = [vp, vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, sz, vp, vp, vp, vp, vp]
        for fn in (l.mh_dev_find_batch_o2_workspace, l.mh_dev_histogram_coded_batch_o2_workspace, l.mh_dev_recode_batch_o2_workspace):
            fn.argtypes = [sz, u64, u32]
            fn.restype = sz
        l.mh_dev_find_batch_o2.argtypes = l.mh_dev_find_batch.argtypes
        l.mh_find_batch_o2.argtypes = l.mh_find_batch.argtypes
        l.mh_dict_create.argtypes = [vp, vp, sz, u32, C.POINTER(vp)]
        l.mh_dict_free.argtypes = [vp]
        l.mh_dict_free.restype = None
        for fn in (l.mh_dict_size, l.mh_dict_states, l.mh_dict_device_bytes):
            fn.argtypes = [vp]
            fn.restype = sz
        l.mh_dict_max_len.argtypes = [vp]
        l.mh_dict_classes.argtypes = [vp]
        l.mh_dict_find_bytes.argtypes = [vp, vp, sz, vp, vp, u64, pu64]
        l.mh_dev_find_dict_workspace.argtypes = [sz, u64, u32]
        l.mh_dev_find_dict_workspace.restype = sz
        for fn in (l.mh_dev_find_dict_batch, l.mh_dev_find_dict_each, l.mh_dev_find_dict_batch_o2):
            fn.argtypes = l.mh_dev_find_batch.argtypes
        l.mh_find_dict_batch.argtypes = l.mh_find_batch.argtypes
        l.mh_find_dict_batch_o2.argtypes = l.mh_find_batch.argtypes
        l.mh_dev_histogram_coded_batch_o2.argtypes = l.mh_dev_histogram_coded_batch.argtypes
        l.mh_dev_recode_batch_o2.argtypes = l.mh_dev_recode_batch.argtypes
        l.mh_recode_batch_o2.argtypes = l.mh_recode_batch.argtypes
        l.mh_dev_batch_states_o2_workspace.argtypes = [sz, u64]
        l.mh_dev_batch_states_o2_workspace.restype = sz
        l.mh_dev_batch_states_o2.argtypes = l.mh_dev_batch_states.argtypes
        l.mh_dev_batch_index_o2.argtypes = l.mh_dev_batch_index.argtypes
        l.mh_dev_batch_emit_o2.argtypes = l.mh_dev_batch_emit.argtypes
        l.mh_index_batch_o2.argtypes = l.mh_index_batch.argtypes
        l.mh_dev_batch_states_stats.argtypes = [vp, vp, C.POINTER(u32), pu64]
        l.mh_dev_crc_batch_workspace.argtypes = [sz, u64, u32]
        l.mh_dev_crc_batch_workspace.restype = sz
        for fn in (l.mh_dev_crc_batch, l.mh_dev_crc_each, l.mh_dev_crc_batch_o2):
            fn.argtypes = [vp, vp, vp, vp, sz, u64, u8, vp, u64, vp, u32, vp, vp, vp, vp, sz, vp]
        for fn in (l.mh_crc_batch, l.mh_crc_batch_o2):
            fn.argtypes = [vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, vp, vp]
        l.mh_dev_crc_raw_batch_workspace.argtypes = [sz, sz]
        l.mh_dev_crc_raw_batch_workspace.restype = sz
        l.mh_dev_crc_raw_batch.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp]
        l.mh_crc32_combine.argtypes = [u32, u32, u64]
        l.mh_crc32_combine.restype = u32
        l.mh_spans_from_hits.argtypes = [vp, vp, u64, sz, vp, vp]
        l.mh_dev_spans_from_hits_workspace.argtypes = [sz, u64]
        l.mh_dev_spans_from_hits_workspace.restype = sz
        l.mh_dev_spans_from_hits.argtypes = [vp, vp, u64, sz, vp, vp, vp, sz, vp]
        l.mh_dev_recode_edit_workspace.argtypes = [sz, u64, u32]
        l.mh_dev_recode_edit_workspace.restype = sz
        for fn in (l.mh_dev_recode_edit_batch, l.mh_dev_recode_edit_each):
            fn.argtypes = l.mh_dev_recode_batch.argtypes[:12] + [vp, vp, vp] + l.mh_dev_recode_batch.argtypes[12:]
        l.mh_recode_edit_batch.argtypes = l.mh_recode_batch.argtypes[:10] + [vp, vp, vp] + l.mh_recode_batch.argtypes[10:]
        l.mh_dev_recode_splice_workspace.argtypes = [sz, u64, u32, u64]
        l.mh_dev_recode_splice_workspace.restype = sz
        for fn in (l.mh_dev_recode_splice_batch, l.mh_dev_recode_splice_each):
            fn.argtypes = l.mh_dev_recode_batch.argtypes[:12] + [vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, u64, vp, vp, vp, sz, vp]
        l.mh_recode_splice_batch.argtypes = l.mh_recode_batch.argtypes[:10] + [vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, u64, vp, vp]
        l.mh_spans_from_hits_tagged.argtypes = [vp, vp, vp, u64, sz, vp, vp, vp]
        l.mh_dev_spans_from_hits_tagged_workspace.argtypes = [sz, u64]
        l.mh_dev_spans_from_hits_tagged_workspace.restype = sz
        l.mh_dev_spans_from_hits_tagged.argtypes = [vp, vp, vp, u64, sz, vp, vp, vp, vp, sz, vp]
        l.mh_dev_recode_splice_table_workspace.argtypes = [sz, u64, u32, u64, sz]
        l.mh_dev_recode_splice_table_workspace.restype = sz
        for fn in (l.mh_dev_recode_splice_table_batch, l.mh_dev_recode_splice_table_each):
            fn.argtypes = l.mh_dev_recode_batch.argtypes[:12] + [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, u64, vp, vp, vp, sz, vp]
        l.mh_recode_splice_table_batch.argtypes = l.mh_recode_batch.argtypes[:10] + [vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, u64, vp, vp]
        l.mh_dev_recode_edit_batch_o2_workspace.argtypes = [sz, u64, u32]
        l.mh_dev_recode_edit_batch_o2_workspace.restype = sz
        l.mh_dev_recode_splice_table_batch_o2_workspace.argtypes = [sz, u64, u32, u64, sz]
        l.mh_dev_recode_splice_table_batch_o2_workspace.restype = sz
        l.mh_dev_recode_edit_batch_o2.argtypes = [C.POINTER(RecodeEditO2Args)]
        l.mh_dev_recode_splice_table_batch_o2.argtypes = [C.POINTER(RecodeSpliceO2Args)]
        l.mh_recode_edit_batch_o2.argtypes = l.mh_recode_edit_batch.argtypes
        l.mh_recode_splice_table_batch_o2.argtypes = l.mh_recode_splice_table_batch.argtypes
        l.mh_dev_select_batch_workspace.argtypes = [sz, sz]
        l.mh_dev_select_batch_workspace.restype = sz
        l.mh_dev_select_batch.argtypes = [C.POINTER(SelectArgs)]
        l.mh_dev_picks_from_hits_workspace.argtypes = [sz]
        l.mh_dev_picks_from_hits_workspace.restype = sz
        l.mh_dev_picks_from_hits.argtypes = [C.POINTER(PicksArgs)]
        l.mh_select_batch.argtypes = [C.POINTER(CodedBatchArgs), u32, vp, sz, vp, sz, vp, vp, vp, vp, u64, u32, vp]
        l.mh_picks_from_hits.argtypes = [vp, vp, sz, u32, u32, vp, vp]
        l.mh_span_token_digest.argtypes = [vp, vp, sz, u32]
        l.mh_span_token_digest.restype = u64
        l.mh_dev_span_tokens_workspace.argtypes = [sz, sz]
        l.mh_dev_span_tokens_workspace.restype = sz
        l.mh_dev_span_tokens_batch.argtypes = [C.POINTER(SpanTokensArgs), C.POINTER(Launch)]
        l.mh_span_tokens_batch.argtypes = [vp, vp, vp, vp, sz, u8, vp, vp, u32, vp, vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, sz, vp, vp]
        _lib = l
    return _lib


def _check(status, what):
    if status != MH_OK:
        raise MhError(status, what)


def device_count():
    return lib().mh_device_count()


def _u8(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data if a.size else None


class _DeviceMemory:
    """The process-wide allocation mode of DeviceBuffer (device_memory below).  `served` / `missed`: the requests without
    `init` that the recycle pool did / did not serve."""

    def __init__(self):
        self.mode, self.byte, self.pool, self.served, self.missed = None, 0, [], 0, 0

    def take(self, nbytes):
        """Best fit: the smallest pooled block of at least nbytes as (address, block size), or None."""
        fit = [k for k, (cap, _) in enumerate(self.pool) if cap >= nbytes]
        if not fit:
            return None
        cap, addr = self.pool.pop(min(fit, key=lambda k: self.pool[k][0]))
        return addr, cap

    def drain(self):
        while self.pool:
            _lib.mh_dev_free(C.c_void_p(self.pool.pop()[1]))


_memory = _DeviceMemory()


class device_memory:
    """Context manager of DeviceBuffer's allocation mode, for tests of dirty and reused workspaces and outputs (process-wide,
    not nested; outside it DeviceBuffer is a plain hipMalloc / hipFree):
      device_memory("fill", byte)   every buffer created without `init` is filled with `byte` before it is handed out;
      device_memory("recycle")      freed buffers go to a pool that is never cleared, a request takes the smallest pooled block
                                    of at least its size and keeps the block's contents (`init`, when given, is uploaded over its
                                    front); leaving the mode frees the pool.
    `with` yields the mode's state: .served / .missed count the requests without `init` that the pool did / did not serve."""

    def __init__(self, mode, byte=0):
        if mode not in ("fill", "recycle"):
            raise ValueError("device_memory mode")
        self.mode, self.byte = mode, byte

    def __enter__(self):
        if _memory.mode is not None:
            raise RuntimeError("device_memory does not nest")
        lib()
        _memory.mode, _memory.byte, _memory.served, _memory.missed = self.mode, self.byte, 0, 0
        return _memory

    def __exit__(self, *exc):
        _memory.mode = None
        _memory.drain()
        return False


class DeviceBuffer:
    """A hipMalloc'ed buffer (for tests that drive the mh_dev_* calls without torch).  Without `init` its contents are
    whatever the allocator returned, or what device_memory arranges."""

    def __init__(self, nbytes, init=None):
        self.nbytes = self.block = nbytes
        self.ptr = C.c_void_p()
        got = _memory.take(nbytes) if _memory.mode == "recycle" else None
        if _memory.mode == "recycle" and init is None:
            _memory.served += got is not None
            _memory.missed += got is None
        if got is not None:
            self.ptr.value, self.block = got
        else:
            _check(lib().mh_dev_malloc(C.byref(self.ptr), nbytes), "mh_dev_malloc")
        if init is None and _memory.mode == "fill":
            init = np.full(nbytes, _memory.byte, dtype=np.uint8)
        if init is not None:
            a = np.ascontiguousarray(init)
            _check(lib().mh_dev_upload(self.ptr, a.ctypes.data, a.nbytes), "mh_dev_upload")

    def download(self, dtype=np.uint8):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().mh_dev_download(out.ctypes.data, self.ptr, out.nbytes), "mh_dev_download")
        return out

    def __del__(self):
        if getattr(self, "ptr", None) and _lib is not None:
            if _memory.mode == "recycle":
                _memory.pool.append((self.block, self.ptr.value))
            else:
                _lib.mh_dev_free(self.ptr)
            self.ptr = None


def histogram_o1(data, prev0=PREV0):
    a = _u8(data)
    out = np.zeros(65536, dtype=np.uint64)
    _check(lib().mh_histogram_o1(_ptr(a), a.size, prev0, out.ctypes.data), "mh_histogram_o1")
    return out


def histogram_o0(data):
    a = _u8(data)
    out = np.zeros(256, dtype=np.uint64)
    _check(lib().mh_histogram_o0(_ptr(a), a.size, out.ctypes.data), "mh_histogram_o0")
    return out


def histogram_o2(data):
    """Order-2 extension (parity unpinned): counts[ctx * 256 + sym], ctx = the two previous bytes."""
    a = _u8(data)
    out = np.zeros(1 << 24, dtype=np.uint64)
    _check(lib().mh_histogram_o2(_ptr(a), a.size, out.ctypes.data), "mh_histogram_o2")
    return out


def batch_offsets(messages):
    """(concatenation as uint8, in_off[n + 1] as uint64) of a list of byte strings."""
    msgs = [bytes(m) for m in messages]
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    return np.frombuffer(b"".join(msgs), dtype=np.uint8), off


def histogram_o1_batch(messages, prev0=PREV0, order=1):
    """Summed histogram of independent messages, each starting in context prev0 (mh_dev_histogram_o1_batch / _o0_batch):
    the training counts of a shared model."""
    data, off = batch_offsets(messages)
    l = lib()
    total, n = int(data.size), len(off) - 1
    d_data = DeviceBuffer(max(total, 1), data if total else None)
    d_off = DeviceBuffer(off.nbytes, off)
    nc = 65536 if order else 256
    d_counts = DeviceBuffer(nc * 8)
    wsb = l.mh_dev_histogram_batch_workspace(total)
    d_ws = DeviceBuffer(wsb)
    if order:
        _check(l.mh_dev_histogram_o1_batch(d_data.ptr, d_off.ptr, n, total, prev0, d_counts.ptr, d_ws.ptr, wsb, None), "mh_dev_histogram_o1_batch")
    else:
        _check(l.mh_dev_histogram_o0_batch(d_data.ptr, d_off.ptr, n, total, d_counts.ptr, d_ws.ptr, wsb, None), "mh_dev_histogram_o0_batch")
    _check(l.mh_dev_status(d_ws.ptr, None), "mh_dev_histogram_batch")
    return d_counts.download(np.uint64)


def histogram_o2_batch(messages, prev0=PREV0):
    """Summed order-2 histogram of independent messages, each starting in context (prev0, prev0) (mh_dev_histogram_o2_batch):
    the training counts of a shared order-2 model, counts[ctx * 256 + sym] (extension, parity unpinned)."""
    data, off = batch_offsets(messages)
    l = lib()
    total, n = int(data.size), len(off) - 1
    d_data = DeviceBuffer(max(total, 1), data if total else None)
    d_off = DeviceBuffer(off.nbytes, off)
    d_counts = DeviceBuffer((1 << 24) * 8)
    wsb = l.mh_dev_histogram_o2_batch_workspace(total)
    d_ws = DeviceBuffer(wsb)
    _check(l.mh_dev_histogram_o2_batch(d_data.ptr, d_off.ptr, n, total, prev0, d_counts.ptr, d_ws.ptr, wsb, None), "mh_dev_histogram_o2_batch")
    _check(l.mh_dev_status(d_ws.ptr, None), "mh_dev_histogram_o2_batch")
    return d_counts.download(np.uint64)


# ---- lookups into batches (include/mh.h, "RANDOM ACCESS INTO BATCHES") -----------------------------------------------------
RANGE_GUARD = 64          # bytes of 0xA5 in front of, between and behind the outputs of the device-call wrappers
RANGE_FILL = 0xA5


def _lookups(lookups):
    return np.ascontiguousarray(np.asarray(lookups, dtype=np.uint64).reshape(-1, 3))


def _lookup_lengths(lk, nbits, sym_off):
    """Output length of every lookup that can be served: end - begin, 0 for a lookup refused by its arguments alone."""
    n = len(nbits)
    s, b, e = lk[:, 0], lk[:, 1], lk[:, 2]
    ok = (s < np.uint64(n)) & (b <= e)
    si = np.where(ok, s, 0).astype(np.int64)
    if sym_off is not None:
        so = np.asarray(sym_off, dtype=np.uint64)
        bound = so[si + 1] - so[si] if n else np.zeros(len(lk), dtype=np.uint64)
    else:
        bound = np.asarray(nbits, dtype=np.uint64)[si] if n else np.zeros(len(lk), dtype=np.uint64)
    ok &= e <= bound
    return np.where(ok, e - b, np.uint64(0)).astype(np.uint64)


def _dev_batch_ranges(fn, handle, payload, pay_off, nbits, lookups, prev0, sym_off, index, chunk_symbols, out_cap):
    """One mh_dev_decode_batch_ranges / mh_dev_decode_each_ranges call with RANGE_GUARD bytes of RANGE_FILL around every
    output.  Returns (list of bytes per lookup, int32 status per lookup, mh_dev_status); asserts that no byte changed outside
    the outputs of the lookups that were decoded (a lookup that failed while decoding may have written part of its own)."""
    l = lib()
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    lk = _lookups(lookups)
    m = lk.shape[0]
    ln = np.where(lk[:, 1] <= lk[:, 2], np.minimum(lk[:, 2] - lk[:, 1], np.uint64(1 << 24)), np.uint64(0)).astype(np.uint64)
    at = np.zeros(max(m, 1), dtype=np.uint64)
    pos = RANGE_GUARD
    for j in range(m):
        at[j] = pos
        pos += int(ln[j]) + RANGE_GUARD
    full = pos
    cap = full if out_cap is None else out_cap
    size = max(full, cap) + RANGE_GUARD
    d_pl = DeviceBuffer(max(payload.size, 1) + 64, payload if payload.size else None)
    d_po, d_nb = DeviceBuffer(pay_off.nbytes, pay_off), DeviceBuffer(max(nbits.nbytes, 8), nbits if n else None)
    d_so = DeviceBuffer(max(n + 1, 1) * 8, np.ascontiguousarray(sym_off, dtype=np.uint64)) if sym_off is not None else None
    d_idx = None
    if index is not None:
        index = np.ascontiguousarray(index, dtype=np.uint64)
        d_idx = DeviceBuffer(max(index.nbytes, 8), index if index.size else None)
    d_lk = DeviceBuffer(max(lk.nbytes, 24), lk if m else None)
    d_at = DeviceBuffer(at.nbytes, at)
    d_out = DeviceBuffer(size, np.full(size, RANGE_FILL, dtype=np.uint8))
    d_st = DeviceBuffer(max(m, 1) * 4, np.full(max(m, 1), 99, dtype=np.int32))
    wsb = l.mh_dev_decode_batch_ranges_workspace(m)
    d_ws = DeviceBuffer(wsb)
    _check(fn(handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, prev0, d_so.ptr if d_so else None, d_idx.ptr if d_idx else None, chunk_symbols,
              d_lk.ptr, m, d_out.ptr, d_at.ptr, cap, d_st.ptr, d_ws.ptr, wsb, None), "mh_dev_decode_*_ranges")
    rc = l.mh_dev_status(d_ws.ptr, None)
    out = d_out.download()
    st = d_st.download(np.int32)[:m]
    may = np.zeros(size, dtype=bool)
    for j in range(m):
        if st[j] in (MH_OK, MH_ERR_CORRUPT, MH_ERR_ARG):        # (MH_ERR_ARG: an index-free walk that ended before `end`)
            may[int(at[j]):int(at[j]) + int(ln[j])] = True
    assert (out[~may] == RANGE_FILL).all(), "bytes written outside the outputs of the lookups that decoded"
    res = [out[int(at[j]):int(at[j]) + int(lk[j, 2] - lk[j, 1])].tobytes() if st[j] == MH_OK else b"" for j in range(m)]
    return res, st, rc


def _host_batch_ranges(call, name, lk, nbits, sym_off):
    """Runs call(out, cap, out_off, status) of a host form; (list of bytes per lookup, int32 status per lookup)."""
    m = lk.shape[0]
    cap = int(np.sum(_lookup_lengths(lk, nbits, sym_off), dtype=np.uint64)) if m else 0
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    out_off = np.zeros(m + 1, dtype=np.uint64)
    st = np.zeros(max(m, 1), dtype=np.int32)
    rc = call(out.ctypes.data, cap, out_off.ctypes.data, st.ctypes.data)
    st = st[:m]
    if rc != MH_OK and not np.any(st == rc):
        raise MhError(rc, name)
    return [out[int(out_off[j]):int(out_off[j + 1])].tobytes() if st[j] == MH_OK else b"" for j in range(m)], st


def last_batch_range_upload_bytes():
    return lib().mh_last_batch_range_upload_bytes()


# ---- search in batches (include/mh.h, "SEARCH IN BATCHES") -------------------------------------------------------------------
FIND_GUARD = 8            # guard words of FIND_FILL behind the hit records, the pattern numbers and hit_off
FIND_FILL = 0xA5A5A5A5A5A5A5A5


class PatternSet:
    """Owns an mh_pattern_set*: up to FIND_MAX_POSITIONS bytes of patterns in all (a host object, no device needed)."""

    def __init__(self, patterns, fold=False, flags=None):
        pats = [bytes(p) for p in patterns]
        buf = np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8)
        off = np.zeros(len(pats) + 1, dtype=np.uint32)
        if pats:
            off[1:] = np.cumsum([len(p) for p in pats])
        h = C.c_void_p()
        _check(lib().mh_pattern_set_create(buf.ctypes.data, off.ctypes.data, len(pats),
                                           (FIND_FOLD_ASCII if fold else 0) if flags is None else flags, C.byref(h)), "mh_pattern_set_create")
        self._h = h
        self.patterns = pats

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mh_pattern_set_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return lib().mh_pattern_set_size(self._h)

    @property
    def max_len(self):
        return lib().mh_pattern_set_max_len(self._h)


class Dict:
    """Owns an mh_dict*: a dictionary of up to DICT_MAX_PATTERNS patterns of at most DICT_MAX_LEN bytes each, as an Aho-Corasick
    DFA (include/mh.h, "DICTIONARY SEARCH IN BATCHES").  Built on the host; with a device its image is uploaded as well.  The
    find_dict calls take it where the find calls take a PatternSet."""

    def __init__(self, patterns, fold=False, flags=None):
        pats = [bytes(p) for p in patterns]
        buf = np.frombuffer(b"".join(pats) or b"\0", dtype=np.uint8)
        off = np.zeros(len(pats) + 1, dtype=np.uint32)
        if pats:
            off[1:] = np.cumsum([len(p) for p in pats])
        h = C.c_void_p()
        _check(lib().mh_dict_create(buf.ctypes.data, off.ctypes.data, len(pats),
                                    (FIND_FOLD_ASCII if fold else 0) if flags is None else flags, C.byref(h)), "mh_dict_create")
        self._h = h
        self.patterns = pats

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mh_dict_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return lib().mh_dict_size(self._h)

    @property
    def max_len(self):
        return lib().mh_dict_max_len(self._h)

    @property
    def states(self):
        return lib().mh_dict_states(self._h)

    @property
    def classes(self):
        return lib().mh_dict_classes(self._h)

    @property
    def device_bytes(self):
        return lib().mh_dict_device_bytes(self._h)

    def find_bytes(self, data, hit_cap=None):
        """mh_dict_find_bytes (host matcher, no device): (hits[k, 2] = (begin, end), hit_pattern[k], total, return code) of one
        message in (end, pattern) order.  hit_cap None: a counting call first, then one with room for every hit."""
        l = lib()
        data = _u8(data)
        total = C.c_uint64(0)
        if hit_cap is None:
            _check(l.mh_dict_find_bytes(self._h, _ptr(data), data.size, None, None, 0, C.byref(total)), "mh_dict_find_bytes")
            hit_cap = total.value
        hits, pat = np.zeros(max(hit_cap, 1) * 2, dtype=np.uint64), np.zeros(max(hit_cap, 1), dtype=np.uint32)
        rc = l.mh_dict_find_bytes(self._h, _ptr(data), data.size, hits.ctypes.data, pat.ctypes.data, hit_cap, C.byref(total))
        if rc not in (MH_OK, MH_ERR_CAPACITY):
            raise MhError(rc, "mh_dict_find_bytes")
        k = min(total.value, hit_cap)
        return hits[:2 * k].reshape(-1, 2), pat[:k], total.value, rc


def _dev_find(fn, handle, ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap, count_only, ws_fn=None):
    """One mh_dev_find_batch / mh_dev_find_each call.  hit_cap None: a count-only call first, then one with room for every
    hit.  Returns (hit_off[n + 1], hits[k, 3], hit_pattern[k], per-stream status[n], mh_dev_status), k = min(total, hit_cap)
    (0 when count_only); asserts that the FIND_GUARD words behind the records, the pattern numbers and hit_off, and every
    record at or beyond hit_cap, kept their fill."""
    l = lib()
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    d_pl = DeviceBuffer(max(payload.size, 1) + 64, payload if payload.size else None)
    d_po, d_nb = DeviceBuffer(pay_off.nbytes, pay_off), DeviceBuffer(max(nbits.nbytes, 8), nbits if n else None)
    d_so, d_idx, sym_total = None, None, 0
    if index is not None:
        so = np.ascontiguousarray(sym_off, dtype=np.uint64)
        sym_total = int(so[n])
        d_so = DeviceBuffer(so.nbytes, so)
        index = np.ascontiguousarray(index, dtype=np.uint64)
        d_idx = DeviceBuffer(max(index.nbytes, 8), index if index.size else None)
    wsb = (ws_fn or l.mh_dev_find_batch_workspace)(n, sym_total, chunk_symbols if index is not None else 0)
    d_ws = DeviceBuffer(wsb)
    d_st = DeviceBuffer(max(n, 1) * 4, np.full(max(n, 1), 99, dtype=np.int32))

    def call(d_hits, d_pat, cap):
        d_ho = DeviceBuffer((n + 1 + FIND_GUARD) * 8, np.full(n + 1 + FIND_GUARD, FIND_FILL, dtype=np.uint64))
        _check(fn(handle, ps.handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), prev0, d_so.ptr if d_so else None, sym_total,
                  d_idx.ptr if d_idx else None, chunk_symbols, d_ho.ptr, d_hits.ptr if d_hits else None, d_pat.ptr if d_pat else None, cap,
                  d_st.ptr, d_ws.ptr, wsb, None), "mh_dev_find_*")
        rc = l.mh_dev_status(d_ws.ptr, None)
        ho = d_ho.download(np.uint64)
        assert (ho[n + 1:] == FIND_FILL).all(), "words written behind hit_off"
        return ho[:n + 1], rc

    none = (np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    if count_only or hit_cap is None:
        ho, rc = call(None, None, 0)
        if count_only:
            return (ho,) + none + (d_st.download(np.int32)[:n], rc)
    cap = int(ho[n]) if hit_cap is None else hit_cap
    room = cap + FIND_GUARD
    d_hits = DeviceBuffer(room * 24, np.full(room * 3, FIND_FILL, dtype=np.uint64))
    d_pat = DeviceBuffer(room * 4, np.full(room, FIND_FILL & 0xFFFFFFFF, dtype=np.uint32))
    ho, rc = call(d_hits, d_pat, cap)
    hits, pat = d_hits.download(np.uint64), d_pat.download(np.uint32)
    k = min(int(ho[n]), cap)
    assert (hits[3 * k:] == FIND_FILL).all() and (pat[k:] == FIND_FILL & 0xFFFFFFFF).all(), "records written at or beyond the hits / hit_cap"
    return ho, hits[:3 * k].reshape(-1, 3), pat[:k], d_st.download(np.int32)[:n], rc


# ---- re-coding batches (include/mh.h, "RE-CODING BATCHES") -------------------------------------------------------------------
def _dev_source(payload, pay_off, nbits, sym_off, index):
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    d_pl = DeviceBuffer(max(payload.size, 1) + 64, payload if payload.size else None)
    d_po, d_nb = DeviceBuffer(pay_off.nbytes, pay_off), DeviceBuffer(max(nbits.nbytes, 8), nbits if n else None)
    so, d_idx = None, None
    if index is not None:
        so = np.ascontiguousarray(sym_off, dtype=np.uint64)
        index = np.ascontiguousarray(index, dtype=np.uint64)
        d_idx = DeviceBuffer(max(index.nbytes, 8), index if index.size else None)
    return n, int(pay_off[n]), d_pl, d_po, d_nb, so, d_idx


# ---- digests of batches (include/mh.h, "DIGESTS OF BATCHES") ---------------------------------------------------------------
def _guarded(nbytes):
    """A DeviceBuffer of nbytes + FIND_GUARD words of FIND_FILL behind them.  The front is created without `init`, so that the
    device_memory modes reach it."""
    d = DeviceBuffer(nbytes + FIND_GUARD * 8)
    g = np.full(FIND_GUARD, FIND_FILL, dtype=np.uint64)
    _check(lib().mh_dev_upload(C.c_void_p(d.ptr.value + nbytes), g.ctypes.data, g.nbytes), "mh_dev_upload")
    return d


def _guard_kept(d, nbytes):
    return (d.download(np.uint8)[nbytes:nbytes + FIND_GUARD * 8].view(np.uint64) == FIND_FILL).all()


def _dev_crc(fn, handle, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, want_len=True, want_status=True):
    """One mh_dev_crc_batch / mh_dev_crc_each / mh_dev_crc_batch_o2 call: (crc[n] uint32, len[n] uint64 or None, per-stream
    status[n] or None, mh_dev_status); asserts that the FIND_GUARD words behind crc and len kept their fill.  The outputs, the
    statuses and the workspace are created without contents of their own."""
    l = lib()
    n, pay_total, d_pl, d_po, d_nb, so, d_idx = _dev_source(payload, pay_off, nbits, sym_off, index)
    sym_total = int(so[n]) if so is not None else 0
    d_so = DeviceBuffer(so.nbytes, so) if so is not None else None
    wsb = l.mh_dev_crc_batch_workspace(n, sym_total, chunk_symbols if index is not None else 0)
    d_ws = DeviceBuffer(wsb)
    d_crc = _guarded(n * 4)
    d_len = _guarded(n * 8) if want_len else None
    d_st = DeviceBuffer(max(n, 1) * 4) if want_status else None
    _check(fn(handle, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, prev0, d_so.ptr if d_so else None, sym_total, d_idx.ptr if d_idx else None,
              chunk_symbols, d_crc.ptr, d_len.ptr if d_len else None, d_st.ptr if d_st else None, d_ws.ptr, wsb, None), "mh_dev_crc_*")
    rc = l.mh_dev_status(d_ws.ptr, None)
    assert _guard_kept(d_crc, n * 4) and (d_len is None or _guard_kept(d_len, n * 8)), "words written behind crc / len"
    return (d_crc.download(np.uint32)[:n], d_len.download(np.uint64)[:n] if d_len else None,
            d_st.download(np.int32)[:n] if d_st else None, rc)


def crc_raw_batch(messages, shift=0):
    """mh_dev_crc_raw_batch of a list of byte strings: (crc[n] uint32, mh_dev_status).  `shift`: d_data starts that many bytes
    into its allocation (an odd address)."""
    l = lib()
    data, off = batch_offsets(messages)
    n, total = len(off) - 1, int(data.size)
    d_data = DeviceBuffer(shift + total + 16, np.concatenate([np.zeros(shift, dtype=np.uint8), data, np.zeros(16, dtype=np.uint8)]))
    d_off = DeviceBuffer(off.nbytes, off)
    wsb = l.mh_dev_crc_raw_batch_workspace(n, total)
    d_ws = DeviceBuffer(wsb)
    d_crc = _guarded(n * 4)
    _check(l.mh_dev_crc_raw_batch(C.c_void_p(d_data.ptr.value + shift), d_off.ptr, n, total, d_crc.ptr, d_ws.ptr, wsb, None), "mh_dev_crc_raw_batch")
    rc = l.mh_dev_status(d_ws.ptr, None)
    assert _guard_kept(d_crc, n * 4), "words written behind crc"
    return d_crc.download(np.uint32)[:n], rc


def crc32_combine(crc_a, crc_b, len_b):
    """mh_crc32_combine (host arithmetic): the CRC-32 of A || B from those of A and B and len(B)."""
    return int(lib().mh_crc32_combine(crc_a, crc_b, len_b))


def _host_crc(fn, what, handle, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, check):
    """mh_crc_batch / mh_crc_batch_o2 (host form): (crc[n] uint32, len[n] uint64, per-stream status[n], return code).
    check=False returns a failed stream's status instead of raising."""
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    so = np.ascontiguousarray(sym_off, dtype=np.uint64) if sym_off is not None else None
    idx = np.ascontiguousarray(index, dtype=np.uint64) if index is not None else None
    crc, ln, st = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.int32)
    rc = fn(handle, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0, so.ctypes.data if so is not None else None,
            (idx.ctypes.data if idx.size else pay_off.ctypes.data) if idx is not None else None, chunk_symbols, crc.ctypes.data, ln.ctypes.data,
            st.ctypes.data)
    if rc != MH_OK and (check or not st[:n].any()):
        raise MhError(rc, what)
    return crc[:n], ln[:n], st[:n], rc


def _dev_histogram_coded(fn, handle, order, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, ws_fn=None):
    """One mh_dev_histogram_coded_batch / _each / _batch_o2 call: (counts[256, 65536 or 1 << 24], per-stream status[n],
    mh_dev_status); asserts that the FIND_GUARD words behind the counts kept their fill."""
    l = lib()
    n, pay_total, d_pl, d_po, d_nb, so, d_idx = _dev_source(payload, pay_off, nbits, sym_off, index)
    sym_total = int(so[n]) if so is not None else 0
    d_so = DeviceBuffer(so.nbytes, so) if so is not None else None
    nc = (1 << 24) if order == 2 else (65536 if order else 256)
    d_counts = DeviceBuffer((nc + FIND_GUARD) * 8, np.full(nc + FIND_GUARD, FIND_FILL, dtype=np.uint64))
    wsb = (ws_fn or l.mh_dev_histogram_coded_workspace)(n, sym_total, chunk_symbols if index is not None else 0)
    d_ws = DeviceBuffer(wsb)
    d_st = DeviceBuffer(max(n, 1) * 4, np.full(max(n, 1), 99, dtype=np.int32))
    _check(fn(handle, order, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, prev0, d_so.ptr if d_so else None, sym_total,
              d_idx.ptr if d_idx else None, chunk_symbols, d_counts.ptr, d_st.ptr, d_ws.ptr, wsb, None), "mh_dev_histogram_coded_*")
    rc = l.mh_dev_status(d_ws.ptr, None)
    counts = d_counts.download(np.uint64)
    assert (counts[nc:] == FIND_FILL).all(), "words written behind the counts"
    return counts[:nc], d_st.download(np.int32)[:n], rc


def _dev_recode(fn, src, dst, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, cap=None, count_only=False, want_index=True,
                sym_total=None, ws_fn=None):
    """One mh_dev_recode_batch / mh_dev_recode_each call with guards around every output.  cap None: a count-only call first,
    then one with exactly out_off[n] bytes of room.  Index-free (index None) with a destination index and no sym_total: the
    count-only call sizes it.  Returns a dict: payload (the min(cap, out_off[n]) bytes), out_off[n + 1], nbits[n], index (the whole
    array, FIND_FILL where no slice lies, or None), dropped[n], status[n], sym_off[n + 1], rc (mh_dev_status).  Asserts that
    nothing changed outside out_off[n] payload bytes, the n + 1 offsets, the n lengths and counts and the index slices of the
    streams that passed."""
    l = lib()
    n, pay_total, d_pl, d_po, d_nb, so, d_idx = _dev_source(payload, pay_off, nbits, sym_off, index)
    indexed = index is not None
    G, F = FIND_GUARD, FIND_FILL
    d_st = DeviceBuffer(max(n, 1) * 4, np.full(max(n, 1), 99, dtype=np.int32))

    def call(room, with_payload, with_index, st):
        d_so = DeviceBuffer((n + 1 + G) * 8, np.concatenate([so if indexed else np.full(n + 1, F, dtype=np.uint64), np.full(G, F, dtype=np.uint64)]))
        wsb = (ws_fn or l.mh_dev_recode_batch_workspace)(n, st, chunk_symbols if indexed else 0)
        d_ws = DeviceBuffer(wsb)
        d_out = DeviceBuffer(room + RANGE_GUARD + 16, np.full(room + RANGE_GUARD + 16, RANGE_FILL, dtype=np.uint8)) if with_payload else None
        d_oo = DeviceBuffer((n + 1 + G) * 8, np.full(n + 1 + G, F, dtype=np.uint64))
        d_onb = DeviceBuffer((n + G) * 8, np.full(n + G, F, dtype=np.uint64))
        d_dr = DeviceBuffer((n + G) * 8, np.full(n + G, F, dtype=np.uint64))
        nidx = int(l.mh_batch_index_capacity(st, n, chunk_symbols)) if with_index else 0
        d_oi = DeviceBuffer((nidx + G) * 8, np.full(nidx + G, F, dtype=np.uint64)) if with_index else None
        _check(fn(src, dst, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, prev0, d_so.ptr, st, d_idx.ptr if d_idx else None, chunk_symbols,
                  d_out.ptr if d_out else None, room, d_oo.ptr, d_onb.ptr, d_oi.ptr if d_oi else None, d_dr.ptr, d_st.ptr, d_ws.ptr, wsb, None),
               "mh_dev_recode_*")
        rc = l.mh_dev_status(d_ws.ptr, None)
        oo, onb, dr, dso = d_oo.download(np.uint64), d_onb.download(np.uint64), d_dr.download(np.uint64), d_so.download(np.uint64)
        status = d_st.download(np.int32)[:n]
        assert (oo[n + 1:] == F).all() and (onb[n:] == F).all() and (dr[n:] == F).all() and (dso[n + 1:] == F).all(), "words written behind an output"
        if indexed:
            assert np.array_equal(dso[:n + 1], so), "sym_off written with an index"
        res = dict(out_off=oo[:n + 1], nbits=onb[:n], dropped=dr[:n], status=status, sym_off=dso[:n + 1], rc=rc, payload=None, index=None)
        if d_out:
            out = d_out.download(np.uint8)
            used = min(int(oo[n]), room) if rc != MH_ERR_CAPACITY else 0
            assert (out[used:] == RANGE_FILL).all(), "bytes written at or beyond min(cap, out_off[n])"
            res["payload"] = out[:used].copy()
        if d_oi:
            oi = d_oi.download(np.uint64)
            mine = np.zeros(nidx + G, dtype=bool)
            if rc != MH_ERR_CAPACITY and dso[n] != F:
                for i in range(n):
                    if status[i] == MH_OK:
                        b = int(dso[i]) // chunk_symbols + i
                        mine[b:b + (int(dso[i + 1] - dso[i]) + chunk_symbols - 1) // chunk_symbols] = True
            assert (oi[~mine] == F).all(), "index entries written outside the slices of the streams that passed"
            res["index"] = oi[:nidx]
        return res

    st = int(so[n]) if indexed else (sym_total or 0)
    idx_now = want_index and bool(chunk_symbols) and (indexed or sym_total is not None)
    if count_only:
        return call(0, False, idx_now, st)
    if cap is None or (want_index and chunk_symbols and not indexed and sym_total is None):
        pre = call(0, False, False, st)
        if cap is None:
            cap = int(pre["out_off"][n])
        if not indexed and sym_total is None:
            st = int(pre["sym_off"][n])
    return call(cap, True, want_index and bool(chunk_symbols), st)


# ---- editing batches (include/mh.h, "EDITING BATCHES") ---------------------------------------------------------------------
def _span_arrays(span_off, spans, byte_map):
    """(span_off[n + 1] uint64 or None, spans as flat uint64 pairs, the 256-byte map) as contiguous arrays."""
    so = None if span_off is None else np.ascontiguousarray(span_off, dtype=np.uint64)
    sp = np.zeros(0, dtype=np.uint64) if spans is None else np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
    m = _u8(byte_map)
    if m.size != 256:
        raise ValueError("the byte map has 256 entries")
    return so, sp, m


def _dev_recode_edit(fn, src, dst, payload, pay_off, nbits, byte_map, span_off, spans, prev0, sym_off, index, chunk_symbols, ws_fn=None, **kw):
    """One mh_dev_recode_edit_batch / _each call through _dev_recode: the same guards around every output, the same dict.
    ws_fn: the sizing call (default mh_dev_recode_edit_workspace)."""
    so, sp, m = _span_arrays(span_off, spans, byte_map)
    d_so = DeviceBuffer(so.nbytes, so) if so is not None else None
    d_sp = DeviceBuffer(max(sp.nbytes, 16), sp if sp.size else None)
    d_map = DeviceBuffer(256, m)

    def call(*a):
        return fn(*a[:12], d_so.ptr if d_so else None, d_sp.ptr, d_map.ptr, *a[12:])

    return _dev_recode(call, src, dst, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, ws_fn=ws_fn or lib().mh_dev_recode_edit_workspace, **kw)


# ---- splicing batches (include/mh.h, "SPLICING BATCHES") -------------------------------------------------------------------
SPLICE_MAX_REP = 255                       # include/mh.h MH_SPLICE_MAX_REP


def _rep_table(reps):
    """A replacement table as the _splice_table calls take it: (rep_off[n_reps + 1], rep_bytes) from a list of byte strings, or
    the pair itself when the caller passes one (a malformed table, for the refusals)."""
    if isinstance(reps, tuple):
        return np.ascontiguousarray(reps[0], dtype=np.uint64), _u8(reps[1])
    off = np.zeros(len(reps) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reps], dtype=np.uint64)
    return off, _u8(b"".join(bytes(r) for r in reps))


def _dev_recode_splice(fn, src, dst, payload, pay_off, nbits, rep, span_off, spans, prev0, sym_off, index, chunk_symbols, cap=None,
                       count_only=False, want_index=True, index_cap=None, n_spans=None, table=None, n_reps=None, ws_fn=None):
    """One mh_dev_recode_splice_batch / _each call with guards around every output, as _dev_recode puts them.  cap None or
    index_cap None: a count-only call first, then one with exactly out_off[n] bytes and (out_sym_off[n] // chunk) + n entries of
    room.  Returns the dict of _dev_recode and out_sym_off[n + 1].  Asserts that nothing changed outside out_off[n] payload
    bytes, the n + 1 offsets, the n lengths and counts and the index slices, laid out by out_sym_off, of the streams that
    passed and did not become empty.  table = (span_tag, reps): fn is a _splice_table call, `rep` is unused, and the
    workspace is mh_dev_recode_splice_table_workspace's (n_reps: what it is sized for, else the table's; ws_fn: another sizing
    call with the same parameters)."""
    l = lib()
    n, pay_total, d_pl, d_po, d_nb, so, d_idx = _dev_source(payload, pay_off, nbits, sym_off, index)
    indexed = index is not None
    G, F = FIND_GUARD, FIND_FILL
    sof = np.ascontiguousarray(span_off, dtype=np.uint64)
    sp = np.zeros(0, dtype=np.uint64) if spans is None else np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
    r = _u8(rep)
    d_sof = DeviceBuffer(sof.nbytes, sof)
    d_sp = DeviceBuffer(max(sp.nbytes, 16), sp if sp.size else None)
    d_rep = DeviceBuffer(max(r.size, 16), np.concatenate([r, np.zeros(16, dtype=np.uint8)])[:max(r.size, 16)]) if r.size else None
    if table is not None:
        tg = np.ascontiguousarray(table[0], dtype=np.uint32)
        roff, rb = _rep_table(table[1])
        nreps = len(roff) - 1
        d_tg = DeviceBuffer(max(tg.nbytes, 16), tg if tg.size else None)
        d_roff = DeviceBuffer(roff.nbytes, roff)
        d_rb = DeviceBuffer(max(rb.size, 16), np.concatenate([rb, np.zeros(16, dtype=np.uint8)])[:max(rb.size, 16)]) if rb.size else None
        how = (d_tg.ptr, d_roff.ptr, d_rb.ptr if d_rb else None, nreps)
    else:
        how = (d_rep.ptr if d_rep else None, r.size)
    d_st = DeviceBuffer(max(n, 1) * 4, np.full(max(n, 1), 99, dtype=np.int32))
    st = int(so[n]) if indexed else 0
    ns = sp.size // 2 if n_spans is None else n_spans

    def call(room, with_payload, nidx):
        d_so = DeviceBuffer((n + 1 + G) * 8, np.concatenate([so if indexed else np.full(n + 1, F, dtype=np.uint64), np.full(G, F, dtype=np.uint64)]))
        if table is not None:
            wsb = (ws_fn or l.mh_dev_recode_splice_table_workspace)(n, st, chunk_symbols if indexed else 0, ns, nreps if n_reps is None else n_reps)
        else:
            wsb = l.mh_dev_recode_splice_workspace(n, st, chunk_symbols if indexed else 0, ns)
        d_ws = DeviceBuffer(wsb)
        d_out = DeviceBuffer(room + RANGE_GUARD + 16, np.full(room + RANGE_GUARD + 16, RANGE_FILL, dtype=np.uint8)) if with_payload else None
        d_oo = DeviceBuffer((n + 1 + G) * 8, np.full(n + 1 + G, F, dtype=np.uint64))
        d_oso = DeviceBuffer((n + 1 + G) * 8, np.full(n + 1 + G, F, dtype=np.uint64))
        d_onb = DeviceBuffer((n + G) * 8, np.full(n + G, F, dtype=np.uint64))
        d_dr = DeviceBuffer((n + G) * 8, np.full(n + G, F, dtype=np.uint64))
        d_oi = DeviceBuffer((nidx + G) * 8, np.full(nidx + G, F, dtype=np.uint64)) if nidx is not None else None
        _check(fn(src, dst, d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, prev0, d_so.ptr, st, d_idx.ptr if d_idx else None, chunk_symbols,
                  d_sof.ptr, d_sp.ptr, *how, d_out.ptr if d_out else None, room, d_oo.ptr, d_onb.ptr, d_oso.ptr,
                  d_oi.ptr if d_oi else None, nidx or 0, d_dr.ptr, d_st.ptr, d_ws.ptr, wsb, None), "mh_dev_recode_splice_*")
        rc = l.mh_dev_status(d_ws.ptr, None)
        oo, onb, dr, dso = d_oo.download(np.uint64), d_onb.download(np.uint64), d_dr.download(np.uint64), d_so.download(np.uint64)
        oso = d_oso.download(np.uint64)
        status = d_st.download(np.int32)[:n]
        assert (oo[n + 1:] == F).all() and (onb[n:] == F).all() and (dr[n:] == F).all() and (dso[n + 1:] == F).all() and (oso[n + 1:] == F).all(), \
            "words written behind an output"
        if indexed:
            assert np.array_equal(dso[:n + 1], so), "sym_off written with an index"
        res = dict(out_off=oo[:n + 1], nbits=onb[:n], dropped=dr[:n], status=status, sym_off=dso[:n + 1], out_sym_off=oso[:n + 1], rc=rc,
                   payload=None, index=None)
        if d_out:
            out = d_out.download(np.uint8)
            used = min(int(oo[n]), room) if rc != MH_ERR_CAPACITY else 0
            assert (out[used:] == RANGE_FILL).all(), "bytes written at or beyond min(cap, out_off[n])"
            res["payload"] = out[:used].copy()
        if d_oi:
            oi = d_oi.download(np.uint64)
            mine = np.zeros(nidx + G, dtype=bool)
            if rc != MH_ERR_CAPACITY and oso[n] != F:
                for i in range(n):
                    if status[i] == MH_OK:
                        b = int(oso[i]) // chunk_symbols + i
                        mine[b:b + (int(oso[i + 1] - oso[i]) + chunk_symbols - 1) // chunk_symbols] = True
            assert (oi[~mine] == F).all(), "index entries written outside the slices of the streams that passed"
            res["index"] = oi[:nidx]
        return res

    with_index = want_index and bool(chunk_symbols)
    if count_only:
        return call(0, False, index_cap if with_index else None)
    if cap is None or (with_index and index_cap is None):
        pre = call(0, False, None)
        if cap is None:
            cap = int(pre["out_off"][n])
        if index_cap is None and with_index:
            index_cap = int(pre["out_sym_off"][n]) // chunk_symbols + n
    return call(cap, True, index_cap if with_index else None)


def spans_from_hits(hit_off, hits, hit_cap=None):
    """mh_spans_from_hits (host, no device): the records of a find call, (hit_off[n + 1], hits[k, 3]), merged into maximal
    spans: (span_off[n + 1], spans[m, 2], return code).  hit_cap None: the number of records given."""
    hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
    n = len(hit_off) - 1
    cap = hits.size // 3 if hit_cap is None else hit_cap
    so, sp = np.full(n + 1, FIND_FILL, dtype=np.uint64), np.zeros(2 * max(cap, 1), dtype=np.uint64)
    rc = lib().mh_spans_from_hits(hit_off.ctypes.data, _ptr(hits), cap, n, so.ctypes.data, sp.ctypes.data)
    if rc not in (MH_OK, MH_ERR_CAPACITY):
        raise MhError(rc, "mh_spans_from_hits")
    return so, sp[:2 * int(so[n])].reshape(-1, 2), rc


def dev_spans_from_hits(hit_off, hits, hit_cap=None):
    """One mh_dev_spans_from_hits call on uploaded records: (span_off[n + 1], spans[m, 2], mh_dev_status); asserts that the
    FIND_GUARD words behind both outputs, and every pair at or beyond the spans, kept their fill."""
    l = lib()
    hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
    n = len(hit_off) - 1
    cap = hits.size // 3 if hit_cap is None else hit_cap
    d_ho = DeviceBuffer(hit_off.nbytes, hit_off)
    d_h = DeviceBuffer(max(hits.nbytes, 8), hits if hits.size else None)
    d_so = DeviceBuffer((n + 1 + FIND_GUARD) * 8, np.full(n + 1 + FIND_GUARD, FIND_FILL, dtype=np.uint64))
    d_sp = DeviceBuffer((2 * cap + FIND_GUARD) * 8, np.full(2 * cap + FIND_GUARD, FIND_FILL, dtype=np.uint64))
    wsb = l.mh_dev_spans_from_hits_workspace(n, cap)
    d_ws = DeviceBuffer(wsb, np.full(wsb, 0xA5, dtype=np.uint8))
    _check(l.mh_dev_spans_from_hits(d_ho.ptr, d_h.ptr, cap, n, d_so.ptr, d_sp.ptr, d_ws.ptr, wsb, None), "mh_dev_spans_from_hits")
    rc = l.mh_dev_status(d_ws.ptr, None)
    so, sp = d_so.download(np.uint64), d_sp.download(np.uint64)
    assert (so[n + 1:] == FIND_FILL).all(), "words written behind span_off"
    m = int(so[n])
    assert m <= cap and (sp[2 * m:] == FIND_FILL).all(), "pairs written at or beyond the spans"
    return so[:n + 1], sp[:2 * m].reshape(-1, 2), rc


class Selected:
    """What a select call wrote: payload and index are the whole buffers (guard bytes and gap entries included), status the
    return code (host form) or mh_dev_status (device form)."""


def _select_sources(batches, upload):
    """(coded_batches array, the arrays or device buffers it points into) of (payload, pay_off, nbits, sym_off, index, chunk)
    tuples of numpy arrays; payload (a batch that is only counted), sym_off and index may be None."""
    rows, keep = [], []
    for payload, pay_off, nbits, sym_off, index, chunk in batches:
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        n = len(pay_off) - 1
        parts = [None if payload is None else _u8(payload), pay_off, np.ascontiguousarray(nbits, dtype=np.uint64),
                 None if sym_off is None else np.ascontiguousarray(sym_off, dtype=np.uint64),
                 None if index is None else np.ascontiguousarray(index, dtype=np.uint64)]
        held = [None if a is None else upload(a) for a in parts]
        keep.append(held)
        at = [None if h is None else (h.ptr if isinstance(h, DeviceBuffer) else (h.ctypes.data if h.size else None)) for h in held]
        rows.append((at[0], at[1], at[2], n, int(pay_off[n]), at[3], int(parts[3][n]) if parts[3] is not None else 0, at[4], chunk))
    return coded_batches(rows), keep


def _select_sizes(batches, picks, chunk_symbols, cap, index_cap):
    """Output sizes large enough for any pick list: every pick at most the longest source stream."""
    n = len(picks)
    most = max([int(np.diff(np.asarray(b[1], dtype=np.uint64).astype(np.int64)).max(initial=0)) for b in batches] + [0])
    syms = max([int(np.diff(np.asarray(b[3], dtype=np.uint64).astype(np.int64)).max(initial=0)) for b in batches if b[3] is not None] + [0])
    cap = n * most if cap is None else cap
    if index_cap is None:
        index_cap = n * syms // chunk_symbols + n + 1 if chunk_symbols else 0
    return cap, index_cap


def select_batch(batches, picks, chunk_symbols=0, cap=None, index_cap=None, want_sym=True, want_index=True, fill=0xA5):
    """mh_select_batch (host, no device) on (payload, pay_off, nbits, sym_off, index, chunk) tuples of numpy arrays: a Selected.
    Buffers are prefilled with `fill`; cap / index_cap None: room for any pick list."""
    picks = np.ascontiguousarray(picks, dtype=np.uint64)
    n = picks.size
    src, keep = _select_sources(batches, lambda a: a)
    cap, index_cap = _select_sizes(batches, picks, chunk_symbols, cap, index_cap)
    r = Selected()
    word = int.from_bytes(bytes([fill]) * 8, "little")
    r.payload = np.full(cap + 64, fill, dtype=np.uint8)
    r.out_off, r.nbits = np.full(n + 1, word, dtype=np.uint64), np.full(n, word, dtype=np.uint64)
    r.sym_off = np.full(n + 1, word, dtype=np.uint64) if want_sym else None
    r.index = np.full(index_cap + 8, word, dtype=np.uint64) if want_index and chunk_symbols else None
    r.pick_status = np.full(n, -99, dtype=np.int32)
    at = lambda a: None if a is None else a.ctypes.data
    r.status = lib().mh_select_batch(src, len(batches), _ptr(picks), n, at(r.payload), cap, at(r.out_off), _ptr(r.nbits), at(r.sym_off),
                                     at(r.index), index_cap, chunk_symbols, _ptr(r.pick_status))
    r.cap, r.index_cap = cap, index_cap
    return r


def dev_select_batch(batches, picks, chunk_symbols=0, cap=None, index_cap=None, want_sym=True, want_index=True, count_only=False, fill=0xA5):
    """One mh_dev_select_batch call on uploaded batches, every output and the workspace prefilled with `fill`: a Selected."""
    l = lib()
    picks = np.ascontiguousarray(picks, dtype=np.uint64)
    n = picks.size
    src, keep = _select_sources(batches, lambda a: DeviceBuffer(max(a.nbytes, 16), a if a.size else None))
    cap, index_cap = _select_sizes(batches, picks, chunk_symbols, cap, index_cap)
    filled = lambda nbytes: DeviceBuffer(max(nbytes, 16), np.full(max(nbytes, 16), fill, dtype=np.uint8))
    d_picks = DeviceBuffer(max(picks.nbytes, 16), picks if n else None)
    d_out = None if count_only else filled(cap + 64)
    d_oo, d_nb, d_st = filled((n + 1) * 8), filled(n * 8), filled(n * 4)
    d_so = filled((n + 1) * 8) if want_sym else None
    d_idx = filled((index_cap + 8) * 8) if want_index and chunk_symbols else None
    wsb = l.mh_dev_select_batch_workspace(sum(len(b[1]) - 1 for b in batches), n)
    d_ws = filled(wsb)
    p = lambda d: None if d is None else d.ptr
    blk = select_args(src, len(batches), d_picks.ptr, n, p(d_out), cap, d_oo.ptr, d_nb.ptr, p(d_so), p(d_idx), index_cap, chunk_symbols, d_st.ptr,
                      d_ws.ptr, wsb, None)
    _check(l.mh_dev_select_batch(C.byref(blk)), "mh_dev_select_batch")
    r = Selected()
    r.status = l.mh_dev_status(d_ws.ptr, None)
    r.payload = None if d_out is None else d_out.download()[:cap + 64]
    r.out_off, r.nbits, r.pick_status = d_oo.download(np.uint64)[:n + 1], d_nb.download(np.uint64)[:n], d_st.download(np.int32)[:n]
    r.sym_off = None if d_so is None else d_so.download(np.uint64)[:n + 1]
    r.index = None if d_idx is None else d_idx.download(np.uint64)[:index_cap + 8]
    r.cap, r.index_cap = cap, index_cap
    return r


def picks_from_hits(hit_off, stream_status, n_streams, source=0, flags=0):
    """mh_picks_from_hits (host, no device): (picks[n_streams], n_kept)."""
    ho = None if hit_off is None else np.ascontiguousarray(hit_off, dtype=np.uint64)
    st = None if stream_status is None else np.ascontiguousarray(stream_status, dtype=np.int32)
    picks, kept = np.full(n_streams, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    _check(lib().mh_picks_from_hits(None if ho is None else ho.ctypes.data, None if st is None or not st.size else st.ctypes.data, n_streams, source,
                                    flags, _ptr(picks), kept.ctypes.data), "mh_picks_from_hits")
    return picks, int(kept[0])


def dev_picks_from_hits(hit_off, stream_status, n_streams, source=0, flags=0):
    """One mh_dev_picks_from_hits call on uploaded arrays, outputs and workspace prefilled with 0xA5: (picks[n_streams], n_kept)."""
    l = lib()
    up = lambda a, t: None if a is None else DeviceBuffer(max(np.asarray(a).size * np.dtype(t).itemsize, 16), np.ascontiguousarray(a, dtype=t))
    d_ho, d_st = up(hit_off, np.uint64), up(stream_status, np.int32)
    filled = lambda nbytes: DeviceBuffer(max(nbytes, 16), np.full(max(nbytes, 16), 0xA5, dtype=np.uint8))
    wsb = l.mh_dev_picks_from_hits_workspace(n_streams)
    d_picks, d_kept, d_ws = filled(n_streams * 8), filled(8), filled(wsb)
    p = lambda d: None if d is None else d.ptr
    blk = picks_args(p(d_ho), p(d_st), n_streams, source, flags, d_picks.ptr, d_kept.ptr, d_ws.ptr, wsb, None)
    _check(l.mh_dev_picks_from_hits(C.byref(blk)), "mh_dev_picks_from_hits")
    _check(l.mh_dev_status(d_ws.ptr, None), "mh_dev_picks_from_hits status")
    return d_picks.download(np.uint64)[:n_streams], int(d_kept.download(np.uint64)[0])


def spans_from_hits_tagged(hit_off, hits, hit_pattern, hit_cap=None):
    """mh_spans_from_hits_tagged (host, no device): spans_from_hits and span_tag[m], the lowest pattern number among the
    records merged into each span: (span_off, spans, span_tag, return code)."""
    hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
    pat = np.ascontiguousarray(hit_pattern, dtype=np.uint32)
    n = len(hit_off) - 1
    cap = hits.size // 3 if hit_cap is None else hit_cap
    so, sp = np.full(n + 1, FIND_FILL, dtype=np.uint64), np.zeros(2 * max(cap, 1), dtype=np.uint64)
    tg = np.full(max(cap, 1), 0xFFFFFFFF, dtype=np.uint32)
    rc = lib().mh_spans_from_hits_tagged(hit_off.ctypes.data, _ptr(hits), pat.ctypes.data, cap, n, so.ctypes.data, sp.ctypes.data, tg.ctypes.data)
    if rc not in (MH_OK, MH_ERR_CAPACITY):
        raise MhError(rc, "mh_spans_from_hits_tagged")
    m = int(so[n])
    return so, sp[:2 * m].reshape(-1, 2), tg[:m], rc


def dev_spans_from_hits_tagged(hit_off, hits, hit_pattern, hit_cap=None):
    """One mh_dev_spans_from_hits_tagged call on uploaded records: (span_off[n + 1], spans[m, 2], span_tag[m], mh_dev_status);
    asserts that the FIND_GUARD words behind the three outputs, and every pair and tag at or beyond the spans, kept their
    fill."""
    l = lib()
    hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
    hits = np.ascontiguousarray(hits, dtype=np.uint64).reshape(-1)
    pat = np.ascontiguousarray(hit_pattern, dtype=np.uint32)
    n = len(hit_off) - 1
    cap = hits.size // 3 if hit_cap is None else hit_cap
    fill32 = FIND_FILL & 0xFFFFFFFF
    d_ho = DeviceBuffer(hit_off.nbytes, hit_off)
    d_h = DeviceBuffer(max(hits.nbytes, 8), hits if hits.size else None)
    d_pat = DeviceBuffer(max(pat.nbytes, 8), pat if pat.size else None)
    d_so = DeviceBuffer((n + 1 + FIND_GUARD) * 8, np.full(n + 1 + FIND_GUARD, FIND_FILL, dtype=np.uint64))
    d_sp = DeviceBuffer((2 * cap + FIND_GUARD) * 8, np.full(2 * cap + FIND_GUARD, FIND_FILL, dtype=np.uint64))
    d_tg = DeviceBuffer((cap + FIND_GUARD) * 4, np.full(cap + FIND_GUARD, fill32, dtype=np.uint32))
    wsb = l.mh_dev_spans_from_hits_tagged_workspace(n, cap)
    d_ws = DeviceBuffer(wsb, np.full(wsb, 0xA5, dtype=np.uint8))
    _check(l.mh_dev_spans_from_hits_tagged(d_ho.ptr, d_h.ptr, d_pat.ptr, cap, n, d_so.ptr, d_sp.ptr, d_tg.ptr, d_ws.ptr, wsb, None),
           "mh_dev_spans_from_hits_tagged")
    rc = l.mh_dev_status(d_ws.ptr, None)
    so, sp, tg = d_so.download(np.uint64), d_sp.download(np.uint64), d_tg.download(np.uint32)
    assert (so[n + 1:] == FIND_FILL).all(), "words written behind span_off"
    m = int(so[n])
    assert m <= cap and (sp[2 * m:] == FIND_FILL).all(), "pairs written at or beyond the spans"
    assert (tg[m:] == fill32).all(), "tags written at or beyond the spans"
    return so[:n + 1], sp[:2 * m].reshape(-1, 2), tg[:m], rc


def histogram_coded_batch_o2(src, order, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
    """The training counts of an order-`order` model from a batch coded under `src`, no decoded byte written
    (mh_dev_histogram_coded_batch_o2; `src` or `order` is 2): counts[256, 65536 or 1 << 24].  Raises when a stream fails."""
    counts, status, rc = src.dev_histogram_coded_o2(order, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols)
    _check(rc, "mh_dev_histogram_coded_batch_o2")
    return counts


# ---- tokens from matched bytes (include/mh.h, "TOKENS FROM MATCHED BYTES") -------------------------------------------------
def span_token_digest(key, data, flags=0):
    """mh_span_token_digest (host, no device): the keyed 64-bit digest of a byte string."""
    k, d = _u8(bytes(key)), _u8(data)
    if k.size != 16:
        raise ValueError("a token key has 16 bytes")
    return int(lib().mh_span_token_digest(k.ctypes.data, _ptr(d), d.size, flags))


def token_formats(formats):
    """(fmt_off[2 n + 1], fmt_bytes, hex_digits[n]) of a list of (prefix, hex_digits, suffix)."""
    off, blob = [0], b""
    for prefix, _, suffix in formats:
        blob += bytes(prefix)
        off.append(len(blob))
        blob += bytes(suffix)
        off.append(len(blob))
    return np.asarray(off, dtype=np.uint64), _u8(blob), np.asarray([h for _, h, _ in formats], dtype=np.uint8)


def dev_span_tokens(src, payload, pay_off, nbits, span_off, spans, span_tag, formats, key, flags=0, prev0=PREV0, sym_off=None, index=None,
                    chunk_symbols=0, n_reps=None, rep_cap=None, count_only=False, ws_n_reps=None, fmt_arrays=None):
    """One mh_dev_span_tokens_batch call on an uploaded batch under src (a Model or a ModelSet), with FIND_GUARD words of
    FIND_FILL behind rep_off, rep_tag and the statuses, RANGE_GUARD bytes behind rep_bytes and the workspace filled with 0xFF
    beforehand.  n_reps None: the number of spans; rep_cap None: a count-only call first, then one with exactly rep_off[n_reps]
    bytes.  ws_n_reps: what the workspace is sized for.  fmt_arrays: (fmt_off, fmt_bytes, hex_digits) as they are, instead of
    `formats`.  Returns dict(rep_off, rep_bytes or None, rep_tag, status, rc = mh_dev_status); a call the library refuses
    before any launch raises MhError.  Asserts that nothing changed behind the outputs or at or beyond rep_off[n_reps] bytes."""
    l = lib()
    n, pay_total, d_pl, d_po, d_nb, so, d_idx = _dev_source(payload, pay_off, nbits, sym_off, index)
    indexed = index is not None
    G, F = FIND_GUARD, FIND_FILL
    sof = np.ascontiguousarray(span_off, dtype=np.uint64)
    sp = np.zeros(0, dtype=np.uint64) if spans is None else np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
    nr = sp.size // 2 if n_reps is None else n_reps
    foff, fb, hexd = fmt_arrays if fmt_arrays is not None else token_formats(formats)
    foff, fb, hexd = np.ascontiguousarray(foff, dtype=np.uint64), _u8(fb), np.ascontiguousarray(hexd, dtype=np.uint8)
    d_sof = DeviceBuffer(sof.nbytes, sof)
    d_sp = DeviceBuffer(max(sp.nbytes, 16), sp if sp.size else None)
    d_tg = None
    if span_tag is not None:
        tg = np.ascontiguousarray(span_tag, dtype=np.uint32)
        d_tg = DeviceBuffer(max(tg.nbytes, 16), tg if tg.size else None)
    d_foff = DeviceBuffer(foff.nbytes, foff)
    d_fb = DeviceBuffer(max(fb.size, 16), np.concatenate([fb, np.zeros(16, dtype=np.uint8)])[:max(fb.size, 16)])
    d_hex = DeviceBuffer(max(hexd.size, 16), np.concatenate([hexd, np.zeros(16, dtype=np.uint8)])[:max(hexd.size, 16)])
    d_so = DeviceBuffer(so.nbytes, so) if indexed else None
    is_set = isinstance(src, ModelSet)

    def call(room, with_bytes):
        wsb = l.mh_dev_span_tokens_workspace(n, nr if ws_n_reps is None else ws_n_reps)
        d_ws = DeviceBuffer(wsb, np.full(wsb, 0xFF, dtype=np.uint8))
        d_roff = DeviceBuffer((nr + 1 + G) * 8, np.full(nr + 1 + G, F, dtype=np.uint64))
        d_rtag = DeviceBuffer((nr + 2 * G) * 4, np.full(nr + 2 * G, F & 0xFFFFFFFF, dtype=np.uint32))
        d_st = DeviceBuffer((n + 2 * G) * 4, np.full(n + 2 * G, 99, dtype=np.int32))
        d_rb = DeviceBuffer(room + RANGE_GUARD + 16, np.full(room + RANGE_GUARD + 16, RANGE_FILL, dtype=np.uint8)) if with_bytes else None
        blk = span_tokens_args(None if is_set else src.handle, src.handle if is_set else None,
                               (d_pl.ptr, d_po.ptr, d_nb.ptr, n, pay_total, d_so.ptr if d_so else None, int(so[n]) if indexed else 0,
                                d_idx.ptr if d_idx else None, chunk_symbols if indexed else 0, prev0),
                               d_sof.ptr, d_sp.ptr, d_tg.ptr if d_tg else None, key, flags, d_foff.ptr, d_fb.ptr, d_hex.ptr, len(hexd), nr,
                               d_roff.ptr, d_rb.ptr if d_rb else None, room, d_rtag.ptr, d_st.ptr)
        launch = launch_args(d_ws.ptr, wsb, None)
        _check(l.mh_dev_span_tokens_batch(C.byref(blk), C.byref(launch)), "mh_dev_span_tokens_batch")
        rc = l.mh_dev_status(d_ws.ptr, None)
        roff, rtag, st = d_roff.download(np.uint64), d_rtag.download(np.uint32), d_st.download(np.int32)
        assert (roff[nr + 1:] == F).all() and (rtag[nr:] == F & 0xFFFFFFFF).all() and (st[n:] == 99).all(), "words written behind an output"
        res = dict(rep_off=roff[:nr + 1], rep_tag=rtag[:nr], status=st[:n], rc=rc, rep_bytes=None)
        if d_rb:
            out = d_rb.download(np.uint8)
            used = min(int(roff[nr]), room) if rc == MH_OK or roff[nr] <= room else 0
            if roff[nr] == F:
                used = 0                                                # (the call stopped before the offsets were written)
            assert (out[used:] == RANGE_FILL).all(), "bytes written at or beyond rep_off[n_reps]"
            res["rep_bytes"] = out[:used].copy()
        if indexed:
            assert np.array_equal(d_so.download(np.uint64), so), "sym_off written"
        return res

    if count_only:
        return call(0, False)
    if rep_cap is None:
        rep_cap = int(call(0, False)["rep_off"][nr])
    return call(rep_cap, True)


def span_tokens_batch(model, payload, pay_off, nbits, span_off, spans, span_tag, formats, key, flags=0, prev0=PREV0, sym_off=None, index=None,
                      chunk_symbols=0, rep_cap=None):
    """mh_span_tokens_batch, the host form: (rep_off, rep_bytes, rep_tag, status, return code)."""
    payload, pay_off, nbits = _u8(payload), np.ascontiguousarray(pay_off, dtype=np.uint64), np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    sof = np.ascontiguousarray(span_off, dtype=np.uint64)
    sp = np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
    nr = sp.size // 2
    tg = None if span_tag is None else np.ascontiguousarray(span_tag, dtype=np.uint32)
    foff, fb, hexd = token_formats(formats)
    k = _u8(bytes(key))
    so = None if sym_off is None else np.ascontiguousarray(sym_off, dtype=np.uint64)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint64)
    cap = SPLICE_MAX_REP * nr if rep_cap is None else rep_cap
    roff, rb, rtag, st = np.zeros(nr + 1, dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(nr, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.int32)
    rc = lib().mh_span_tokens_batch(model.handle, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data, n, prev0, so.ctypes.data if so is not None else None,
                                    idx.ctypes.data if idx is not None else None, chunk_symbols, sof.ctypes.data, _ptr(sp), _ptr(tg) if tg is not None else None,
                                    k.ctypes.data, flags, foff.ctypes.data, _ptr(fb), _ptr(hexd), len(hexd), roff.ctypes.data, rb.ctypes.data, cap,
                                    rtag.ctypes.data, st.ctypes.data)
    return roff, rb[:min(int(roff[nr]), cap)], rtag[:nr], st[:n], rc


class Model:
    """Owns an mh_model* (tables resident on the current device)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_counts(cls, counts, order, max_len=0):
        """max_len (8..64, order 0 / 1): no code longer than that, at the least cost in bits; 0 = no limit."""
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != {0: 256, 1: 65536, 2: 1 << 24}[order]:
            raise ValueError("counts size")
        h = C.c_void_p()
        if max_len:
            _check(lib().mh_model_from_counts_limited(c.ctypes.data, order, max_len, C.byref(h)), "mh_model_from_counts_limited")
        else:
            _check(lib().mh_model_from_counts(c.ctypes.data, order, C.byref(h)), "mh_model_from_counts")
        return cls(h)

    @classmethod
    def from_device_counts(cls, d_counts_ptr, order, stream=None, max_len=0):
        h = C.c_void_p()
        if max_len:
            _check(lib().mh_dev_model_from_counts_limited(d_counts_ptr, order, max_len, stream, C.byref(h)),
                   "mh_dev_model_from_counts_limited")
        else:
            _check(lib().mh_dev_model_from_counts(d_counts_ptr, order, stream, C.byref(h)), "mh_dev_model_from_counts")
        return cls(h)

    @classmethod
    def from_device_counts_ws(cls, d_counts_ptr, order, d_ws_ptr, ws_bytes, stream=None, max_len=0):
        """Model built into a caller workspace (no allocation inside, one stream sync); the caller keeps
        the workspace alive for as long as the model is used."""
        h = C.c_void_p()
        if max_len:
            _check(lib().mh_dev_model_from_counts_limited_ws(d_counts_ptr, order, max_len, d_ws_ptr, ws_bytes, stream, C.byref(h)),
                   "mh_dev_model_from_counts_limited_ws")
        else:
            _check(lib().mh_dev_model_from_counts_ws(d_counts_ptr, order, d_ws_ptr, ws_bytes, stream, C.byref(h)),
                   "mh_dev_model_from_counts_ws")
        return cls(h)

    @classmethod
    def from_data(cls, data, order=1):
        """Histogram on the GPU, then tree build (the `markovhuffman in -d table` path)."""
        return cls.from_counts({0: histogram_o0, 1: histogram_o1, 2: histogram_o2}[order](data), order)

    @classmethod
    def from_table(cls, table_bytes):
        a = _u8(table_bytes)
        h = C.c_void_p()
        _check(lib().mh_model_from_table_bits(_ptr(a), a.size, C.byref(h)), "mh_model_from_table_bits")
        return cls(h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mh_model_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    @property
    def type(self):
        return lib().mh_model_type(self._h)

    @property
    def max_code_len(self):
        return lib().mh_model_max_code_len(self._h)

    @property
    def min_code_len(self):
        return lib().mh_model_min_code_len(self._h)

    def payload_bits(self, counts):
        """Exact payload bits of data with this histogram (host counts: 65536 for a Markov model, 256 for a Huffman model)."""
        c = np.ascontiguousarray(counts, dtype=np.uint64)
        if c.size != (65536 if self.type else 256):
            raise ValueError("counts size")
        n = C.c_uint64(0)
        _check(lib().mh_model_payload_bits(self._h, c.ctypes.data, C.byref(n)), "mh_model_payload_bits")
        return n.value

    def decode_layout(self):
        """(primary_bits, secondary_entries, in_lds) of the device decode tables."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(lib().mh_model_decode_layout(self._h, C.byref(a), C.byref(b), C.byref(c)), "mh_model_decode_layout")
        return a.value, b.value, bool(c.value)

    def tile_layout(self):
        """(primary_bits, secondary_bits, secondary_entries) of the tile decoder's tables; primary_bits 0 = none."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        _check(lib().mh_model_tile_layout(self._h, C.byref(a), C.byref(b), C.byref(c)), "mh_model_tile_layout")
        return a.value, b.value, c.value

    def image(self, which):
        """Device image `which` (see mh.h: 0 enc16 ... 7 walk tree) as bytes."""
        n = C.c_size_t(0)
        _check(lib().mh_model_image(self._h, which, None, 0, C.byref(n)), "mh_model_image")
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mh_model_image(self._h, which, out.ctypes.data, n.value, C.byref(n)), "mh_model_image")
        return out[:n.value].tobytes()

    def table_bytes(self):
        n = C.c_size_t(0)
        _check(lib().mh_model_write_table(self._h, None, 0, C.byref(n)), "mh_model_write_table")
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        _check(lib().mh_model_write_table(self._h, out.ctypes.data, n.value, C.byref(n)), "mh_model_write_table")
        return out[:n.value].tobytes()

    def codes(self):
        """(len8[65536], code64[65536]) indexed prev*256+sym (get_encoding for every pair)."""
        lens = np.zeros(65536, dtype=np.uint8)
        codes = np.zeros(65536, dtype=np.uint64)
        l, c = C.c_int(), C.c_uint64()
        for p in range(256):
            for s in range(256):
                lib().mh_model_get_code(self._h, p, s, C.byref(l), C.byref(c))
                lens[p * 256 + s] = l.value
                codes[p * 256 + s] = c.value
        return lens, codes

    def codes_o2(self):
        """Order-2 model: (len8[1 << 24], code64[1 << 24]) indexed ctx*256+sym, straight from the device tables."""
        return (np.frombuffer(self.image(1), dtype=np.uint8), np.frombuffer(self.image(3), dtype=np.uint64))

    def lut(self, prev, w):
        p, i, v, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib().mh_model_get_lut(self._h, prev, w, C.byref(p), C.byref(i), C.byref(v), C.byref(d))
        return bool(p.value), bool(i.value), v.value, d.value

    # ---- host-buffer codec calls -------------------------------------------------------------
    def encode(self, data, prev0=PREV0, chunk_symbols=None):
        """Returns (payload bytes, nbits, index or None)."""
        a = _u8(data)
        cap = lib().mh_encode_bound(self._h, a.size)
        out = np.zeros(cap, dtype=np.uint8)
        nbits = C.c_uint64(0)
        idx = None
        if chunk_symbols:
            idx = np.zeros(max((a.size + chunk_symbols - 1) // chunk_symbols, 1), dtype=np.uint64)
        _check(lib().mh_encode(self._h, _ptr(a), a.size, prev0, out.ctypes.data, cap, C.byref(nbits),
                               idx.ctypes.data if idx is not None else None, chunk_symbols or 0), "mh_encode")
        nb = (nbits.value + 7) // 8
        if idx is not None:
            idx = idx[:(a.size + chunk_symbols - 1) // chunk_symbols]
        return out[:nb].tobytes(), nbits.value, idx

    def compress(self, data, chunk_symbols=None):
        """Whole compressed file (header byte + payload), as i_coding_provider::compress writes it."""
        payload, nbits, idx = self.encode(data, PREV0, chunk_symbols)
        return bytes([lib().mh_stream_header(self._h, nbits)]) + payload, nbits, idx

    def decode(self, payload, nbits, prev0=PREV0, index=None, chunk_symbols=0, n_symbols=0, cap=None):
        a = _u8(payload)
        if cap is None:
            cap = n_symbols if index is not None else nbits
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        n = C.c_size_t(0)
        ip = None
        if index is not None:
            index = np.ascontiguousarray(index, dtype=np.uint64)
            ip = index.ctypes.data if index.size else None
            if ip is None and n_symbols == 0:
                ip = out.ctypes.data  # any non-null pointer: zero entries are read
        _check(lib().mh_decode(self._h, _ptr(a), nbits, prev0, out.ctypes.data, cap, C.byref(n), ip,
                               chunk_symbols, n_symbols), "mh_decode")
        return out[:n.value].tobytes()

    def decompress(self, blob, index=None, chunk_symbols=0, n_symbols=0):
        """Whole compressed file in, original bytes out (i_coding_provider::decompress)."""
        a = _u8(blob)
        nbits = C.c_uint64(0)
        if a.size < 1:
            raise MhError(MH_ERR_CORRUPT, "decompress")
        _check(lib().mh_stream_parse_header(self._h, int(a[0]), a.size, C.byref(nbits)), "mh_stream_parse_header")
        return self.decode(a[1:], nbits.value, PREV0, index, chunk_symbols, n_symbols)

    # ---- random access (mh_decode_ranges) -----------------------------------------------------------------------------
    def decode_ranges(self, payload, nbits, index, chunk_symbols, n_symbols, ranges):
        """Bytes [begin, end) of the original input for every (begin, end) in `ranges`, from an indexed stream (payload without
        the header byte, its chunk index).  Returns (list of byte strings, int32 status per range); a failed range's bytes are
        empty.  Raises MhError on a call-level error (bad arguments, no device)."""
        return self._decode_ranges(payload, nbits, index, chunk_symbols, n_symbols, ranges, "mh_decode_ranges")

    def decode_ranges_o2(self, payload, nbits, index, chunk_symbols, n_symbols, ranges):
        """decode_ranges for an order-2 model (mh_decode_ranges_o2; index entries carry two context bytes).  Any other model is
        refused with MhError(MH_ERR_ARG)."""
        self._require_o2("mh_decode_ranges_o2")
        return self._decode_ranges(payload, nbits, index, chunk_symbols, n_symbols, ranges, "mh_decode_ranges_o2")

    def _decode_ranges(self, payload, nbits, index, chunk_symbols, n_symbols, ranges, fn):
        a = _u8(payload)
        rg = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 2))
        n = rg.shape[0]
        idx = np.ascontiguousarray(index if index is not None else np.zeros(0), dtype=np.uint64)
        ok = (rg[:, 0] <= rg[:, 1]) & (rg[:, 1] <= np.uint64(n_symbols))
        cap = int(np.sum(np.where(ok, rg[:, 1] - rg[:, 0], 0), dtype=np.uint64)) if n else 0
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(max(n, 1), dtype=np.int32)
        ip = idx.ctypes.data if idx.size else (out.ctypes.data if n_symbols == 0 else None)
        rc = getattr(lib(), fn)(self._h, _ptr(a), nbits, ip, chunk_symbols, n_symbols, rg.ctypes.data if n else None, n,
                                out.ctypes.data, cap, out_off.ctypes.data, status.ctypes.data)
        status = status[:n]
        if rc != MH_OK and not np.any(status == rc):
            raise MhError(rc, fn)
        res = [out[int(out_off[j]):int(out_off[j + 1])].tobytes() if status[j] == MH_OK else b"" for j in range(n)]
        return res, status


    # ---- lookups into batches (mh_decode_batch_ranges / mh_dev_decode_batch_ranges) ------------------------------------
    def decode_batch_ranges(self, payload, pay_off, nbits, lookups, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
        """Bytes [begin, end) of stream `stream` for every (stream, begin, end) in `lookups`, from a batch (packed payloads,
        pay_off[n + 1], nbits[n]; with an index, sym_off is the encode's in_off).  Returns (list of byte strings, int32 status
        per lookup); a failed lookup's bytes are empty.  Raises MhError on a call-level error (mh_decode_batch_ranges)."""
        return self._decode_batch_ranges(payload, pay_off, nbits, lookups, prev0, sym_off, index, chunk_symbols, "mh_decode_batch_ranges")

    def _decode_batch_ranges(self, payload, pay_off, nbits, lookups, prev0, sym_off, index, chunk_symbols, fn):
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        so = np.ascontiguousarray(sym_off, dtype=np.uint64) if sym_off is not None else None
        idx = np.ascontiguousarray(index, dtype=np.uint64) if index is not None else None
        lk = _lookups(lookups)
        m = lk.shape[0]
        call = lambda out, cap, oo, st: getattr(lib(), fn)(
            self._h, _ptr(payload), payload.size, pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0,
            so.ctypes.data if so is not None else None,
            (idx.ctypes.data if idx.size else pay_off.ctypes.data) if idx is not None else None, chunk_symbols,
            lk.ctypes.data if m else None, m, out, cap, oo, st)
        return _host_batch_ranges(call, fn, lk, nbits[:n], so)

    def dev_decode_batch_ranges(self, payload, pay_off, nbits, lookups, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, out_cap=None):
        """One mh_dev_decode_batch_ranges call with guard bytes around every output: (list of bytes, status per lookup,
        mh_dev_status)."""
        return _dev_batch_ranges(lib().mh_dev_decode_batch_ranges, self._h, payload, pay_off, nbits, lookups, prev0, sym_off, index,
                                 chunk_symbols, out_cap)

    def find_batch(self, ps, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, check=True):
        """mh_find_batch (host form): the arguments and results of _find_batch."""
        return self._find_batch(lib().mh_find_batch, "mh_find_batch", ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols,
                                hit_cap, check)

    def _find_batch(self, fn, what, ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap, check):
        """mh_find_batch / mh_find_batch_o2 (host form): (hit_off[n + 1], hits[k, 3] = (stream, begin, end), hit_pattern[k], per-stream status[n],
        return code).  hit_cap None: a count-only call first, then one with room for every hit; hit_cap 'count': count only.
        check=False returns a failed stream's status or MH_ERR_CAPACITY instead of raising."""
        l = lib()
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        so = np.ascontiguousarray(sym_off, dtype=np.uint64) if sym_off is not None else None
        idx = np.ascontiguousarray(index, dtype=np.uint64) if index is not None else None
        ho = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)

        def call(hits, pat, cap):
            rc = fn(self._h, ps.handle, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0,
                    so.ctypes.data if so is not None else None,
                    (idx.ctypes.data if idx.size else pay_off.ctypes.data) if idx is not None else None, chunk_symbols,
                    ho.ctypes.data, hits.ctypes.data if hits is not None else None, pat.ctypes.data if pat is not None else None,
                    cap, st.ctypes.data)
            if rc != MH_OK and (check or not (st[:n].any() or rc == MH_ERR_CAPACITY)):
                raise MhError(rc, what)
            return rc

        if hit_cap is None or hit_cap == "count":
            rc = call(None, None, 0)
            if hit_cap == "count":
                return ho, np.zeros((0, 3), dtype=np.uint64), np.zeros(0, dtype=np.uint32), st[:n], rc
        cap = int(ho[n]) if hit_cap is None else hit_cap
        hits, pat = np.zeros(max(cap, 1) * 3, dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32)
        rc = call(hits, pat, cap)
        k = min(int(ho[n]), cap)
        return ho, hits[:3 * k].reshape(-1, 3), pat[:k], st[:n], rc

    def dev_find_batch(self, ps, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, count_only=False):
        """One mh_dev_find_batch call (two when hit_cap is None: count, then records) with guard words behind its outputs:
        (hit_off[n + 1], hits[k, 3], hit_pattern[k], per-stream status[n], mh_dev_status)."""
        return _dev_find(lib().mh_dev_find_batch, self._h, ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap, count_only)

    def find_dict_batch(self, d, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, check=True):
        """mh_find_dict_batch (host form): find_batch's arguments and results with a Dict for the pattern set."""
        return self._find_batch(lib().mh_find_dict_batch, "mh_find_dict_batch", d, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols,
                                hit_cap, check)

    def dev_find_dict_batch(self, d, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None,
                            count_only=False):
        """One mh_dev_find_dict_batch call (two when hit_cap is None) with guard words behind its outputs: dev_find_batch's results."""
        return _dev_find(lib().mh_dev_find_dict_batch, self._h, d, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap,
                         count_only, ws_fn=lib().mh_dev_find_dict_workspace)

    def crc_batch(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, check=True):
        """mh_crc_batch (host form): (crc[n], len[n], per-stream status[n], return code)."""
        return _host_crc(lib().mh_crc_batch, "mh_crc_batch", self._h, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, check)

    def dev_crc_batch(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_crc_batch call with guard words behind its outputs: (crc[n], len[n], per-stream status[n], mh_dev_status)."""
        return _dev_crc(lib().mh_dev_crc_batch, self._h, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, **kw)

    def dev_histogram_coded(self, order, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
        """One mh_dev_histogram_coded_batch call on a batch coded under this model: (counts, per-stream status[n], mh_dev_status)."""
        return _dev_histogram_coded(lib().mh_dev_histogram_coded_batch, self._h, order, payload, pay_off, nbits, prev0, sym_off, index,
                                    chunk_symbols)

    def dev_recode_batch(self, dst, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_batch call (a batch coded under this model, coded again under `dst`) with guards around its outputs:
        the dict of _dev_recode."""
        return _dev_recode(lib().mh_dev_recode_batch, self._h, dst.handle, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, **kw)

    def dev_recode_edit_batch(self, dst, payload, pay_off, nbits, byte_map, span_off=None, spans=None, prev0=PREV0, sym_off=None, index=None,
                              chunk_symbols=0, **kw):
        """One mh_dev_recode_edit_batch call: dev_recode_batch with map[b] coded for every byte b inside the spans (span_off None:
        everywhere).  The dict of _dev_recode, with its guards."""
        return _dev_recode_edit(lib().mh_dev_recode_edit_batch, self._h, dst.handle, payload, pay_off, nbits, byte_map, span_off, spans, prev0,
                                sym_off, index, chunk_symbols, **kw)

    def dev_recode_splice_batch(self, dst, payload, pay_off, nbits, rep, span_off, spans, prev0=PREV0, sym_off=None, index=None,
                                chunk_symbols=0, **kw):
        """One mh_dev_recode_splice_batch call: dev_recode_batch with every span replaced by `rep` (b"": deleted).  The dict of
        _dev_recode_splice (out_sym_off and the index laid out by it included), with its guards."""
        return _dev_recode_splice(lib().mh_dev_recode_splice_batch, self._h, dst.handle, payload, pay_off, nbits, rep, span_off, spans, prev0,
                                  sym_off, index, chunk_symbols, **kw)

    def dev_recode_splice_table_batch(self, dst, payload, pay_off, nbits, span_tag, reps, span_off, spans, prev0=PREV0, sym_off=None,
                                      index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_splice_table_batch call: span r replaced by reps[span_tag[r]] (b"": deleted; begin == end: an
        insertion).  reps: a list of byte strings, or (rep_off, rep_bytes).  The dict of _dev_recode_splice, with its guards."""
        return _dev_recode_splice(lib().mh_dev_recode_splice_table_batch, self._h, dst.handle, payload, pay_off, nbits, b"", span_off, spans, prev0,
                                  sym_off, index, chunk_symbols, table=(span_tag, reps), **kw)

    def recode_splice_table_batch(self, dst, payload, pay_off, nbits, span_tag, reps, span_off, spans, **kw):
        """mh_recode_splice_table_batch (host form): recode_splice_batch with a replacement per span; the same dict."""
        return self.recode_splice_batch(dst, payload, pay_off, nbits, b"", span_off, spans, table=(span_tag, reps), **kw)

    # ---- order 2 in editing and splicing (include/mh.h, "ORDER 2 IN EDITING AND SPLICING") -----------------------------------
    def dev_recode_edit_batch_o2(self, dst, payload, pay_off, nbits, byte_map, span_off=None, spans=None, prev0=PREV0, sym_off=None, index=None,
                                 chunk_symbols=0, **kw):
        """One mh_dev_recode_edit_batch_o2 call (this model or `dst` is order 2): dev_recode_edit_batch's arguments, dict and guards."""
        l = lib()

        def call(*a):
            return l.mh_dev_recode_edit_batch_o2(C.byref(args_block(RecodeEditO2Args, *a)))

        return _dev_recode_edit(call, self._h, dst.handle, payload, pay_off, nbits, byte_map, span_off, spans, prev0, sym_off, index, chunk_symbols,
                                ws_fn=l.mh_dev_recode_edit_batch_o2_workspace, **kw)

    def dev_recode_splice_table_batch_o2(self, dst, payload, pay_off, nbits, span_tag, reps, span_off, spans, prev0=PREV0, sym_off=None,
                                         index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_splice_table_batch_o2 call (this model is order 2): dev_recode_splice_table_batch's arguments, dict
        and guards."""
        l = lib()

        def call(*a):
            return l.mh_dev_recode_splice_table_batch_o2(C.byref(args_block(RecodeSpliceO2Args, *a)))

        return _dev_recode_splice(call, self._h, dst.handle, payload, pay_off, nbits, b"", span_off, spans, prev0, sym_off, index, chunk_symbols,
                                  table=(span_tag, reps), ws_fn=l.mh_dev_recode_splice_table_batch_o2_workspace, **kw)

    def recode_edit_batch_o2(self, dst, payload, pay_off, nbits, byte_map, **kw):
        """mh_recode_edit_batch_o2 (host form; this model or `dst` is order 2): recode_edit_batch's arguments and results."""
        return self.recode_edit_batch(dst, payload, pay_off, nbits, byte_map, o2=True, **kw)

    def recode_splice_table_batch_o2(self, dst, payload, pay_off, nbits, span_tag, reps, span_off, spans, **kw):
        """mh_recode_splice_table_batch_o2 (host form; this model is order 2): recode_splice_table_batch's arguments and results."""
        return self.recode_splice_batch(dst, payload, pay_off, nbits, b"", span_off, spans, table=(span_tag, reps), o2=True, **kw)

    def recode_splice_batch(self, dst, payload, pay_off, nbits, rep, span_off, spans, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0,
                            cap=None, want_index=True, index_cap=None, check=True, table=None, o2=False):
        """mh_recode_splice_batch (host form): the dict of _recode_batch and out_sym_off[n + 1].  cap / index_cap None: room for
        the worst case, every span one byte wide and replaced.  table = (span_tag, reps): mh_recode_splice_table_batch."""
        l = lib()
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        sof = np.ascontiguousarray(span_off, dtype=np.uint64)
        sp = np.zeros(0, dtype=np.uint64) if spans is None else np.ascontiguousarray(spans, dtype=np.uint64).reshape(-1)
        r = _u8(rep)
        idx = np.ascontiguousarray(index, dtype=np.uint64) if index is not None else None
        if idx is not None:
            so = np.ascontiguousarray(sym_off, dtype=np.uint64).copy()
            bound = int(so[n])
        else:
            so = np.zeros(n + 1, dtype=np.uint64)
            bound = int(sum(int(b) // max(self.min_code_len, 1) for b in nbits))
        bound += (sp.size // 2) * int(r.size)
        if table is not None:
            tg = np.ascontiguousarray(table[0], dtype=np.uint32)
            roff, rb = _rep_table(table[1])
            bound += (sp.size // 2) * SPLICE_MAX_REP
            how = (tg.ctypes.data if tg.size else pay_off.ctypes.data, roff.ctypes.data, _ptr(rb), len(roff) - 1)
            fn, name = l.mh_recode_splice_table_batch, "mh_recode_splice_table_batch"
            if o2:
                fn, name = l.mh_recode_splice_table_batch_o2, "mh_recode_splice_table_batch_o2"
        else:
            how = (_ptr(r), r.size)
            fn, name = l.mh_recode_splice_batch, "mh_recode_splice_batch"
        if cap is None:
            cap = l.mh_encode_batch_bound(dst.handle, bound, n)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        oo, onb, dr = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        oso = np.zeros(n + 1, dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        oi = None
        if want_index and chunk_symbols:
            if index_cap is None:
                index_cap = int(l.mh_batch_index_capacity(bound, n, chunk_symbols))
            oi = np.full(max(index_cap, 1), FIND_FILL, dtype=np.uint64)
        rc = fn(self._h, dst.handle, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0,
                so.ctypes.data, (idx.ctypes.data if idx.size else pay_off.ctypes.data) if idx is not None else None,
                chunk_symbols, sof.ctypes.data, _ptr(sp), *how, out.ctypes.data, cap, oo.ctypes.data,
                onb.ctypes.data, oso.ctypes.data, oi.ctypes.data if oi is not None else None, index_cap or 0, dr.ctypes.data,
                st.ctypes.data)
        if rc != MH_OK and (check or not (st[:n].any() or rc == MH_ERR_CAPACITY)):
            raise MhError(rc, name)
        return dict(payload=out[:min(int(oo[n]), cap)], out_off=oo, nbits=onb[:n], index=oi, dropped=dr[:n], status=st[:n], sym_off=so,
                    out_sym_off=oso, rc=rc)

    def recode_edit_batch(self, dst, payload, pay_off, nbits, byte_map, span_off=None, spans=None, prev0=PREV0, sym_off=None, index=None,
                          chunk_symbols=0, cap=None, want_index=True, check=True, o2=False):
        """mh_recode_edit_batch (host form): recode_batch with the edit; the arguments and results of _recode_batch.  o2:
        mh_recode_edit_batch_o2."""
        so, sp, m = _span_arrays(span_off, spans, byte_map)
        fn = lib().mh_recode_edit_batch_o2 if o2 else lib().mh_recode_edit_batch

        def call(*a):
            return fn(*a[:10], so.ctypes.data if so is not None else None, _ptr(sp), m.ctypes.data, *a[10:])

        return self._recode_batch(call, "mh_recode_edit_batch_o2" if o2 else "mh_recode_edit_batch", dst, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, cap, want_index,
                                  check)

    def recode_batch(self, dst, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, cap=None, want_index=True,
                     check=True):
        """mh_recode_batch (host form): the arguments and results of _recode_batch."""
        return self._recode_batch(lib().mh_recode_batch, "mh_recode_batch", dst, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols,
                                  cap, want_index, check)

    def _recode_batch(self, fn, what, dst, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, cap, want_index, check):
        """mh_recode_batch / mh_recode_batch_o2 (host form): dict(payload, out_off[n + 1], nbits[n], index or None, dropped[n], status[n], sym_off[n + 1], rc).
        cap None: room for the destination's worst case.  check=False returns a failed stream's status or MH_ERR_CAPACITY
        instead of raising."""
        l = lib()
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        idx = np.ascontiguousarray(index, dtype=np.uint64) if index is not None else None
        if idx is not None:
            so = np.ascontiguousarray(sym_off, dtype=np.uint64).copy()
            bound = int(so[n])
        else:
            so = np.zeros(n + 1, dtype=np.uint64)
            bound = int(sum(int(b) // max(self.min_code_len, 1) for b in nbits))
        if cap is None:
            cap = l.mh_encode_batch_bound(dst.handle, bound, n)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        oo, onb, dr = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        st = np.zeros(max(n, 1), dtype=np.int32)
        oi = None
        if want_index and chunk_symbols:
            oi = np.full(max(int(l.mh_batch_index_capacity(bound, n, chunk_symbols)), 1), FIND_FILL, dtype=np.uint64)
        rc = fn(self._h, dst.handle, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0,
                so.ctypes.data, (idx.ctypes.data if idx.size else pay_off.ctypes.data) if idx is not None else None,
                chunk_symbols, out.ctypes.data, cap, oo.ctypes.data, onb.ctypes.data, oi.ctypes.data if oi is not None else None,
                dr.ctypes.data, st.ctypes.data)
        if rc != MH_OK and (check or not (st[:n].any() or rc == MH_ERR_CAPACITY)):
            raise MhError(rc, what)
        return dict(payload=out[:min(int(oo[n]), cap)], out_off=oo, nbits=onb[:n], index=oi, dropped=dr[:n], status=st[:n], sym_off=so, rc=rc)

    def decompress_batch_ranges(self, blobs, lookups, indices=None, chunk_symbols=0, lengths=None):
        """Lookups into whole `.cm` files of this model (decompress_batch's inputs): (list of bytes, status per lookup)."""
        return self._decompress_batch_ranges(blobs, lookups, indices, chunk_symbols, lengths, self.decode_batch_ranges)

    def _decompress_batch_ranges(self, blobs, lookups, indices, chunk_symbols, lengths, decode):
        l = lib()
        payloads, nbits = [], []
        for b in blobs:
            a = _u8(b)
            if a.size < 1:
                raise MhError(MH_ERR_CORRUPT, "decompress_batch_ranges")
            nb = C.c_uint64(0)
            _check(l.mh_stream_parse_header(self._h, int(a[0]), a.size, C.byref(nb)), "mh_stream_parse_header")
            payloads.append(a[1:].tobytes())
            nbits.append(nb.value)
        payload, pay_off = batch_offsets(payloads)
        sym_off = _offsets(lengths) if lengths is not None else None
        index = None
        if indices is not None:
            if lengths is None:
                raise ValueError("decompress_batch_ranges with indices needs the original lengths")
            index = _batch_index(indices, sym_off, chunk_symbols)
        return decode(payload, pay_off, np.array(nbits, dtype=np.uint64), lookups, PREV0, sym_off, index, chunk_symbols)

    # ---- batches of independent streams (mh_encode_batch / mh_decode_batch) -------------------------------------------
    def encode_batch(self, messages, prev0=PREV0, chunk_symbols=None):
        """(packed payloads, out_off[n + 1], nbits[n], index or None, in_off[n + 1]) of one mh_encode_batch call."""
        return self._encode_batch(messages, prev0, chunk_symbols, "mh_encode_batch")

    def _encode_batch(self, messages, prev0, chunk_symbols, fn):
        data, off = batch_offsets(messages)
        l = lib()
        n, total = len(off) - 1, int(data.size)
        cap = l.mh_encode_batch_bound(self._h, total, n)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        nbits = np.zeros(max(n, 1), dtype=np.uint64)
        idx = None
        if chunk_symbols:
            idx = np.zeros(max(l.mh_batch_index_capacity(total, n, chunk_symbols), 1), dtype=np.uint64)
        _check(getattr(l, fn)(self._h, _ptr(data), off.ctypes.data, n, prev0, out.ctypes.data, cap, out_off.ctypes.data,
                              nbits.ctypes.data, idx.ctypes.data if idx is not None else None, chunk_symbols or 0), fn)
        return out[:int(out_off[n])], out_off, nbits[:n], idx, off

    def compress_batch(self, messages, chunk_symbols=None):
        """[(header + payload, nbits, index slice or None)] per message: each blob is the `.cm` file of that message alone."""
        return self._compress_batch(messages, chunk_symbols, self.encode_batch)

    def _compress_batch(self, messages, chunk_symbols, encode):
        messages = [bytes(m) for m in messages]
        payload, out_off, nbits, idx, off = encode(messages, PREV0, chunk_symbols)
        l = lib()
        res = []
        for i, m in enumerate(messages):
            nb = int(nbits[i])
            blob = bytes([l.mh_stream_header(self._h, nb)]) + payload[int(out_off[i]):int(out_off[i + 1])].tobytes()
            sl = None
            if chunk_symbols:
                b = l.mh_batch_index_base(int(off[i]), i, chunk_symbols)
                sl = idx[b:b + (len(m) + chunk_symbols - 1) // chunk_symbols].copy()
            res.append((blob, nb, sl))
        return res

    def decode_batch(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, out_cap=None, check=True):
        """mh_decode_batch: (output bytes, sym_off[n + 1], per-stream status[n]).  With an index, sym_off is the encode's in_off.
        check=False returns the per-stream statuses of a batch with failed streams instead of raising."""
        return self._decode_batch(payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, out_cap, check, "mh_decode_batch")

    def _decode_batch(self, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, out_cap, check, fn):
        l = lib()
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        if index is not None:
            so = np.ascontiguousarray(sym_off, dtype=np.uint64).copy()
            cap = int(so[n]) if out_cap is None else out_cap
            index = np.ascontiguousarray(index, dtype=np.uint64)
        else:
            so = np.zeros(n + 1, dtype=np.uint64)
            minl = max(self.min_code_len, 1)
            cap = int(sum(int(b) // minl for b in nbits)) if out_cap is None else out_cap
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        st = np.zeros(max(n, 1), dtype=np.int32)
        rc = getattr(l, fn)(self._h, _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0, out.ctypes.data, cap,
                            so.ctypes.data, index.ctypes.data if index is not None and index.size else (out.ctypes.data if index is not None else None),
                            chunk_symbols, st.ctypes.data)
        if rc != MH_OK and (check or rc == MH_ERR_ARG or not st[:n].any()):
            raise MhError(rc, fn)
        return out[:int(so[n])].tobytes(), so, st[:n]

    def index_batch(self, payload, pay_off, nbits, chunk_symbols, prev0=PREV0):
        """States + index of index-free payloads on the device: (sym_off[n + 1], index, per-stream status).  The outputs plug
        into decode_batch(..., sym_off=..., index=...) and decode_batch_ranges."""
        return _index_batch(self, payload, pay_off, nbits, chunk_symbols, prev0)

    def decode_batch_segments(self, payload, pay_off, nbits, prev0=PREV0, out_cap=None):
        """States + emit of index-free payloads on the device: (output bytes, sym_off[n + 1], per-stream status)."""
        return _decode_batch_segments(self, payload, pay_off, nbits, prev0, out_cap)

    def decompress_batch(self, blobs, indices=None, chunk_symbols=0, lengths=None):
        """Whole `.cm` files in, original messages out.  With indices (one slice per blob, from compress_batch) the original
        lengths must be given too: the index does not record where a stream's last chunk ends."""
        return self._decompress_batch(blobs, indices, chunk_symbols, lengths, self.decode_batch)

    def _decompress_batch(self, blobs, indices, chunk_symbols, lengths, decode):
        l = lib()
        payloads, nbits = [], []
        for b in blobs:
            a = _u8(b)
            if a.size < 1:
                raise MhError(MH_ERR_CORRUPT, "decompress_batch")
            nb = C.c_uint64(0)
            _check(l.mh_stream_parse_header(self._h, int(a[0]), a.size, C.byref(nb)), "mh_stream_parse_header")
            payloads.append(a[1:].tobytes())
            nbits.append(nb.value)
        payload, pay_off = batch_offsets(payloads)
        sym_off, index = None, None
        if indices is not None:
            if lengths is None:
                raise ValueError("decompress_batch with indices needs the original lengths")
            sym_off = np.zeros(len(blobs) + 1, dtype=np.uint64)
            sym_off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
            total, n = int(sym_off[-1]), len(blobs)
            index = np.zeros(max(l.mh_batch_index_capacity(total, n, chunk_symbols), 1), dtype=np.uint64)
            for i, sl in enumerate(indices):
                b = l.mh_batch_index_base(int(sym_off[i]), i, chunk_symbols)
                index[b:b + len(sl)] = sl
        out, so, _ = decode(payload, pay_off, np.array(nbits, dtype=np.uint64), PREV0, sym_off, index, chunk_symbols)
        return [out[int(so[i]):int(so[i + 1])] for i in range(len(blobs))]

    # ---- batches of order-2 streams (mh_encode_batch_o2 / mh_decode_batch_o2; extension, parity unpinned) ---------------
    def encode_batch_o2(self, messages, prev0=PREV0, chunk_symbols=None):
        """encode_batch for an order-2 model: one mh_encode_batch_o2 call (index entries carry two context bytes)."""
        return self._encode_batch(messages, prev0, chunk_symbols, "mh_encode_batch_o2")

    def compress_batch_o2(self, messages, chunk_symbols=None):
        """compress_batch for an order-2 model: each blob is what compress gives for that message alone."""
        return self._compress_batch(messages, chunk_symbols, self.encode_batch_o2)

    def decode_batch_o2(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, out_cap=None, check=True):
        """decode_batch for an order-2 model (mh_decode_batch_o2)."""
        return self._decode_batch(payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, out_cap, check, "mh_decode_batch_o2")

    def decompress_batch_o2(self, blobs, indices=None, chunk_symbols=0, lengths=None):
        """decompress_batch for an order-2 model."""
        return self._decompress_batch(blobs, indices, chunk_symbols, lengths, self.decode_batch_o2)

    # ---- random access into order-2 streams (mh_decode_batch_o2_ranges / mh_dev_decode_batch_o2_ranges; extension) -------
    def _require_o2(self, what):
        if self.type != 2:
            raise MhError(MH_ERR_ARG, what)

    def decode_batch_o2_ranges(self, payload, pay_off, nbits, lookups, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
        """decode_batch_ranges for an order-2 model (mh_decode_batch_o2_ranges): lookups into an encode_batch_o2 batch."""
        self._require_o2("mh_decode_batch_o2_ranges")
        return self._decode_batch_ranges(payload, pay_off, nbits, lookups, prev0, sym_off, index, chunk_symbols, "mh_decode_batch_o2_ranges")

    def dev_decode_batch_o2_ranges(self, payload, pay_off, nbits, lookups, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0,
                                   out_cap=None):
        """One mh_dev_decode_batch_o2_ranges call with guard bytes around every output: (list of bytes, status per lookup,
        mh_dev_status)."""
        self._require_o2("mh_dev_decode_batch_o2_ranges")
        return _dev_batch_ranges(lib().mh_dev_decode_batch_o2_ranges, self._h, payload, pay_off, nbits, lookups, prev0, sym_off, index,
                                 chunk_symbols, out_cap)

    # ---- order 2 in search and re-coding (include/mh.h, "ORDER 2 IN SEARCH AND RE-CODING") -----------------------------------
    def find_batch_o2(self, ps, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, check=True):
        """mh_find_batch_o2 (host form; this model is order 2): find_batch's arguments and results."""
        return self._find_batch(lib().mh_find_batch_o2, "mh_find_batch_o2", ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols,
                                hit_cap, check)

    def find_dict_batch_o2(self, d, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, check=True):
        """mh_find_dict_batch_o2 (host form; this model is order 2): find_batch's arguments and results with a Dict."""
        return self._find_batch(lib().mh_find_dict_batch_o2, "mh_find_dict_batch_o2", d, payload, pay_off, nbits, prev0, sym_off, index,
                                chunk_symbols, hit_cap, check)

    def dev_find_dict_batch_o2(self, d, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None,
                               count_only=False):
        """One mh_dev_find_dict_batch_o2 call (two when hit_cap is None) with guard words behind its outputs: dev_find_batch's results."""
        return _dev_find(lib().mh_dev_find_dict_batch_o2, self._h, d, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap,
                         count_only, ws_fn=lib().mh_dev_find_dict_workspace)

    def dev_find_batch_o2(self, ps, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None,
                          count_only=False):
        """One mh_dev_find_batch_o2 call (two when hit_cap is None) with guard words behind its outputs: dev_find_batch's results."""
        return _dev_find(lib().mh_dev_find_batch_o2, self._h, ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap,
                         count_only, ws_fn=lib().mh_dev_find_batch_o2_workspace)

    def crc_batch_o2(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, check=True):
        """mh_crc_batch_o2 (host form; this model is order 2): crc_batch's arguments and results."""
        return _host_crc(lib().mh_crc_batch_o2, "mh_crc_batch_o2", self._h, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, check)

    def dev_crc_batch_o2(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_crc_batch_o2 call with guard words behind its outputs: dev_crc_batch's results."""
        return _dev_crc(lib().mh_dev_crc_batch_o2, self._h, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, **kw)

    def dev_histogram_coded_o2(self, order, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
        """One mh_dev_histogram_coded_batch_o2 call on a batch coded under this model (any order; the model or `order` is 2):
        (counts[256, 65536 or 1 << 24], per-stream status[n], mh_dev_status)."""
        return _dev_histogram_coded(lib().mh_dev_histogram_coded_batch_o2, self._h, order, payload, pay_off, nbits, prev0, sym_off, index,
                                    chunk_symbols, ws_fn=lib().mh_dev_histogram_coded_batch_o2_workspace)

    def dev_recode_batch_o2(self, dst, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_batch_o2 call (this model or `dst` is order 2) with guards around its outputs: the dict of _dev_recode."""
        return _dev_recode(lib().mh_dev_recode_batch_o2, self._h, dst.handle, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols,
                           ws_fn=lib().mh_dev_recode_batch_o2_workspace, **kw)

    def recode_batch_o2(self, dst, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, cap=None, want_index=True,
                        check=True):
        """mh_recode_batch_o2 (host form; this model or `dst` is order 2): recode_batch's arguments and results."""
        return self._recode_batch(lib().mh_recode_batch_o2, "mh_recode_batch_o2", dst, payload, pay_off, nbits, prev0, sym_off, index,
                                  chunk_symbols, cap, want_index, check)

    # ---- segment states of index-free order-2 batches (include/mh.h, "SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES") --------
    def index_batch_o2(self, payload, pay_off, nbits, chunk_symbols, prev0=PREV0):
        """index_batch for an order-2 model (mh_dev_batch_states_o2 + mh_dev_batch_index_o2): the outputs plug into
        decode_batch_o2(..., sym_off=..., index=...), decode_batch_o2_ranges and the indexed find / recode calls."""
        return _index_batch(self, payload, pay_off, nbits, chunk_symbols, prev0, o2=True)

    def decode_batch_segments_o2(self, payload, pay_off, nbits, prev0=PREV0, out_cap=None):
        """decode_batch_segments for an order-2 model (mh_dev_batch_states_o2 + mh_dev_batch_emit_o2)."""
        return _decode_batch_segments(self, payload, pay_off, nbits, prev0, out_cap, o2=True)

    def decompress_batch_o2_ranges(self, blobs, lookups, indices=None, chunk_symbols=0, lengths=None):
        """decompress_batch_ranges for an order-2 model: lookups into whole `.cm` files of compress_batch_o2."""
        self._require_o2("mh_decode_batch_o2_ranges")
        return self._decompress_batch_ranges(blobs, lookups, indices, chunk_symbols, lengths, self.decode_batch_o2_ranges)


# ---- batches of streams, one model each (include/mh.h, "BATCHES OF STREAMS, ONE MODEL EACH") ----------------------------
def stream_header(order, nbits):
    """The `.cm` / `.ch` header byte of a payload of nbits under an order-0/1 model (src/coding.cpp:88)."""
    return 0x30 | ((~order & 1) << 3) | ((8 - nbits % 8) % 8)


def table_order(table):
    """Order of a table file: 1 for a Markov table (leading 1 bit), 0 for a Huffman tree (and the empty order-0 table)."""
    return (table[0] >> 7) & 1 if len(table) else 0


def parse_stream_header(order, blob):
    """nbits of a whole `.cm` / `.ch` file written under a model of this order."""
    a = _u8(blob)
    if a.size < 1:
        raise MhError(MH_ERR_CORRUPT, "parse_stream_header")
    h = int(a[0])
    if (h & 0xF0) != 0x30:
        raise MhError(MH_ERR_CORRUPT, "parse_stream_header")
    if ((h >> 3) & 1) != (~order & 1):
        raise MhError(MH_ERR_TYPE, "parse_stream_header")
    pad = h & 7
    if (a.size - 1) * 8 < pad:
        raise MhError(MH_ERR_CORRUPT, "parse_stream_header")
    return (a.size - 1) * 8 - pad


def _offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        off[1:] = np.cumsum(np.asarray(lengths, dtype=np.uint64), dtype=np.uint64)
    return off


class ModelSet:
    """Owns an mh_model_set*: one model per stream, resident on the current device."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def train(cls, messages, order=1, prev0=PREV0):
        """One model per message, trained on the device (mh_dev_model_set_train)."""
        data, off = batch_offsets(messages)
        l = lib()
        total, n = int(data.size), len(off) - 1
        d_data = DeviceBuffer(max(total, 1), data if total else None)
        d_off = DeviceBuffer(off.nbytes, off)
        wsb = l.mh_dev_model_set_train_workspace(n)
        d_ws = DeviceBuffer(wsb)
        h = C.c_void_p()
        _check(l.mh_dev_model_set_train(d_data.ptr, d_off.ptr, n, total, order, prev0, d_ws.ptr, wsb, None, C.byref(h)), "mh_dev_model_set_train")
        return cls(h)

    @classmethod
    def from_models(cls, models):
        arr = (C.c_void_p * max(len(models), 1))(*[m.handle for m in models])
        h = C.c_void_p()
        _check(lib().mh_model_set_from_models(arr, len(models), C.byref(h)), "mh_model_set_from_models")
        return cls(h)

    @classmethod
    def from_tables(cls, tables):
        tables = [bytes(t) for t in tables]
        buf = np.frombuffer(b"".join(tables), dtype=np.uint8)
        off = _offsets([len(t) for t in tables])
        h = C.c_void_p()
        _check(lib().mh_model_set_from_tables(_ptr(buf), off.ctypes.data, len(tables), C.byref(h)), "mh_model_set_from_tables")
        return cls(h)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.mh_model_set_free(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def __len__(self):
        return lib().mh_model_set_size(self._h)

    @property
    def slots(self):
        return lib().mh_model_set_slots(self._h)

    def stream_info(self, i):
        """(type, max code length) of stream i's model."""
        t, m = C.c_int(), C.c_int()
        _check(lib().mh_model_set_stream_info(self._h, i, C.byref(t), C.byref(m)), "mh_model_set_stream_info")
        return t.value, m.value

    def code_lens(self):
        a, b = C.c_int(), C.c_int()
        _check(lib().mh_model_set_code_lens(self._h, C.byref(a), C.byref(b)), "mh_model_set_code_lens")
        return a.value, b.value

    def table_bytes(self):
        """Every stream's table file (mh_dev_model_set_tables)."""
        l = lib()
        n = len(self)
        cap = l.mh_model_set_tables_bound(self._h)
        wsb = l.mh_dev_model_set_tables_workspace(self._h)
        d_out, d_off, d_ws = DeviceBuffer(max(cap, 1)), DeviceBuffer((n + 1) * 8), DeviceBuffer(wsb)
        _check(l.mh_dev_model_set_tables(self._h, d_out.ptr, cap, d_off.ptr, d_ws.ptr, wsb, None), "mh_dev_model_set_tables")
        _check(l.mh_dev_status(d_ws.ptr, None), "mh_dev_model_set_tables")
        off = d_off.download(np.uint64)
        out = d_out.download()
        return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]

    def encode(self, messages, prev0=PREV0, chunk_symbols=None, cap=None, guard=0):
        """mh_dev_encode_each: (packed payloads, out_off[n + 1], nbits[n], index or None, in_off[n + 1], status).  With cap,
        the payload buffer has that size and `guard` bytes behind it, which must come back untouched."""
        data, off = batch_offsets(messages)
        l = lib()
        n, total = len(off) - 1, int(data.size)
        if cap is None:
            cap = l.mh_encode_each_bound(self._h, total, n)
        init = np.full(cap + guard, 0xA5, dtype=np.uint8) if guard else None
        d_data = DeviceBuffer(max(total, 1), data if total else None)
        d_in = DeviceBuffer(off.nbytes, off)
        d_out = DeviceBuffer(max(cap + guard, 1), init)
        d_oo, d_nb = DeviceBuffer((n + 1) * 8), DeviceBuffer(max(n, 1) * 8)
        d_idx = None
        if chunk_symbols:
            nidx = max(l.mh_batch_index_capacity(total, n, chunk_symbols), 1)
            d_idx = DeviceBuffer(nidx * 8, np.zeros(nidx, dtype=np.uint64))       # (gap entries are left untouched: mh.h)
        wsb = l.mh_dev_encode_each_workspace(n, total)
        d_ws = DeviceBuffer(wsb)
        _check(l.mh_dev_encode_each(self._h, d_data.ptr, d_in.ptr, n, total, prev0, d_out.ptr, cap, d_oo.ptr, d_nb.ptr,
                                    d_idx.ptr if d_idx else None, chunk_symbols or 0, d_ws.ptr, wsb, None), "mh_dev_encode_each")
        rc = l.mh_dev_status(d_ws.ptr, None)
        out = d_out.download()
        if guard:
            assert (out[cap:cap + guard] == 0xA5).all(), "bytes written at or beyond cap"
        oo = d_oo.download(np.uint64)
        idx = d_idx.download(np.uint64) if d_idx else None
        return out[:int(oo[n]) if rc == MH_OK else 0], oo, d_nb.download(np.uint64)[:n], idx, off, rc

    def decode(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, out_cap=None, guard=0):
        """mh_dev_decode_each: (output bytes, sym_off[n + 1], per-stream status[n], device status)."""
        l = lib()
        payload = _u8(payload)
        pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        n = len(pay_off) - 1
        if index is not None:
            so = np.ascontiguousarray(sym_off, dtype=np.uint64).copy()
            cap = int(so[n]) if out_cap is None else out_cap
        else:
            so = np.zeros(n + 1, dtype=np.uint64)
            minl = max(self.code_lens()[1], 1)
            cap = int(sum(int(b) // minl for b in nbits)) if out_cap is None else out_cap
        d_pl = DeviceBuffer(max(payload.size, 1) + 64, payload if payload.size else None)
        d_po, d_nb = DeviceBuffer(pay_off.nbytes, pay_off), DeviceBuffer(max(nbits.nbytes, 8), nbits if n else None)
        d_out = DeviceBuffer(max(cap + guard, 1), np.full(cap + guard, 0xA5, dtype=np.uint8) if guard else None)
        d_so = DeviceBuffer(so.nbytes, so)
        d_idx = None
        if index is not None:
            index = np.ascontiguousarray(index, dtype=np.uint64)
            d_idx = DeviceBuffer(max(index.nbytes, 8), index if index.size else None)
        d_st = DeviceBuffer(max(n, 1) * 4)
        wsb = l.mh_dev_decode_each_workspace(n)
        d_ws = DeviceBuffer(wsb)
        _check(l.mh_dev_decode_each(self._h, d_pl.ptr, d_po.ptr, d_nb.ptr, n, int(pay_off[n]), prev0, d_out.ptr, cap, d_so.ptr,
                                    int(so[n]), d_idx.ptr if d_idx else None, chunk_symbols, d_st.ptr, d_ws.ptr, wsb, None), "mh_dev_decode_each")
        rc = l.mh_dev_status(d_ws.ptr, None)
        out = d_out.download()
        if guard:
            assert (out[cap:cap + guard] == 0xA5).all(), "bytes written at or beyond out_cap"
        so = d_so.download(np.uint64)
        return out[:min(int(so[n]), cap)].tobytes(), so, d_st.download(np.int32)[:n], rc


    def index_batch(self, payload, pay_off, nbits, chunk_symbols, prev0=PREV0):
        """States + index under the set (stream i under model i): (sym_off[n + 1], index, per-stream status)."""
        return _index_batch(self, payload, pay_off, nbits, chunk_symbols, prev0)

    def decode_batch_segments(self, payload, pay_off, nbits, prev0=PREV0, out_cap=None):
        """States + emit under the set: (output bytes, sym_off[n + 1], per-stream status)."""
        return _decode_batch_segments(self, payload, pay_off, nbits, prev0, out_cap)

    def decode_ranges(self, payload, pay_off, nbits, lookups, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, out_cap=None):
        """One mh_dev_decode_each_ranges call with guard bytes around every output: (list of bytes, status per lookup,
        mh_dev_status)."""
        return _dev_batch_ranges(lib().mh_dev_decode_each_ranges, self._h, payload, pay_off, nbits, lookups, prev0, sym_off, index,
                                 chunk_symbols, out_cap)

    def find(self, ps, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, count_only=False):
        """One mh_dev_find_each call (two when hit_cap is None) with guard words behind its outputs, stream i under model i:
        (hit_off[n + 1], hits[k, 3], hit_pattern[k], per-stream status[n], mh_dev_status)."""
        return _dev_find(lib().mh_dev_find_each, self._h, ps, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap, count_only)

    def find_dict(self, d, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, hit_cap=None, count_only=False):
        """One mh_dev_find_dict_each call (two when hit_cap is None) with guard words behind its outputs, stream i under model i:
        find's results with a Dict for the pattern set."""
        return _dev_find(lib().mh_dev_find_dict_each, self._h, d, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, hit_cap,
                         count_only, ws_fn=lib().mh_dev_find_dict_workspace)

    def crc(self, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_crc_each call with guard words behind its outputs, stream i under model i: (crc[n], len[n], per-stream
        status[n], mh_dev_status)."""
        return _dev_crc(lib().mh_dev_crc_each, self._h, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, **kw)

    def histogram_coded(self, order, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0):
        """One mh_dev_histogram_coded_each call: (counts, per-stream status[n], mh_dev_status)."""
        return _dev_histogram_coded(lib().mh_dev_histogram_coded_each, self._h, order, payload, pay_off, nbits, prev0, sym_off, index,
                                    chunk_symbols)

    def recode(self, dst, payload, pay_off, nbits, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_each call (stream i coded under this set's model i, coded again under the shared model `dst`):
        the dict of _dev_recode."""
        return _dev_recode(lib().mh_dev_recode_each, self._h, dst.handle, payload, pay_off, nbits, prev0, sym_off, index, chunk_symbols, **kw)

    def recode_edit(self, dst, payload, pay_off, nbits, byte_map, span_off=None, spans=None, prev0=PREV0, sym_off=None, index=None,
                    chunk_symbols=0, **kw):
        """One mh_dev_recode_edit_each call: recode with map[b] coded for every byte b inside the spans: the dict of _dev_recode."""
        return _dev_recode_edit(lib().mh_dev_recode_edit_each, self._h, dst.handle, payload, pay_off, nbits, byte_map, span_off, spans, prev0,
                                sym_off, index, chunk_symbols, **kw)

    def recode_splice_table(self, dst, payload, pay_off, nbits, span_tag, reps, span_off, spans, prev0=PREV0, sym_off=None, index=None,
                            chunk_symbols=0, **kw):
        """One mh_dev_recode_splice_table_each call: Model.dev_recode_splice_table_batch under this set."""
        return _dev_recode_splice(lib().mh_dev_recode_splice_table_each, self._h, dst.handle, payload, pay_off, nbits, b"", span_off, spans, prev0,
                                  sym_off, index, chunk_symbols, table=(span_tag, reps), **kw)

    def recode_splice(self, dst, payload, pay_off, nbits, rep, span_off, spans, prev0=PREV0, sym_off=None, index=None, chunk_symbols=0, **kw):
        """One mh_dev_recode_splice_each call: recode with every span replaced by `rep` (b"": deleted): the dict of
        _dev_recode_splice."""
        return _dev_recode_splice(lib().mh_dev_recode_splice_each, self._h, dst.handle, payload, pay_off, nbits, rep, span_off, spans, prev0,
                                  sym_off, index, chunk_symbols, **kw)

    # ---- banks of shared models (include/mh.h, "BANKS OF SHARED MODELS"): this set is the bank, its streams the entries ----
    @classmethod
    def train_bank(cls, messages, k, order=1, max_iters=8, prev0=PREV0, host=False):
        """K shared models trained on the messages: (bank, choice uint32[n], iterations run).  host=False drives
        mh_dev_bank_train on device buffers, host=True the host form mh_bank_train."""
        data, off = batch_offsets(messages)
        l = lib()
        total, n = int(data.size), len(off) - 1
        h, it = C.c_void_p(), C.c_int(0)
        if host:
            ch = np.zeros(max(n, 1), dtype=np.uint32)
            _check(l.mh_bank_train(_ptr(data), off.ctypes.data, n, order, prev0, k, max_iters, ch.ctypes.data, C.byref(it), C.byref(h)),
                   "mh_bank_train")
            return cls(h), ch[:n], it.value
        d_data = DeviceBuffer(max(total, 1), data if total else None)
        d_off = DeviceBuffer(off.nbytes, off)
        d_ch = DeviceBuffer(max(n, 1) * 4)
        wsb = l.mh_dev_bank_train_workspace(n, total, k)
        d_ws = DeviceBuffer(wsb)
        _check(l.mh_dev_bank_train(d_data.ptr, d_off.ptr, n, total, order, prev0, k, max_iters, d_ch.ptr, C.byref(it), d_ws.ptr, wsb, None,
                                   C.byref(h)), "mh_dev_bank_train")
        return cls(h), d_ch.download(np.uint32)[:n], it.value

    def select(self, messages, prev0=PREV0, in_off=None):
        """mh_dev_bank_select with this set as the bank: (choice uint32[n], nbits uint64[n]).  messages: a list of byte strings,
        or the concatenation with in_off (which may be malformed: the device status is then raised)."""
        l = lib()
        if in_off is None:
            data, off = batch_offsets(messages)
        else:
            data, off = _u8(messages), np.ascontiguousarray(in_off, dtype=np.uint64)
        total, n = int(data.size), len(off) - 1
        d_data = DeviceBuffer(max(total, 1), data if total else None)
        d_off = DeviceBuffer(off.nbytes, off)
        d_ch, d_nb = DeviceBuffer(max(n, 1) * 4), DeviceBuffer(max(n, 1) * 8)
        wsb = l.mh_dev_bank_select_workspace(len(self), n, total)
        d_ws = DeviceBuffer(wsb)
        _check(l.mh_dev_bank_select(self._h, d_data.ptr, d_off.ptr, n, total, prev0, d_ch.ptr, d_nb.ptr, d_ws.ptr, wsb, None), "mh_dev_bank_select")
        _check(l.mh_dev_status(d_ws.ptr, None), "mh_dev_bank_select")
        return d_ch.download(np.uint32)[:n], d_nb.download(np.uint64)[:n]

    def pick(self, choice):
        """mh_dev_model_set_pick: the set in which stream i is coded under this bank's entry choice[i]."""
        ch = np.ascontiguousarray(choice, dtype=np.uint32)
        d_ch = DeviceBuffer(max(ch.nbytes, 4), ch if ch.size else None)
        h = C.c_void_p()
        _check(lib().mh_dev_model_set_pick(self._h, d_ch.ptr, ch.size, None, C.byref(h)), "mh_dev_model_set_pick")
        return ModelSet(h)


def encode_bank_bound(bank, messages, choice):
    _, off = batch_offsets(messages)
    ch = np.ascontiguousarray(choice, dtype=np.uint32)
    return lib().mh_encode_bank_bound(bank.handle, _ptr(ch), off.ctypes.data, len(off) - 1)


def encode_bank(bank, messages, choice, chunk_symbols=None, prev0=PREV0):
    """mh_encode_bank: (packed payloads, out_off[n + 1], nbits[n], index or None, in_off[n + 1]); stream i under bank entry choice[i]."""
    data, off = batch_offsets(messages)
    l = lib()
    n, total = len(off) - 1, int(data.size)
    ch = np.ascontiguousarray(choice, dtype=np.uint32)
    cap = l.mh_encode_bank_bound(bank.handle, _ptr(ch), off.ctypes.data, n)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    nbits = np.zeros(max(n, 1), dtype=np.uint64)
    idx = None
    if chunk_symbols:
        idx = np.zeros(max(l.mh_batch_index_capacity(total, n, chunk_symbols), 1), dtype=np.uint64)
    _check(l.mh_encode_bank(bank.handle, _ptr(data), off.ctypes.data, n, prev0, _ptr(ch), out.ctypes.data, cap, out_off.ctypes.data,
                            nbits.ctypes.data, idx.ctypes.data if idx is not None else None, chunk_symbols or 0), "mh_encode_bank")
    return out[:int(out_off[n])], out_off, nbits[:n], idx, off


def decode_bank(bank, choice, payload, pay_off, nbits, sym_off=None, index=None, chunk_symbols=0, out_cap=None, prev0=PREV0, check=True):
    """mh_decode_bank: (output bytes, sym_off[n + 1], per-stream status[n]).  With an index, sym_off is the encode's in_off."""
    l = lib()
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    ch = np.ascontiguousarray(choice, dtype=np.uint32)
    n = len(pay_off) - 1
    if index is not None:
        so = np.ascontiguousarray(sym_off, dtype=np.uint64).copy()
        cap = int(so[n]) if out_cap is None else out_cap
        index = np.ascontiguousarray(index, dtype=np.uint64)
    else:
        so = np.zeros(n + 1, dtype=np.uint64)
        minl = max(bank.code_lens()[1], 1)
        cap = int(sum(int(b) // minl for b in nbits)) if out_cap is None else out_cap
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = l.mh_decode_bank(bank.handle, _ptr(ch), _ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0, out.ctypes.data,
                          cap, so.ctypes.data, (index.ctypes.data if index.size else out.ctypes.data) if index is not None else None, chunk_symbols,
                          st.ctypes.data)
    if rc != MH_OK and (check or rc == MH_ERR_ARG or not st[:n].any()):
        raise MhError(rc, "mh_decode_bank")
    return out[:int(so[n])].tobytes(), so, st[:n]


def compress_each(messages, order=1, chunk_symbols=None, prev0=PREV0):
    """[(table bytes, header + payload, nbits, index slice or None)] per message: the `.e`/`.eh` table and `.cm`/`.ch` file the
    reference writes for that message alone (mh_compress_each)."""
    messages = [bytes(m) for m in messages]
    data, off = batch_offsets(messages)
    l = lib()
    n = len(messages)
    tb, pb = C.c_size_t(0), C.c_size_t(0)
    _check(l.mh_compress_each_bounds(off.ctypes.data, n, C.byref(tb), C.byref(pb)), "mh_compress_each_bounds")
    tables = np.zeros(max(tb.value, 1), dtype=np.uint8)
    payload = np.zeros(max(pb.value, 1), dtype=np.uint8)
    tab_off, out_off = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    nbits = np.zeros(max(n, 1), dtype=np.uint64)
    idx = None
    if chunk_symbols:
        idx = np.zeros(max(l.mh_batch_index_capacity(int(data.size), n, chunk_symbols), 1), dtype=np.uint64)
    _check(l.mh_compress_each(_ptr(data), off.ctypes.data, n, order, prev0, tables.ctypes.data, tb.value, tab_off.ctypes.data,
                              payload.ctypes.data, pb.value, out_off.ctypes.data, nbits.ctypes.data,
                              idx.ctypes.data if idx is not None else None, chunk_symbols or 0), "mh_compress_each")
    res = []
    for i, m in enumerate(messages):
        nb = int(nbits[i])
        sl = None
        if chunk_symbols:
            b = l.mh_batch_index_base(int(off[i]), i, chunk_symbols)
            sl = idx[b:b + (len(m) + chunk_symbols - 1) // chunk_symbols].copy()
        res.append((tables[int(tab_off[i]):int(tab_off[i + 1])].tobytes(),
                    bytes([stream_header(order, nb)]) + payload[int(out_off[i]):int(out_off[i + 1])].tobytes(), nb, sl))
    return res


def decompress_each(tables, blobs, indices=None, chunk_symbols=0, lengths=None, prev0=PREV0, check=True):
    """Table files and whole `.cm` / `.ch` files in, original messages out (mh_decompress_each).  With indices (one slice per
    blob, from compress_each) the original lengths must be given too.  check=False returns (messages, per-stream status)
    instead of raising on a failed stream."""
    l = lib()
    tables = [bytes(t) for t in tables]
    payloads, nbits = [], []
    for t, b in zip(tables, blobs):
        nbits.append(parse_stream_header(table_order(t), b))
        payloads.append(bytes(b)[1:])
    n = len(tables)
    tab, tab_off = batch_offsets(tables)
    payload, pay_off = batch_offsets(payloads)
    nb = np.array(nbits if n else [0], dtype=np.uint64)
    idx = None
    if indices is not None:
        if lengths is None:
            raise ValueError("decompress_each with indices needs the original lengths")
        sym_off = _offsets(lengths)
        cap = int(sym_off[n])
        idx = np.zeros(max(l.mh_batch_index_capacity(cap, n, chunk_symbols), 1), dtype=np.uint64)
        for i, sl in enumerate(indices):
            b = l.mh_batch_index_base(int(sym_off[i]), i, chunk_symbols)
            idx[b:b + len(sl)] = sl
    else:
        sym_off = np.zeros(n + 1, dtype=np.uint64)
        cap = int(sum(int(b) for b in nbits))             # every code has at least one bit
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = l.mh_decompress_each(_ptr(tab), tab_off.ctypes.data, _ptr(payload), pay_off.ctypes.data, nb.ctypes.data, n, prev0,
                              out.ctypes.data, cap, sym_off.ctypes.data, idx.ctypes.data if idx is not None else None,
                              chunk_symbols, st.ctypes.data)
    if rc != MH_OK and (check or rc == MH_ERR_ARG or not st[:n].any()):
        raise MhError(rc, "mh_decompress_each")
    msgs = [out[int(sym_off[i]):int(sym_off[i + 1])].tobytes() for i in range(n)]
    return msgs if check else (msgs, st[:n])



# ---- segment states of index-free batches (include/mh.h, "SEGMENT STATES OF INDEX-FREE BATCHES") -------------------------
class SegmentStates:
    """mh_dev_batch_states / mh_dev_each_states on a batch of index-free payloads (model: a Model or a ModelSet), with the
    batch and the workspace kept on the device for index() and emit().  o2=True: the _o2 calls, for a batch coded under a
    Model of type 2 (the order-0/1 calls refuse one).  Attributes: sym_off[n + 1], status[n] (per stream), rc
    (mh_dev_status after the states)."""

    def __init__(self, model, payload, pay_off, nbits, prev0=PREV0, o2=False):
        l = lib()
        self.model = model
        self.is_set = isinstance(model, ModelSet)
        if o2 and self.is_set:
            raise MhError(MH_ERR_ARG, "mh_dev_batch_states_o2")
        self.o2 = o2
        payload = _u8(payload)
        self.pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
        nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
        self.n = n = len(self.pay_off) - 1
        self.pay_total = int(self.pay_off[n])
        self.prev0 = prev0
        self.d_pl = DeviceBuffer(max(payload.size, 1) + 64, payload if payload.size else None)
        self.d_po = DeviceBuffer(self.pay_off.nbytes, self.pay_off)
        self.d_nb = DeviceBuffer(max(nbits.nbytes, 8), nbits if n else None)
        self.d_so = DeviceBuffer((n + 1) * 8)
        self.d_st = DeviceBuffer(max(n, 1) * 4)
        self.wsb = (l.mh_dev_batch_states_o2_workspace if o2 else l.mh_dev_batch_states_workspace)(n, self.pay_total)
        self.d_ws = DeviceBuffer(self.wsb)
        fn = l.mh_dev_batch_states_o2 if o2 else l.mh_dev_each_states if self.is_set else l.mh_dev_batch_states
        _check(fn(model.handle, self.d_pl.ptr, self.d_po.ptr, self.d_nb.ptr, n, self.pay_total, prev0, self.d_so.ptr, self.d_st.ptr,
                  self.d_ws.ptr, self.wsb, None), fn.__name__)
        self.rc = l.mh_dev_status(self.d_ws.ptr, None)
        self.sym_off = self.d_so.download(np.uint64)
        self.status = self.d_st.download(np.int32)[:n]

    def _args(self):
        return (self.model.handle, self.d_pl.ptr, self.d_po.ptr, self.d_nb.ptr, self.n, self.pay_total, self.prev0)

    def states_stats(self):
        """mh_dev_batch_states_stats of this workspace: (repair launches that rewrote a record, streams the one-lane fallback
        walked)."""
        passes, walked = C.c_uint32(0), C.c_uint64(0)
        _check(lib().mh_dev_batch_states_stats(self.d_ws.ptr, None, C.byref(passes), C.byref(walked)), "mh_dev_batch_states_stats")
        return passes.value, walked.value

    def index(self, chunk_symbols, index_cap=None, init=None, guard=0, ws=None):
        """(index[index_cap], per-stream status, device status).  init: the index's previous contents (gap entries keep
        them); ws: another SegmentStates whose workspace is handed over instead of this one's."""
        l = lib()
        if index_cap is None:
            index_cap = l.mh_batch_index_capacity(int(self.sym_off[self.n]), self.n, chunk_symbols)
        buf = np.full(index_cap + guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64) if init is None else np.concatenate(
            [np.ascontiguousarray(init, dtype=np.uint64), np.full(guard, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)])
        d_idx = DeviceBuffer(max(buf.nbytes, 8), buf if buf.size else None)
        d_st = DeviceBuffer(max(self.n, 1) * 4)
        w = ws if ws is not None else self
        fn = l.mh_dev_batch_index_o2 if self.o2 else l.mh_dev_each_index if self.is_set else l.mh_dev_batch_index
        _check(fn(*self._args(), d_idx.ptr, index_cap, chunk_symbols, d_st.ptr, w.d_ws.ptr, w.wsb, None), fn.__name__)
        rc = l.mh_dev_status(w.d_ws.ptr, None)
        out = d_idx.download(np.uint64)[:buf.size]
        if guard:
            assert (out[index_cap:] == 0xA5A5A5A5A5A5A5A5).all(), "index entries written at or beyond index_cap"
        return out[:index_cap], d_st.download(np.int32)[:self.n], rc

    def emit(self, out_cap=None, guard=0, ws=None):
        """(output bytes, per-stream status, device status): the decoded streams at out[sym_off[i] ...)."""
        l = lib()
        if out_cap is None:
            out_cap = int(self.sym_off[self.n])
        d_out = DeviceBuffer(max(out_cap + guard, 1), np.full(out_cap + guard, 0xA5, dtype=np.uint8) if guard else None)
        d_st = DeviceBuffer(max(self.n, 1) * 4)
        w = ws if ws is not None else self
        fn = l.mh_dev_batch_emit_o2 if self.o2 else l.mh_dev_each_emit if self.is_set else l.mh_dev_batch_emit
        _check(fn(*self._args(), d_out.ptr, out_cap, d_st.ptr, w.d_ws.ptr, w.wsb, None), fn.__name__)
        rc = l.mh_dev_status(w.d_ws.ptr, None)
        out = d_out.download()
        if guard:
            assert (out[out_cap:out_cap + guard] == 0xA5).all(), "bytes written at or beyond out_cap"
        return out[:min(int(self.sym_off[self.n]), out_cap)].tobytes(), d_st.download(np.int32)[:self.n], rc


def _index_batch(model, payload, pay_off, nbits, chunk_symbols, prev0, o2=False):
    st = SegmentStates(model, payload, pay_off, nbits, prev0, o2=o2)
    idx, status, _ = st.index(chunk_symbols, init=np.zeros(lib().mh_batch_index_capacity(int(st.sym_off[st.n]), st.n, chunk_symbols),
                                                         dtype=np.uint64))
    return st.sym_off, idx, status


def _decode_batch_segments(model, payload, pay_off, nbits, prev0, out_cap, o2=False):
    st = SegmentStates(model, payload, pay_off, nbits, prev0, o2=o2)
    out, status, _ = st.emit(out_cap)
    return out, st.sym_off, status


def index_batch_host(model, payload, pay_off, nbits, chunk_symbols, prev0=PREV0, check=True):
    """mh_index_batch: (sym_off[n + 1], index, per-stream status) of index-free payloads under one shared model; streams the
    device refuses are indexed one by one."""
    return _index_host(lambda *a: lib().mh_index_batch(model.handle, *a), payload, pay_off, nbits, chunk_symbols, prev0, check)


def index_batch_host_o2(model, payload, pay_off, nbits, chunk_symbols, prev0=PREV0, check=True):
    """mh_index_batch_o2: index_batch_host for a batch coded under an order-2 model."""
    return _index_host(lambda *a: lib().mh_index_batch_o2(model.handle, *a), payload, pay_off, nbits, chunk_symbols, prev0, check)


def _index_host(call, payload, pay_off, nbits, chunk_symbols, prev0, check):
    l = lib()
    payload = _u8(payload)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    cap = l.mh_batch_index_capacity(int(sum(int(b) for b in nbits)), n, chunk_symbols)   # every code has at least one bit
    so = np.zeros(n + 1, dtype=np.uint64)
    idx = np.zeros(max(cap, 1), dtype=np.uint64)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = call(_ptr(payload), pay_off.ctypes.data, nbits.ctypes.data if n else None, n, prev0, chunk_symbols, so.ctypes.data,
              idx.ctypes.data, cap, st.ctypes.data)
    if rc != MH_OK and (check or rc == MH_ERR_ARG or not st[:n].any()):
        raise MhError(rc, "index (host form)")
    return so, idx[:l.mh_batch_index_capacity(int(so[n]), n, chunk_symbols)], st[:n]


def index_each(tables, blobs, chunk_symbols, prev0=PREV0, check=True):
    """Table files and whole `.cm` / `.ch` files (what the reference writes) in: (sym_off[n + 1], index, per-stream status)
    of the batch (mh_index_each).  sym_off and index plug into decompress_each / ModelSet.decode / decode_ranges."""
    tables = [bytes(t) for t in tables]
    payloads, nbits = [], []
    for t, b in zip(tables, blobs):
        nbits.append(parse_stream_header(table_order(t), b))
        payloads.append(bytes(b)[1:])
    tab, tab_off = batch_offsets(tables)
    payload, pay_off = batch_offsets(payloads)
    call = lambda *a: lib().mh_index_each(_ptr(tab), tab_off.ctypes.data, *a)
    return _index_host(call, payload, pay_off, np.array(nbits, dtype=np.uint64), chunk_symbols, prev0, check)


def _batch_index(indices, sym_off, chunk_symbols):
    """The batch index of per-stream slices (compress_batch / compress_each), at mh_batch_index_base."""
    l = lib()
    n = len(indices)
    idx = np.zeros(max(l.mh_batch_index_capacity(int(sym_off[n]), n, chunk_symbols), 1), dtype=np.uint64)
    for i, sl in enumerate(indices):
        b = l.mh_batch_index_base(int(sym_off[i]), i, chunk_symbols)
        idx[b:b + len(sl)] = sl
    return idx


def decompress_each_ranges(tables, blobs, lookups, indices=None, chunk_symbols=0, lengths=None, prev0=PREV0):
    """Lookups (stream, begin, end) into messages given as their table files and whole `.cm` / `.ch` files (decompress_each's
    inputs), through mh_decompress_each_ranges: only the touched streams' tables are parsed and only their payloads uploaded.
    Returns (list of byte strings, int32 status per lookup)."""
    tables = [bytes(t) for t in tables]
    payloads, nbits = [], []
    for t, b in zip(tables, blobs):
        nbits.append(parse_stream_header(table_order(t), b))
        payloads.append(bytes(b)[1:])
    tab, tab_off = batch_offsets(tables)
    payload, pay_off = batch_offsets(payloads)
    return _each_ranges(tab, tab_off, payload, pay_off, np.array(nbits, dtype=np.uint64), lookups, indices, chunk_symbols, lengths, prev0)


def _each_ranges(tab, tab_off, payload, pay_off, nbits, lookups, indices=None, chunk_symbols=0, lengths=None, prev0=PREV0, index=None):
    """mh_decompress_each_ranges on packed inputs (tables + tab_off, payloads + pay_off, nbits); the index either as per-stream
    slices (indices) or as the batch index itself (index)."""
    tab, payload = _u8(tab), _u8(payload)
    tab_off = np.ascontiguousarray(tab_off, dtype=np.uint64)
    pay_off = np.ascontiguousarray(pay_off, dtype=np.uint64)
    nbits = np.ascontiguousarray(nbits, dtype=np.uint64)
    n = len(pay_off) - 1
    sym_off = _offsets(lengths) if lengths is not None else None
    if indices is not None:
        if lengths is None:
            raise ValueError("decompress_each_ranges with indices needs the original lengths")
        index = _batch_index(indices, sym_off, chunk_symbols)
    if index is not None:
        index = np.ascontiguousarray(index, dtype=np.uint64)
    lk = _lookups(lookups)
    m = lk.shape[0]
    call = lambda out, cap, oo, st: lib().mh_decompress_each_ranges(
        _ptr(tab), tab.size, tab_off.ctypes.data, _ptr(payload), payload.size, pay_off.ctypes.data, nbits.ctypes.data if n else None, n,
        prev0, sym_off.ctypes.data if sym_off is not None else None, index.ctypes.data if index is not None else None,
        chunk_symbols, lk.ctypes.data if m else None, m, out, cap, oo, st)
    return _host_batch_ranges(call, "mh_decompress_each_ranges", lk, nbits[:n], sym_off)
