/*
 * mh.h — C ABI of the MI355X-native Markov-Huffman codec (libmhc.so).
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (jeremy-rifkin/Markov-Huffman-Coding) has no FFI of its own: its seam is the
 * C++ class i_coding_provider (src/coding.h:18-35) built in main()
 * (src/main.cpp:136-184) from a histogram made by construct_table()
 * (src/main.cpp:29-39).  Each entry point below names the reference interface
 * it replaces; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns an int status
 *     (MH_OK == 0, negative = error).  The reference's convention is
 *     eprintf + exit(1) (src/utils.cpp:62-65, src/coding.cpp:103-110); the
 *     C++ face in markov-huffman-coding_amd/host/ turns a non-zero status into
 *     exactly that.
 *   - the caller owns every buffer.  "mh_*" functions take HOST pointers and
 *     stage through HBM internally; "mh_dev_*" functions take DEVICE pointers
 *     plus a hipStream_t (as void*) and neither allocate nor synchronise,
 *     with the exceptions stated at their declarations: the model builders
 *     (mh_dev_model_from_counts allocates and synchronises once,
 *     mh_dev_model_from_counts_ws only synchronises once), mh_dev_build_index
 *     and mh_dev_status.
 *   - all compute runs in hand-written HIP kernels for gfx950.  There is no
 *     CPU fallback: without a usable GPU every compute call returns
 *     MH_ERR_NO_DEVICE.
 *   - an mh_model is immutable after construction and may be shared by threads.
 *   - bit order everywhere: MSB first inside a byte (src/bitbuffer.cpp:12).
 */
#ifndef MH_H
#define MH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_VERSION 100

enum {
    MH_OK = 0,
    MH_ERR_ARG = -1,           /* null/misaligned pointer, bad size or option            */
    MH_ERR_NO_DEVICE = -2,     /* no usable gfx950 device / HIP runtime                  */
    MH_ERR_HIP = -3,           /* a HIP call failed (mh_last_hip_error() has the code)   */
    MH_ERR_CORRUPT = -4,       /* stream not decodable (src/coding.cpp:103-106)          */
    MH_ERR_TYPE = -5,          /* stream/table type mismatch (src/coding.cpp:107-110)    */
    MH_ERR_BADTABLE = -6,      /* table file not parseable (src/huffman.cpp:166-172)     */
    MH_ERR_CODE_TOO_LONG = -7, /* a codeword exceeds 64 bits (not reachable < 2^44 B;
                                  never with a length-limited model)                   */
    MH_ERR_CAPACITY = -8,      /* output buffer or workspace too small                   */
    MH_ERR_TIMEOUT = -9,       /* bounded device-side wait expired (should not happen)   */
    MH_ERR_NOMEM = -10,
};

/* Initial context of every stream: the space character (src/main.cpp:32, src/coding.cpp:67,118). */
#define MH_PREV0 0x20

const char *mh_strerror(int status);
int mh_last_hip_error(void);
/* Diagnostic: how the calling thread's last mh_decode / mh_decode_to WITHOUT an index rebuilt it (codes of
 * mh_dev_index_path below). */
int mh_last_index_path(void);
/* Diagnostic: how many segments of the calling thread's last mh_encode* call the one-pass order-2 encoder gave up on
 * (MH_ERR_TIMEOUT: its bounded waits ran out, e.g. on a device shared with a long-running kernel) and that were encoded
 * again with the two-pass pair — the bytes are the same, the time is not, so the retry is counted, never silent.
 * 0 in normal operation.  mh_total_encode_retries: the same over all threads since the library was loaded. */
int mh_last_encode_retries(void);
uint64_t mh_total_encode_retries(void);
/* Number of usable devices; 0 when there is none (never an error). */
int mh_device_count(void);
/* Device used by the calling thread's subsequent mh_* / mh_dev_* calls (hipSetDevice). */
int mh_set_device(int ordinal);

/* Minimal device-memory helpers for hosts that have no HIP allocator of their own (the Python tests):
 * hipMalloc / hipFree / synchronous hipMemcpy. */
int mh_dev_malloc(void **d_ptr, size_t bytes);
int mh_dev_free(void *d_ptr);
int mh_dev_upload(void *d_dst, const void *h_src, size_t bytes);
int mh_dev_download(void *h_dst, const void *d_src, size_t bytes);

/* ------------------------------------------------------------------ model */

typedef struct mh_model mh_model;

/* Replaces huffman_table(int*) (src/huffman.h:14, src/huffman.cpp:18-20,131-164; order 0, 256 counts)
 * and markov_huffman_table(int*) (src/markov_huffman.h:12, src/markov_huffman.cpp:9-13; order 1,
 * counts[256*prev+sym], 65536 counts).  Tie-breaking reproduces min_pq (src/min_pq.tpp:4-52) and the
 * height swap (src/huffman.cpp:147-149) exactly; counts are 64-bit (reference: int).
 * order 2 (extension, described before the chunk-index section): 1 << 24 counts, needs a device.
 * Builds the code tables and decode LUTs (src/huffman.cpp:91-123) and uploads them to the current
 * device.  Host pointer in. */
int mh_model_from_counts(const uint64_t *counts, int order, mh_model **out);

/* Same, counts resident in HBM (e.g. straight out of mh_dev_histogram_o1 or an RCCL all-reduce).
 * Order 1: the per-context tree build (heap emulation), code derivation and table fill run in HIP
 * kernels on `stream` (mh_tree.hip); the counts never leave the device.  The call synchronises the
 * stream (16 KiB of table sizes come back so that the host can pick the decode-table layout); the host
 * copy of the trees that table files and the query calls below need is made lazily, on first use.
 * Order 0 (one tree) takes the host route. */
int mh_dev_model_from_counts(const uint64_t *d_counts, int order, void *stream, mh_model **out);
/* The same (order 1 only) with every device byte of the model placed in a caller workspace of at least
 * mh_dev_model_workspace(1) bytes (16-byte aligned): no allocation inside, and `stream` is synchronised
 * exactly once.  The model borrows the workspace: keep it alive, and do not rebuild into it, until the
 * model has been freed and the work that uses it has finished.  MH_ERR_CAPACITY when it is too small. */
size_t mh_dev_model_workspace(int order);
int mh_dev_model_from_counts_ws(const uint64_t *d_counts, int order, void *d_ws, size_t ws_bytes, void *stream, mh_model **out);

/* Length-limited models (extension): no code of the model is longer than `max_len` bits, at the smallest
 * possible cost in payload bits.  Per context: the reference tree is built as above; when its depth is <= max_len it is
 * kept unchanged, otherwise the whole context is re-coded with the lengths package-merge gives (leaves ordered by count,
 * then symbol; on equal weight a leaf precedes a package) and canonical codewords (order: length, then symbol; first
 * code all zero bits).  The result is an ordinary mh_model: every call takes it, its table file is a valid reference
 * table (the file stores the tree), and a model whose trees all fit the limit is the model of the unlimited call, byte
 * for byte.  With max_len <= 12 the encoders never take an escape route and the decoders' second level resolves every code.
 * max_len: 8..64, or 0 = no limit (exactly the unlimited call).  Order 0 and 1; order 2 and any other max_len:
 * MH_ERR_ARG, before a device is touched.  Package weights are sums of at most max_len context totals and are held in
 * 64 bits: a context that has to be re-coded and whose counts add up to 2^56 or more is refused with MH_ERR_ARG (not
 * handled in wider arithmetic).
 * The device calls follow their unlimited twins (order 0 takes the host route; _ws: order 1 only, no allocation, one
 * synchronisation).  The contexts over the limit are re-coded by one more kernel on `stream` (limit_recode_kernel, one wave
 * each, all state in LDS) that rewrites their part of the images in place: mh_dev_model_workspace(1) does not grow. */
int mh_model_from_counts_limited(const uint64_t *counts, int order, int max_len, mh_model **out);
int mh_dev_model_from_counts_limited(const uint64_t *d_counts, int order, int max_len, void *stream, mh_model **out);
int mh_dev_model_from_counts_limited_ws(const uint64_t *d_counts, int order, int max_len, void *d_ws, size_t ws_bytes, void *stream,
                                        mh_model **out);

/* Replaces the table-file constructors huffman_table(bitbuffer&) / markov_huffman_table(bitbuffer&)
 * (src/huffman.cpp:22-25,166-172; src/markov_huffman.cpp:15-25) and main()'s type sniffing on the
 * first bit (src/main.cpp:147-161).  `bytes` = whole table file. */
int mh_model_from_table_bits(const uint8_t *bytes, size_t n, mh_model **out);

/* Replaces write_coding_tree (src/markov_huffman.cpp:80-88, src/huffman.cpp:83-85,174-188) plus the
 * bitbuffer flush that pads to a byte (src/bitbuffer.cpp:170-180).  *nbytes = size needed/written. */
int mh_model_write_table(const mh_model *m, uint8_t *out, size_t cap, size_t *nbytes);

/* get_type() (src/coding.h:29-32): 0 simple Huffman, 1 Markov-Huffman. */
int mh_model_type(const mh_model *m);
/* Longest codeword in bits (0 for an all-empty model). */
int mh_model_max_code_len(const mh_model *m);
/* The shortest code of any context (0: a model without codes).  A payload of nbits bits holds at most nbits / min symbols:
 * the bound for index and fine-index capacities of a stream whose symbol count is not known (mh_dev_build_index_fine). */
int mh_model_min_code_len(const mh_model *m);
/* get_encoding(prev, c) (src/markov_huffman.cpp:52-54 -> src/huffman.cpp:71-73): *len bits,
 * *code right-aligned (valid when *len <= 64).  *len == 0: symbol has no code in this context. */
int mh_model_get_code(const mh_model *m, int prev, int sym, int *len, uint64_t *code);
/* decoding_lookup(prev, w) (src/markov_huffman.cpp:56-58 -> src/huffman.cpp:87-89): the 8-bit-window
 * LUT entry.  *present == 0 for a null entry (empty context). */
int mh_model_get_lut(const mh_model *m, int prev, int w, int *present, int *is_internal, int *value, int *depth);
/* How the decode tables of this model are laid out on the device: *primary_bits = width P of the
 * first-level window (8 = the reference's own 8-bit LUT, src/huffman.cpp:97-123; narrower when that
 * is what makes both table levels fit LDS), *secondary_entries = second-level entries,
 * *in_lds = 1 when both levels are LDS-resident in the decode kernel. */
int mh_model_decode_layout(const mh_model *m, int *primary_bits, int *secondary_entries, int *in_lds);
/* The same for the tile decoder's tables (mh_dev_decode_fine; LSB-first indexed): *primary_bits = width of the
 * LDS-resident first level (0: this model has no tile tables, mh_dev_decode_fine then runs the chunk decoder),
 * *secondary_bits = height of the uniform second-level tables, *secondary_entries = their total entry count (L2). */
int mh_model_tile_layout(const mh_model *m, int *primary_bits, int *secondary_bits, int *secondary_entries);
/* Diagnostic: copies one of the model's device images to the host (tests compare the host-built and the
 * device-built tables bit for bit).  which: 0 enc16, 1 len8, 2 len_slot, 3 code64, 4 decode prim,
 * 5 decode sec, 6 sec_base, 7 walk tree, 8 / 9 the tile decoder's first- / second-level tables (LSB-first
 * indexed, see mh_dev_decode_fine; empty when the model has none).  *bytes = image size; copied when cap suffices. */
int mh_model_image(const mh_model *m, int which, void *out, size_t cap, size_t *bytes);
void mh_model_free(mh_model *m);

/*
 * ORDER 2 — EXTENSION, PARITY UNPINNED.  order == 2 selects 65536 contexts, ctx = (byte before previous)
 * << 8 | previous byte (both ' ' before the stream): counts[ctx * 256 + sym], 1 << 24 entries.  The
 * reference implements order 1 only and merely speculates about higher orders (README.md:158-166), so
 * there is nothing to pin this against; the spec is the generalised oracle (oracle/mh_oracle.h): the same
 * per-context algorithm (src/huffman.cpp:131-164) per two-byte context.  Differences at the boundary:
 *   - mh_model_type() == 2; mh_model_get_code() takes the 16-bit context as `prev`; mh_model_get_lut() is
 *     not available; the model always lives on the device (there is no host-only order-2 model);
 *   - stream header 0x40 | unused bits (mh_stream_header / mh_stream_parse_header): the reference's magic
 *     is 0x30 (src/coding.cpp:103-106), so its decompress reports an order-2 stream as corrupt;
 *   - table file: the 33 bytes of an EMPTY order-1 table (which is what the reference's type sniffing,
 *     src/main.cpp:147-161, and loader make of it), the magic "MH2\x01", then per context bit 0 | bit 1 +
 *     tree (src/huffman.cpp:174-188), zero padded;
 *   - index entries carry the two context bytes in bits 48..63 (MH_INDEX2_BIT_MASK);
 *   - `prev0` arguments stand for BOTH context bytes.
 * All tables live in HBM and are served from L2 / the Infinity Cache (16.7 M codewords do not fit LDS).
 */
/* The order-2 model build in two steps, for ranks that share it: after a reduce-scatter of the 1 << 24
 * counts every rank holds the summed counts of its 65536 / G contexts, builds THEIR trees into a workspace of
 * mh_dev_model2_workspace() bytes (mh_dev_model2_build_slice; d_counts_slice = first count of context ctx_first), the
 * ranks all-gather the per-context arrays in place — mh_dev_model2_array(which, &offset, &bytes_per_context), which = 0..6:
 * a rank's share of array `which` is the byte range [offset + ctx_first * bytes_per_context, offset + ctx_end *
 * bytes_per_context) — and mh_dev_model2_finish derives every table from them (one stream synchronisation).  The model
 * borrows the workspace.  mh_dev_model_from_counts(order 2) is the same two steps over all contexts, in a ~600 MiB block of
 * its own; that block is kept when the model is freed and reused by the next order-2 build on the same device (a codec
 * that rebuilds its model per stream would otherwise allocate and free it every time). */
size_t mh_dev_model2_workspace(void);
int mh_dev_model2_array(int which, size_t *offset, size_t *bytes_per_context);
int mh_dev_model2_build_slice(const uint64_t *d_counts_slice, uint32_t ctx_first, uint32_t ctx_end,
                              void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_model2_finish(void *d_ws, size_t ws_bytes, void *stream, mh_model **out);
int mh_histogram_o2(const uint8_t *data, size_t n, uint64_t *counts /* 1 << 24 */);
int mh_dev_histogram_o2(const uint8_t *d_data, size_t n, uint16_t ctx0, uint64_t *d_counts /* 1 << 24 */, void *stream);
/* [r4] The same with a workspace (256-byte aligned, mh_dev_histogram_o2_workspace(n) bytes: 2 bytes per input byte, at
 * most 4 GiB, + 34 to 97 MiB of tables): sources with millions of live (context, symbol) keys — Zipf or uniform bytes — overflow the kernel's LDS tag
 * cache and would count at the rate of 64-bit global atomics (36 ms per GiB); with the workspace such a slab of the input is
 * partitioned by the context's high byte and every bucket counted in LDS like an order-1 histogram.  The choice is made on
 * the device per 2 GiB slab, from the cache misses of the slab's first 4 MiB; mh_dev_index_path(d_ws) afterwards says what
 * was chosen (bit 0: a slab stayed in the tag cache, bit 1: a slab was partitioned).  Without a workspace (or below 32 MiB) everything goes through the tag cache. */
size_t mh_dev_histogram_o2_workspace(size_t n);
int mh_dev_histogram_o2_ws(const uint8_t *d_data, size_t n, uint16_t ctx0, uint64_t *d_counts /* 1 << 24 */,
                           void *d_ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------- chunk index */
/*
 * The reference's stream has no index (src/coding.cpp:35-59), and a decoder's state is
 * (bit position, previous byte), so parallel decode needs an out-of-band index: one uint64 per chunk
 * of `chunk_symbols` input bytes,
 *        entry = (context byte at the chunk start << 56) | payload bit offset of the chunk start.
 * mh_encode / mh_dev_encode produce it; it never changes the payload bytes.  chunk_symbols must be a
 * power of two in [MH_CHUNK_MIN, MH_CHUNK_MAX].
 */
#define MH_CHUNK_MIN 256u
#define MH_CHUNK_MAX 8192u
#define MH_CHUNK_DEFAULT 1024u
#define MH_INDEX_BIT_MASK 0x00FFFFFFFFFFFFFFull
/* order-2 models (extension below): entry = (two context bytes << 48) | bit offset */
#define MH_INDEX2_BIT_MASK 0x0000FFFFFFFFFFFFull
static inline uint64_t mh_index_entries(uint64_t n_symbols, uint32_t chunk_symbols) {
    return (n_symbols + chunk_symbols - 1) / chunk_symbols;
}

/* ------------------------------------------------------- host-buffer calls */

/* Replaces construct_table + the order-1 lambda (src/main.cpp:29-39,173-181): counts[256*prev+c]++,
 * prev starting at prev0.  counts: 65536 entries, overwritten. */
int mh_histogram_o1(const uint8_t *data, size_t n, uint8_t prev0, uint64_t *counts);
/* Replaces construct_table + the order-0 lambda (src/main.cpp:164-171).  counts: 256 entries. */
int mh_histogram_o0(const uint8_t *data, size_t n, uint64_t *counts);

/* Option for two-pass callers (histogram, then encode, of the SAME host buffer — what the CLI does,
 * src/main.cpp:173-183 + 204-212): when on, mh_histogram_o0/o1/o2 leave their upload of the input in HBM
 * (if it fits beside everything else) and the next mh_encode of that buffer — same pointer, size and
 * sampled content — reads it there, so the data crosses PCIe once.  The caller promises not to modify the
 * buffer between the two calls.  Off by default; turning it off frees what is held. */
int mh_set_input_residency(int on);

/* Replaces the body of i_coding_provider::compress (src/coding.cpp:61-94) between the header
 * placeholder and the header rewrite: payload bits only.  *nbits = payload length in bits; payload
 * bytes written = ceil(*nbits / 8), zero padded (src/bitbuffer.cpp:175).  cap must be >=
 * mh_encode_bound(n).  index/chunk_symbols optional (index == NULL: none). */
int mh_encode(const mh_model *m, const uint8_t *data, size_t n, uint8_t prev0,
              uint8_t *out_payload, size_t cap, uint64_t *nbits,
              uint64_t *index, uint32_t chunk_symbols);
/* Worst-case payload bytes for n input bytes under model m (n * max_code_len bits, rounded up, + slack). */
size_t mh_encode_bound(const mh_model *m, size_t n);
/* The header byte of src/coding.cpp:88: 0x30 | (~type & 1) << 3 | (8 - nbits % 8) % 8. */
uint8_t mh_stream_header(const mh_model *m, uint64_t nbits);
/* Validates a header byte as src/coding.cpp:100-116 does and returns the payload length in bits for a
 * file of file_bytes bytes: MH_ERR_CORRUPT on bad magic, MH_ERR_TYPE on a table/stream mismatch. */
int mh_stream_parse_header(const mh_model *m, uint8_t header, uint64_t file_bytes, uint64_t *nbits);

/* Replaces the loop of i_coding_provider::decompress (src/coding.cpp:118-157): decode exactly `nbits`
 * payload bits.  With an index (from mh_encode) chunks decode in parallel and n_symbols must be the
 * original length; with index == NULL (a stream produced by the reference) a device-side
 * index-building pass runs first and n_symbols is ignored.  *nbytes = decoded size (written if cap
 * suffices, else MH_ERR_CAPACITY with *nbytes set). */
int mh_decode(const mh_model *m, const uint8_t *payload, uint64_t nbits, uint8_t prev0,
              uint8_t *out, size_t cap, size_t *nbytes,
              const uint64_t *index, uint32_t chunk_symbols, uint64_t n_symbols);

/* Device footprint of the host-buffer calls: bounded by the segment size (256 MiB, MH_SEGMENT_BYTES) for
 * mh_histogram_*, mh_encode and mh_decode WITH an index.  mh_decode / mh_decode_to WITHOUT an index are the
 * exception: the whole payload is uploaded, an index of nbits / chunk_symbols + 2 entries is rebuilt beside it,
 * and the index builder's workspace takes about 28 bytes per 512 bytes of payload — roughly 1.1 x the payload
 * in total, plus one output segment. */
/* mh_decode for callers that cannot know the output size beforehand (a stream without an index):
 * get_out(ctx, n) is called exactly once, when the symbol count n is known, and returns where the n
 * bytes go (NULL -> MH_ERR_CAPACITY).  The CLI maps its output file there. */
typedef uint8_t *(*mh_output_fn)(void *ctx, size_t n);
int mh_decode_to(const mh_model *m, const uint8_t *payload, uint64_t nbits, uint8_t prev0,
                 mh_output_fn get_out, void *ctx, size_t *nbytes,
                 const uint64_t *index, uint32_t chunk_symbols, uint64_t n_symbols);

/* Payload bits this model produces for data with the given histogram (host counts: 65536 entries for a
 * Markov model, 256 for a Huffman model): the exact size of the compressed file before encoding. */
int mh_model_payload_bits(const mh_model *m, const uint64_t *counts, uint64_t *nbits);

/* ------------------------------------------------------------ device calls */
/* Device pointers, stream-ordered, no allocation, no synchronisation.  d_data / d_payload / d_out must
 * be 16-byte aligned.  Workspaces: query the size, allocate once, reuse. */

/* Optional workspace of mh_dev_histogram_o1 (pass NULL, 0 to do without): with it the workgroups'
 * counters leave as plain stores and are summed by a second kernel instead of 16.7 M device-scope
 * atomics, ~0.5 ms less per call.  A workspace of the full size (16-byte aligned) also keeps what
 * mh_dev_encode_hist needs: every workgroup counts one contiguous region of the input and leaves that
 * region's own pair counts behind. */
size_t mh_dev_histogram_workspace(size_t n);
/* d_counts (65536 or 256 x uint64) is overwritten.  With a workspace (>= 256 bytes) the order-1 call also checks
 * on the device that the counts add up to n (src/main.cpp:176-178: the reference's counts sum to the file size; a
 * spilled LDS counter field or a lost fix-up cannot hide): mh_dev_status(d_ws) then reports MH_ERR_CORRUPT. */
int mh_dev_histogram_o1(const uint8_t *d_data, size_t n, uint8_t prev0, uint64_t *d_counts,
                        void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_histogram_o0(const uint8_t *d_data, size_t n, uint64_t *d_counts,
                        void *d_ws, size_t ws_bytes, void *stream);

/* (large enough for the encoder to take a region-mode histogram of the input by itself when the call comes without
 * one: mh_dev_encode, mh_dev_encode_at and mh_encode then run the same fast encoder as mh_dev_encode_hist) */
size_t mh_dev_encode_workspace(size_t n);
/* d_nbits: one uint64 (payload bits).  d_index: mh_index_entries(n, chunk_symbols) entries or NULL.
 * Errors found on the device (capacity overrun) go to the int32 at the start of d_ws: mh_dev_status(). */
int mh_dev_encode(const mh_model *m, const uint8_t *d_data, size_t n, uint8_t prev0,
                  uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                  uint64_t *d_index, uint32_t chunk_symbols,
                  void *d_ws, size_t ws_bytes, void *stream);

/* mh_dev_encode_at for the compress path, where a histogram of the SAME device buffer was taken just before
 * (src/main.cpp:173-183, then 204-212): d_hist_ws / hist_ws_bytes is the workspace mh_dev_histogram_o1
 * filled for (d_data, n, prev0), untouched since.  The encoder then prices each of the histogram's regions from
 * its pair counts and the code lengths and needs no pass of its own over the input to find where everything
 * goes: the input is read once.  Same payload, index and *d_nbits as mh_dev_encode_at.  Falls back to
 * mh_dev_encode_at by itself for order-2 models or a workspace that is too small (codes over 12 bits are handled
 * inside: src/bitbuffer.cpp:45-73 appends descriptors of any length).  A workspace that holds some other buffer's
 * histogram is reported as MH_ERR_CORRUPT by mh_dev_status(d_ws) and nothing is written.  d_data itself must be
 * unchanged too: if the buffer was refilled between the two calls, the header still matches, the regions are priced
 * from the old contents, and what is written (never beyond `cap`) is not a valid stream — every region compares
 * the bits it emitted with its price and mh_dev_status(d_ws) reports MH_ERR_CORRUPT. */
int mh_dev_encode_hist(const mh_model *m, const uint8_t *d_data, size_t n, uint8_t prev0,
                       const uint64_t *d_start_bit,
                       uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                       uint64_t *d_index, uint32_t chunk_symbols,
                       const void *d_hist_ws, size_t hist_ws_bytes,
                       void *d_ws, size_t ws_bytes, void *stream);

/* Sharded encode (contiguous byte ranges, one rank per shard).  A shard's payload length
 * is known before it is encoded: it is the dot product of the shard's LOCAL histogram with the code
 * lengths of the (global) model.  d_counts: 65536 (order 1) or 256 (order 0) uint64 counts on the
 * device; *d_nbits receives the bits. */
int mh_dev_payload_bits(const mh_model *m, const uint64_t *d_counts, uint64_t *d_nbits, void *stream);
/* mh_dev_encode with the payload emitted pre-shifted: *d_start_bit (device memory, may be NULL = 0) is
 * the global bit position at which this shard starts; its first code is written at bit
 * (*d_start_bit & 7) of d_payload[0], the bits before it are zero, so consecutive shards concatenate at
 * byte offset start_bit / 8 with ONE OR-merged seam byte.  *d_nbits = (*d_start_bit & 7) + payload bits,
 * i.e. the end position inside d_payload; index entries are positions inside d_payload as well, so the
 * shard decodes from its own buffer with mh_dev_decode(nbits = *d_nbits). */
int mh_dev_encode_at(const mh_model *m, const uint8_t *d_data, size_t n, uint8_t prev0,
                     const uint64_t *d_start_bit,
                     uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                     uint64_t *d_index, uint32_t chunk_symbols,
                     void *d_ws, size_t ws_bytes, void *stream);

/* mh_dev_encode_at with the full start context of the shard: the previous byte (order 0/1 models, ctx0 < 256) or,
 * for an order-2 model, (byte before previous) << 8 | previous byte — a shard of an order-2 stream starts in
 * the context of the last TWO bytes of the shard before it. */
int mh_dev_encode_ctx(const mh_model *m, const uint8_t *d_data, size_t n, uint32_t ctx0,
                      const uint64_t *d_start_bit,
                      uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                      uint64_t *d_index, uint32_t chunk_symbols,
                      void *d_ws, size_t ws_bytes, void *stream);

/* 64-byte status block + one uint32 per chunk (list of the chunks whose codes exceed the decode
 * tables and are decoded by a second launch); 0 for an invalid chunk size. */
size_t mh_dev_decode_workspace(uint64_t nbits, uint64_t n_symbols, uint32_t chunk_symbols);
/* Parallel decode with an index.  ws_bytes must be at least mh_dev_decode_workspace(...) (MH_ERR_ARG).
 * d_payload and d_out are 16-byte aligned; the kernel reads the payload in aligned 32- or 64-byte pieces,
 * so d_payload must be readable up to the next 64-byte boundary after its last byte (any hipMalloc'ed
 * buffer is).  Errors found on the device (null LUT entry, walk past the end)
 * are reported through the int32 at the start of the workspace: mh_dev_status() reads it. */
int mh_dev_decode(const mh_model *m, const uint8_t *d_payload, uint64_t nbits,
                  uint8_t *d_out, uint64_t n_symbols,
                  const uint64_t *d_index, uint32_t chunk_symbols,
                  void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_decode for a payload whose length is still on the device (e.g. straight after mh_dev_encode, with
 * no host round trip in between): the kernels read *d_nbits.  nbits_hint (0 = unknown) only steers the
 * choice between kernel variants; results never depend on it. */
int mh_dev_decode_dn(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_nbits, uint64_t nbits_hint,
                     uint8_t *d_out, uint64_t n_symbols,
                     const uint64_t *d_index, uint32_t chunk_symbols,
                     void *d_ws, size_t ws_bytes, void *stream);
/*
 * FINE INDEX — a device-only acceleration structure of the decoder, never part of the stream or of the sidecar
 * index: one uint32 per MH_FINE_SYMBOLS = 64 input bytes,
 *        entry = context byte at that byte << 24 | (payload bit offset of its code & 0xFFFFFF);
 * the chunk index entry in front of it supplies the offset's high bits.  With it one wave decodes 64 adjacent
 * 64-symbol pieces: its compressed input and its output are each one contiguous run of memory (mh_tile.hip)
 * instead of 64 scattered cache lines per access.  It costs 1/16 of the input size in HBM, is written by
 * mh_dev_encode_fine alongside the payload (or by mh_dev_build_index_fine for a stream that came without any
 * index) and is consumed by mh_dev_decode_fine; it lives and dies in device memory.  chunk_symbols <= 4096 for the
 * decoder to use it.  Order-2 models (extension): entry = two context bytes << 16 | bits from the chunk's index entry
 * to the piece (0xFFFF: does not fit), chunk_symbols <= 1024, and only models whose live contexts all have a slot in
 * the decoder's LDS tables (text-like sources: a few hundred contexts) use it; mh_dev_build_index_fine writes none.  The
 * order-2 range calls (mh_dev_decode_ranges_o2) consume the order-2 form for any order-2 model, as work units of
 * MH_FINE_SYMBOLS symbols; a piece whose entry is 0xFFFF is decoded from an earlier piece of its chunk.
 */
#ifndef MH_T_SUB_SHIFT            /* (an experimental build may halve the piece: csrc/Makefile, MH_T_SUB_SHIFT=5) */
#define MH_T_SUB_SHIFT 6
#endif
#define MH_FINE_SYMBOLS (1u << MH_T_SUB_SHIFT)
static inline uint64_t mh_fine_entries(uint64_t n_symbols) { return (n_symbols + MH_FINE_SYMBOLS - 1) / MH_FINE_SYMBOLS; }
/* mh_dev_encode_hist (d_hist_ws may be NULL: then mh_dev_encode_at) that also fills d_fine[mh_fine_entries(n)]
 * (d_fine may be NULL).  Payload, index and *d_nbits do not depend on d_fine. */
int mh_dev_encode_fine(const mh_model *m, const uint8_t *d_data, size_t n, uint8_t prev0,
                       const uint64_t *d_start_bit,
                       uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                       uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_fine,
                       const void *d_hist_ws, size_t hist_ws_bytes,
                       void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_encode_ctx (full start context: two bytes for an order-2 model) that also fills d_fine. */
int mh_dev_encode_ctx_fine(const mh_model *m, const uint8_t *d_data, size_t n, uint32_t ctx0,
                           const uint64_t *d_start_bit,
                           uint8_t *d_payload, size_t cap, uint64_t *d_nbits,
                           uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_fine,
                           void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_decode / mh_dev_decode_dn (d_nbits != NULL: the payload length is read there, nbits is a hint) with the
 * fine index of the same stream.  d_fine == NULL, a model without tile tables, chunk_symbols > 4096 or a small
 * stream: exactly mh_dev_decode.  Same output either way; same workspace size. */
int mh_dev_decode_fine(const mh_model *m, const uint8_t *d_payload, uint64_t nbits, const uint64_t *d_nbits,
                       uint8_t *d_out, uint64_t n_symbols,
                       const uint64_t *d_index, uint32_t chunk_symbols, const uint32_t *d_fine,
                       void *d_ws, size_t ws_bytes, void *stream);

/* Index building for a stream without one (what the reference writes: src/coding.cpp:35-59 has no
 * index): parallel fixed-point iteration over 512-byte bit segments — each segment is decoded from a
 * guessed state and re-decoded while its predecessor's end state changes; Huffman streams
 * re-synchronise, so a few passes converge, and a sequential pass is the fallback.  Fills d_index
 * (capacity index_cap entries) and *d_n_symbols.  Unlike the other device calls this one synchronises
 * `stream` between batches of passes (the pass count depends on the data). */
size_t mh_dev_build_index_workspace(uint64_t nbits);
int mh_dev_build_index(const mh_model *m, const uint8_t *d_payload, uint64_t nbits, uint8_t prev0,
                       uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols,
                       uint64_t *d_n_symbols, void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_build_index that also fills the fine index (see above) of the stream: d_fine[fine_cap], one entry per 64
 * symbols (nbits / 64 + 2 entries always suffice: a code has at least one bit).  Synchronises `stream` as mh_dev_build_index
 * does. */
int mh_dev_build_index_fine(const mh_model *m, const uint8_t *d_payload, uint64_t nbits, uint8_t prev0,
                            uint64_t *d_index, uint64_t index_cap, uint32_t chunk_symbols,
                            uint32_t *d_fine, uint64_t fine_cap,
                            uint64_t *d_n_symbols, void *d_ws, size_t ws_bytes, void *stream);
/*
 * STREAMS WITHOUT AN INDEX IN TWO PASSES OVER THE PAYLOAD (round 5) — what i_coding_provider::decompress is handed
 * (src/coding.cpp:96-160: a `.cm` carries nothing but the header byte and the bits).  Building both indices and then decoding
 * reads the payload three times; these two calls read it twice and write no index at all:
 *   mh_dev_decode_stream_states  pass 1: the payload is cut into 352-bit segments, every segment is decoded from a guessed
 *       state after a short warm-up, the segments whose guess was wrong are decoded again from their predecessor's end state
 *       until none is left (the fixed point of mh_dev_build_index), a prefix sum of the segments' symbol counts gives every
 *       segment its output offset; *d_n_symbols = the decoded size.  Synchronises `stream` between its passes.
 *       mh_dev_index_path(d_ws) afterwards: 6 = the workspace holds the states, mh_dev_decode_stream_emit may follow;
 *       0 = this model / stream does not take this path (an order-2 model, no tile tables, a code-length lattice, under a
 *       megabit, or segments that do not synchronise): build an index
 *       (mh_dev_build_index_fine) and decode from it instead.
 *   mh_dev_decode_stream_emit    pass 2: every segment is decoded once more from its true state and its bytes are written
 *       to d_out[offset of its first symbol ...); nothing is written at or beyond out_cap (MH_ERR_CAPACITY via mh_dev_status).
 *       End state and count of every segment must come out as converged and the stream must end exactly at nbits
 *       (src/coding.cpp:124,158): MH_ERR_CORRUPT otherwise.  Segments that hold a code longer than the tile tables resolve
 *       take the path too: the emit pass walks them one lane each, the stream's last segment included.  No allocation; synchronises `stream` once, before its launch (it
 *       reads the workspace's path word: MH_ERR_ARG when the workspace does not hold the states of this stream).
 * Workspace for both: mh_dev_build_index_workspace(nbits), the same buffer, untouched in between.
 */
int mh_dev_decode_stream_states(const mh_model *m, const uint8_t *d_payload, uint64_t nbits, uint8_t prev0,
                                uint64_t *d_n_symbols, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_decode_stream_emit(const mh_model *m, const uint8_t *d_payload, uint64_t nbits, uint8_t prev0,
                              uint8_t *d_out, uint64_t out_cap, void *d_ws, size_t ws_bytes, void *stream);
/* Diagnostic: how the last mh_dev_build_index on this workspace arrived at the index — 1 the segment iteration
 * converged, 2 per-group context maps (fixed-length codes), 3 per-group state maps (mixed lengths), 4 the one-lane
 * walk, 5 the tile decoder's segment states (the fast path: a model with tile tables, a stream of a megabit or more), 0 nothing
 * ran.  Synchronises `stream`. */
int mh_dev_index_path(const void *d_ws, void *stream);
/* Diagnostic: which encoder the last mh_dev_encode* call on this workspace ran — 1 the region encoder (priced from a
 * histogram of the input, one read), 3 the same with its escape variant launched too (model with codes over 12
 * bits), 2 the length pass + emit pair (inputs under 4 MiB without a histogram; order-2 models whose live contexts
 * do not fit the LDS image, or MH_ENCODE2_PATH=two_pass), 4 the one-pass order-2 encoder (enc_chain_kernel: every
 * symbol looked up once, start bits by a chained scan over groups of wave-tiles that are handed out by a ticket counter,
 * so a wait is only ever for a workgroup that is running).  Synchronises.
 * Every wait of the one-pass encoder is bounded; should one run out all the same, the workspace's status is
 * MH_ERR_TIMEOUT (nothing valid was written): mh_encode* retry with the pair by themselves, a caller of mh_dev_encode*
 * runs again with MH_ENCODE2_PATH=two_pass. */
int mh_dev_encode_path(const void *d_ws, void *stream);
/* Diagnostic: which decoder the last mh_dev_decode* call on this workspace ran — 1 the tile decoder (fine index given, 8 MiB
 * or more, average code shorter than the tile tables' first level), 2 the chunk decoder.  Synchronises. */
int mh_dev_decode_path(const void *d_ws, void *stream);
/* Diagnostic: which instantiation of the chunk decoder that call launched (csrc/mh_decode.hip, dec_cfg) — chosen from the
 * model's table layout and the stream's ratio, never from the environment:
 *   0 LDS_WIDE          both table levels in LDS, no code over 8 bits, ratio over 0.6: two streams, 64-byte granules and bursts
 *   1 LDS_SHORT         the same model on a better-compressed stream: four light streams
 *   2 LDS_TWO_LEVEL     both levels in LDS, first level narrower than 8 bits;   3 LDS_TWO_LEVEL_P8   ... of 8 bits
 *   4 L2_DIRECT         first level in LDS, uniform second-level tables of 2^H entries in L2, H read from the model;
 *   5 / 6 / 7 / 8       ... with H = 2 / 3 / 4 / 8 as a compile-time constant (longest code 10 / 11 / 12 / 16 or more bits)
 * -1: the chunk decoder did not run on this workspace (the tile decoder did).  The redo pass behind it (codes longer than
 * both levels, ragged ends: one lane per chunk, tree walk) uses variant 9 REDO_LDS or 10 REDO_L2_DIRECT of the same layout.
 * Synchronises. */
int mh_dev_decode_variant(const void *d_ws, void *stream);
/* Synchronises `stream` and returns the device-side status word of a workspace (MH_OK, MH_ERR_CORRUPT,
 * MH_ERR_TIMEOUT, MH_ERR_CAPACITY). */
int mh_dev_status(const void *d_ws, void *stream);

/* ------------------------------------------------ batches of independent streams */
/*
 * BATCHES OF INDEPENDENT STREAMS — many small messages (log lines, records, packets) under ONE shared model, in a fixed
 * number of launches instead of several launches and host waits per message: the reference's own remedy for the table
 * overhead of small files (README.md:152-157; its CLI: `markovhuffman msg -e shared.e -o msg.cm`).  Order 0 and order 1
 * models; an order-2 model is refused with MH_ERR_ARG.
 *   - Stream i is bytes [in_off[i], in_off[i+1]) of one buffer; in_off has n_streams + 1 entries, in_off[0] == 0,
 *     non-decreasing, in_off[n] == total.  Empty streams may appear anywhere, n_streams == 0 is valid.  The device calls
 *     take n_streams and total as host values (grids are sized without a synchronisation) and check the offsets on the
 *     device: MH_ERR_ARG through mh_dev_status(d_ws).  The host calls check them before touching a device.
 *   - Every stream starts in context prev0 (MH_PREV0 for the reference, src/coding.cpp:67,118).  Its payload bits, nbits and
 *     chunk index are what mh_encode produces for that message alone, so mh_stream_header + payload is the `.cm` file the
 *     reference writes for it with the shared table — including the reference's NDEBUG behaviour for a pair without a code
 *     (the symbol is skipped, the context still advances).
 *   - Payloads are packed byte-aligned, back to back: out_off[n + 1] = exclusive scan of ceil(nbits_i / 8).
 *   - Chunk index (optional, chunk_symbols under the chunk-index rules): stream i's entries start at
 *     mh_batch_index_base(in_off[i], i, chunk) = in_off[i] / chunk + i, capacity mh_batch_index_capacity(total, n, chunk)
 *     = total / chunk + n + 1 entries.  The slices never overlap: ceil(m / c) <= floor((a + m) / c) - floor(a / c) + 1.
 *     Each slice equals mh_encode's index of that message (context in bits 56..63, bit offsets relative to the stream's own
 *     payload); entries in the gaps between slices are left untouched.  (Exported functions rather than static inlines:
 *     every name this header declares is a symbol of the library.)
 */
uint64_t mh_batch_index_base(uint64_t in_off, uint64_t stream, uint32_t chunk_symbols);
uint64_t mh_batch_index_capacity(uint64_t total, uint64_t n_streams, uint32_t chunk_symbols);

/* Training histogram of a shared model: the summed counts of all streams, each starting in context prev0 (the order-1
 * histogram of the concatenation, then one fix-up per stream boundary: counts[last byte of the previous stream][first
 * byte] moves to counts[prev0][first byte]).  d_ws: at least mh_dev_histogram_batch_workspace(total) bytes (>= 256,
 * 16-byte aligned; its status word carries MH_ERR_ARG for bad offsets and the order-1 conservation check). */
size_t mh_dev_histogram_batch_workspace(size_t total);
int mh_dev_histogram_o1_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                              uint64_t *d_counts /* 65536 */, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_histogram_o0_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total,
                              uint64_t *d_counts /* 256 */, void *d_ws, size_t ws_bytes, void *stream);

/* Worst-case packed payload bytes of a batch: total * max_code_len bits, one partial byte per stream, + slack. */
size_t mh_encode_batch_bound(const mh_model *m, size_t total, size_t n_streams);
size_t mh_dev_encode_batch_workspace(size_t n_streams, size_t total);
/* Writes d_out_off[n + 1], d_nbits[n], the packed payloads (d_payload 16-byte aligned) and, when d_index != NULL, the index
 * slices.  Payloads that do not fit `cap`: MH_ERR_CAPACITY through mh_dev_status(d_ws), nothing written beyond cap (the
 * offsets and lengths are still written).  The input may start anywhere (no alignment needed for d_data). */
int mh_dev_encode_batch(const mh_model *m, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total,
                        uint8_t prev0, uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits,
                        uint64_t *d_index, uint32_t chunk_symbols, void *d_ws, size_t ws_bytes, void *stream);

/* Index-free batch decode walks each stream with one lane, from its first bit to its last: a stream longer than this is
 * refused by the device call (its status is MH_ERR_ARG; the others still decode), because one lane would take the whole
 * batch's time on it — 8 Mbit already take milliseconds at one lane's rate.  mh_decode_batch decodes such streams with
 * mh_decode by itself, so the host call never refuses a valid batch. */
#define MH_BATCH_WALK_MAX_BITS (1ull << 23)
size_t mh_dev_decode_batch_workspace(size_t n_streams);
/* Decodes stream i (payload bytes [d_pay_off[i], d_pay_off[i+1]), d_nbits[i] bits, pay_total = pay_off[n]) into d_out.
 * d_payload and d_out 16-byte aligned; reads stay inside the aligned dwords that hold a stream's payload.
 *   - with d_index (chunk_symbols, the layout above): d_sym_off[n + 1] is INPUT (the d_in_off of the encode), sym_total its
 *     last entry as a host value (<= out_cap, else MH_ERR_CAPACITY).  One lane per (stream, chunk); every chunk must end
 *     exactly at the next entry's offset (the last one at nbits_i), else that stream is MH_ERR_CORRUPT.
 *   - without (streams the reference wrote): d_sym_off[n + 1] is OUTPUT; a count pass decodes every stream without writing
 *     and checks that it ends exactly at nbits_i (src/coding.cpp:124,158), a scan gives the offsets, an emit pass writes the
 *     bytes — nothing at or beyond out_cap (the stream that does not fit: MH_ERR_CAPACITY).  A stream that the count pass
 *     refuses or finds corrupt takes 0 symbols in d_sym_off and writes no byte; the streams behind it move up.
 * d_stream_status[n] (may be NULL): MH_OK or the stream's error (MH_ERR_CORRUPT, MH_ERR_ARG: nbits_i beyond its payload
 * bytes or over MH_BATCH_WALK_MAX_BITS, MH_ERR_CAPACITY).  mh_dev_status(d_ws): the first error found. */
int mh_dev_decode_batch(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                        size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                        uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                        int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);

/* Host-buffer forms: the whole batch is uploaded and the device call runs once.  Device footprint of mh_encode_batch:
 * total + min(cap, mh_encode_batch_bound) + 24 bytes per stream + the index + the workspace (about 8 bytes per KiB of
 * input and per stream); of mh_decode_batch: the payloads + the output (index-free: at most nbits / shortest code per
 * stream) + 28 bytes per stream + the index.  `cap` / `out_cap` are the caller's buffer sizes; `index` (when not NULL)
 * has mh_batch_index_capacity entries, and entries between slices keep their values.  mh_decode_batch: sym_off is input
 * with an index, output without; stream_status (may be NULL) as above; returns the first stream's error, if any. */
int mh_encode_batch(const mh_model *m, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                    uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols);
int mh_decode_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                    uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                    int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * BATCHES OF ORDER-2 STREAMS — the batch section above for ONE shared order-2 model (extension, parity unpinned): the
 * 65 536-context table is written once for the whole corpus, and every message gets the order-2 payload.  The calls of that
 * section keep refusing an order-2 model; these refuse any other (MH_ERR_ARG).  Everything not said here is word for word
 * the section above: in_off[n + 1] and its checks (host calls on the host, device calls through mh_dev_status(d_ws)),
 * packed byte-aligned payloads with out_off[n + 1], nbits[n], index slices at mh_batch_index_base(in_off[i], i, chunk),
 * MH_BATCH_WALK_MAX_BITS, d_stream_status, the host forms' footprints.
 *   - Every stream starts in context (prev0, prev0), as mh_encode starts an order-2 stream: stream i's
 *     mh_stream_header(m, nbits_i) followed by its payload is what mh_encode writes for that message alone — including the
 *     skip rule for a pair without a code (the symbol is skipped, the context still advances).
 *   - Index entries are order-2 entries: (two context bytes) << 48 | bit offset relative to the stream's own payload, equal
 *     to mh_encode's index of that message.
 *   - mh_encode_batch_bound serves this family too (it works from the model's longest code).
 * --------------------------------------------------------------------------------------------------------------------- */
/* Training histogram of a shared order-2 model: the summed 1 << 24 order-2 counts of all streams, stream i's first symbol
 * counted in context (prev0, prev0), its second in (prev0, its first byte).  d_ws: at least
 * mh_dev_histogram_o2_batch_workspace(total) bytes, 256-byte aligned; its status word carries MH_ERR_ARG for bad offsets
 * and the order-2 conservation check (the counts add up to total).  Needs no model. */
size_t mh_dev_histogram_o2_batch_workspace(size_t total);
int mh_dev_histogram_o2_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint8_t prev0,
                              uint64_t *d_counts /* 1 << 24 */, void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_encode_batch for an order-2 model (arguments, outputs and capacity rule alike). */
size_t mh_dev_encode_batch_o2_workspace(size_t n_streams, size_t total);
int mh_dev_encode_batch_o2(const mh_model *m, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total,
                           uint8_t prev0, uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits,
                           uint64_t *d_index, uint32_t chunk_symbols, void *d_ws, size_t ws_bytes, void *stream);
/* mh_dev_decode_batch for an order-2 model: indexed (every chunk must end exactly at the next entry) or index-free (count
 * pass, scan, emit pass; a stream must end exactly at nbits_i; streams over MH_BATCH_WALK_MAX_BITS get MH_ERR_ARG). */
size_t mh_dev_decode_batch_o2_workspace(size_t n_streams);
int mh_dev_decode_batch_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                           size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                           uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                           int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
/* Host-buffer forms, as mh_encode_batch / mh_decode_batch: streams over the walk cap are decoded by mh_decode by themselves,
 * so a valid batch is never refused. */
int mh_encode_batch_o2(const mh_model *m, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                       uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols);
int mh_decode_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                       uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                       int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * BATCHES OF STREAMS, ONE MODEL EACH — the reference's default per-file flow (`markovhuffman f -o f.cm -d f.e`: train a
 * model on the file, write its table next to its payload) for many messages at once.  Order 0 and order 1; order 2 is
 * refused with MH_ERR_ARG.  Stream i, in_off, prev0, payload packing and the chunk-index slices are exactly as in the
 * batch section above.  For every stream each output equals what the single-stream calls give for that message alone
 * (mh_histogram_o1(m, prev0) or mh_histogram_o0, mh_model_from_counts, then mh_model_write_table and mh_encode): its
 * table file (an empty order-1 stream: the 33-byte all-empty table; an empty order-0 stream: 0 bytes), its payload and
 * nbits (mh_stream_header + payload is its `.cm` / `.ch`), its index slice.
 *
 * An mh_model_set holds one model per stream on the device: per stream a 256-entry context -> slot map, per live
 * context (order 1: prev0 and the distinct bytes before the stream's last one) one slot of 3 840 bytes with the
 * encoder's codes, the reference's 8-bit first decode level and a walk tree for longer codes.  A set takes about
 * 1 KiB per stream plus 3.8 KiB per live context of device memory.  Codes are at most 64 bits: a tree deeper than that
 * needs Fibonacci-weighted counts, which take more than 2^40 bytes of input; MH_ERR_CODE_TOO_LONG if it is ever met.
 * A set is immutable after construction and may be shared by threads.
 * --------------------------------------------------------------------------------------------------------------------- */
typedef struct mh_model_set mh_model_set;

/* Trains one model per stream on the device: live contexts, per-stream histograms, one tree per (stream, live context)
 * with the reference's tie-breaking.  Allocates the set (and, for the duration of the call, 3.1 KiB of tree nodes per
 * live context), and synchronises `stream` twice: once to size the set (its live-context count), once at the end for the
 * status.  d_data needs no alignment; d_ws: at least
 * mh_dev_model_set_train_workspace(n_streams) bytes, 16-byte aligned.  Bad offsets: MH_ERR_ARG. */
size_t mh_dev_model_set_train_workspace(size_t n_streams);
int mh_dev_model_set_train(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, int order, uint8_t prev0,
                           void *d_ws, size_t ws_bytes, void *stream, mh_model_set **out);
/* A set from host models (order 0/1, mixed orders allowed): stream i is coded under models[i]. */
int mh_model_set_from_models(const mh_model *const *models, size_t n_streams, mh_model_set **out);
/* A set from table files: stream i's table is bytes [tab_off[i], tab_off[i+1]) of `tables` (a 0-byte table is the
 * empty order-0 model of an empty stream).  A malformed table: MH_ERR_BADTABLE. */
int mh_model_set_from_tables(const uint8_t *tables, const uint64_t *tab_off, size_t n_streams, mh_model_set **out);
void mh_model_set_free(mh_model_set *s);
size_t mh_model_set_size(const mh_model_set *s);          /* streams */
size_t mh_model_set_slots(const mh_model_set *s);         /* live contexts over all streams */
/* Stream i's model: its type (0 or 1) and longest code (0: no code).  Reads the device (synchronous). */
int mh_model_set_stream_info(const mh_model_set *s, size_t i, int *type, int *max_code_len);
/* Longest and shortest code of any stream of the set (0: no codes at all). */
int mh_model_set_code_lens(const mh_model_set *s, int *max_code_len, int *min_code_len);

/* Every stream's table file, packed back to back (no alignment between them): d_tab_off[n + 1] (written).  Table sizes are
 * computed on the device; they never exceed mh_model_set_tables_bound(s) bytes in all.  Tables that do not fit cap:
 * MH_ERR_CAPACITY through mh_dev_status(d_ws), nothing written at or beyond cap.  d_out and d_ws 16-byte aligned. */
size_t mh_model_set_tables_bound(const mh_model_set *s);
size_t mh_dev_model_set_tables_workspace(const mh_model_set *s);
int mh_dev_model_set_tables(const mh_model_set *s, uint8_t *d_out, size_t cap, uint64_t *d_tab_off, void *d_ws, size_t ws_bytes, void *stream);

/* mh_dev_encode_batch / mh_dev_decode_batch with stream i under the set's model i (n_streams == mh_model_set_size(s), else
 * MH_ERR_ARG).  Same layouts, checks, per-stream statuses and MH_BATCH_WALK_MAX_BITS cap.  A symbol whose context or pair
 * has no code in the stream's model is skipped, as mh_encode does. */
size_t mh_encode_each_bound(const mh_model_set *s, size_t total, size_t n_streams);
size_t mh_dev_encode_each_workspace(size_t n_streams, size_t total);
int mh_dev_encode_each(const mh_model_set *s, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total,
                       uint8_t prev0, uint8_t *d_payload, size_t cap, uint64_t *d_out_off, uint64_t *d_nbits,
                       uint64_t *d_index, uint32_t chunk_symbols, void *d_ws, size_t ws_bytes, void *stream);
size_t mh_dev_decode_each_workspace(size_t n_streams);
int mh_dev_decode_each(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                       size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                       uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                       int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);

/* Host-buffer forms.  Offsets are checked before a device is touched.  The streams are coded in groups whose device
 * footprint stays near MH_EACH_GROUP_BYTES (environment variable of the same name overrides it, in bytes): a set grows
 * with the streams' live contexts, up to 256 x 3.8 KiB per stream.  A stream longer than MH_EACH_DIRECT_BYTES goes
 * through the single-stream calls instead, where the per-call cost is already small against its work.
 *   mh_compress_each: data + in_off -> tables (tab_off[n + 1]), payloads (out_off[n + 1], nbits[n]) and, when index is not
 *     NULL, the index slices (mh_batch_index_capacity entries; gap entries keep their values).  The outputs never exceed
 *     the sizes mh_compress_each_bounds gives: tables 33 n + ceil(20 total / 8) + 16 bytes, payloads the sum over streams
 *     of ceil(len_i x max(1, min(64, len_i - 1)) / 8), + n + 16.  Smaller caps: MH_ERR_CAPACITY.
 *   mh_decompress_each: tables + payloads + nbits -> messages (sym_off as in mh_decode_batch: input with an index, output
 *     without) and per-stream statuses (may be NULL).  Streams over MH_BATCH_WALK_MAX_BITS without an index are decoded
 *     by mh_decode.  Returns the first stream's error, if any. */
#define MH_EACH_GROUP_BYTES (1ull << 30)
#define MH_EACH_DIRECT_BYTES (1ull << 24)
int mh_compress_each_bounds(const uint64_t *in_off, size_t n_streams, size_t *tables_bound, size_t *payload_bound);
int mh_compress_each(const uint8_t *data, const uint64_t *in_off, size_t n_streams, int order, uint8_t prev0,
                     uint8_t *tables, size_t tab_cap, uint64_t *tab_off, uint8_t *out_payload, size_t cap, uint64_t *out_off,
                     uint64_t *nbits, uint64_t *index, uint32_t chunk_symbols);
int mh_decompress_each(const uint8_t *tables, const uint64_t *tab_off, const uint8_t *payload, const uint64_t *pay_off,
                       const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off,
                       const uint64_t *index, uint32_t chunk_symbols, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * RANDOM ACCESS: BYTE RANGES OF AN INDEXED STREAM — a few bytes out of a large stream (4 KiB at offset 9 GiB of a `.cm` with
 * its --index sidecar; records spread over a compressed log) without decoding or uploading the rest.  Order 0 and order 1
 * models; an order-2 model is refused with MH_ERR_ARG before anything is launched, and so is n_symbols > nbits (every code
 * has at least one bit: no stream of n_symbols fits in fewer bits).
 *   - A range is [begin, end) in symbols, i.e. bytes of the original input: 2 x uint64 per range.  Empty ranges (begin ==
 *     end, [n, n) included) are MH_OK and write nothing.  Ranges may overlap each other and come in any order.
 *   - The stream needs its chunk index (mh_encode, mh_dev_encode*, a batch stream's slice).  A stream without one (what the
 *     reference writes) gets both indices from mh_dev_build_index_fine first.
 *   - Work unit: a chunk of the index, or MH_FINE_SYMBOLS symbols with the fine index.  One lane decodes one (range, unit)
 *     item: it starts at the unit's entry, decodes the symbols in front of the range without storing them, then stores the
 *     rest of its share.  Without a fine index a lane may skip up to chunk_symbols - 1 symbols to store one; with it, at most
 *     MH_FINE_SYMBOLS - 1.
 *   - Checks.  An item that ends exactly on a unit boundary must use exactly the bits between its unit's entry and the next
 *     one (nbits after the stream's last symbol).  An item that ends inside a unit is checked only for null table entries
 *     and for running past nbits.  A unit whose entry lies past nbits or behind the entry before it is corrupt: every range
 *     that touches it or ends on its start boundary gets MH_ERR_CORRUPT; the others decode byte-exact.  Huffman decoding
 *     re-synchronises, so an entry moved to another plausible position is not always detected.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_decode_ranges_workspace(size_t n_ranges);
/* Decodes n_ranges ranges of ONE stream.  d_ranges: 2 x uint64 per range.  Range j's end - begin bytes go to
 * d_out[d_out_at[j] ...); outputs of different ranges must not overlap; a range whose output would reach past out_cap writes
 * nothing (MH_ERR_CAPACITY for that range).  Nothing is written outside the outputs of the ranges that are decoded.
 * d_payload (any alignment) holds the stream's payload bytes [payload_byte_base, payload_byte_base + payload_bytes): a window
 * of the payload (the whole payload is base 0, bytes ceil(nbits / 8)); index bit offsets stay relative to the stream start.
 * Reads touch only the aligned dwords that hold window bytes.  A batch stream is d_payload = batch payload + pay_off[i]
 * with d_index = its slice (mh_batch_index_base).  d_fine (NULL = none): the stream's fine index (mh_dev_encode_fine,
 * mh_dev_build_index_fine).  d_out: 16-byte aligned.  d_range_status[j]: MH_OK, MH_ERR_ARG (begin > end, end > n_symbols,
 * a unit outside the payload window), MH_ERR_CAPACITY or MH_ERR_CORRUPT; the workspace's status word (mh_dev_status) keeps
 * one of them.  No host synchronisation, no allocation. */
int mh_dev_decode_ranges(const mh_model *m, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes,
                         uint64_t nbits, const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols,
                         const uint32_t *d_fine, const uint64_t *d_ranges, size_t n_ranges,
                         uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                         int32_t *d_range_status, void *d_ws, size_t ws_bytes, void *stream);
/* Host form: payload and index are the whole stream in host memory (for example a mapped .cm and its sidecar).  Outputs are
 * packed in range order: out_off[j] = sum of the lengths of the ranges before j (n_ranges + 1 entries, written; a range
 * refused with MH_ERR_ARG has length 0).  Only the payload bytes of the chunks the ranges touch are uploaded: the byte spans
 * of those chunks are sorted, spans less than 1 MiB apart are merged into one window, windows are cut at the segment size
 * (MH_SEGMENT_BYTES), and each window is one mh_dev_decode_ranges call; ranges that cross a window edge are split.  Device
 * footprint: about one segment of payload and one of output, plus the pieces.  range_status (may be NULL) as above;
 * returns MH_OK or the first failing range's status. */
int mh_decode_ranges(const mh_model *m, const uint8_t *payload, uint64_t nbits, const uint64_t *index,
                     uint32_t chunk_symbols, uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges,
                     uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *range_status);
/* Diagnostic: payload bytes the calling thread's last mh_decode_ranges uploaded. */
uint64_t mh_last_range_upload_bytes(void);

/* ---------------------------------------------------------------------------------------------------------------------
 * RANDOM ACCESS INTO BATCHES — point lookups into packed records: bytes [begin, end) of stream `stream` of a batch (the
 * batch section or the one-model-each section above), for many lookups in one call and a fixed number of launches.
 * Order 0 and order 1; a shared order-2 model is refused with MH_ERR_ARG before anything is launched.  No new format: the
 * batch is pay_off[n + 1], nbits[n], prev0 and, optionally, the closed-form index slices (mh_batch_index_base).
 *   - A lookup is 3 x uint64: stream, begin, end; begin and end count symbols from the start of that stream.  Lookups may
 *     repeat, overlap and come in any order.  Empty lookups ([n_i, n_i) included) are MH_OK and write nothing.
 *   - With an index, sym_off[n + 1] (the encode's in_off) is input and a lookup with end > n_i is MH_ERR_ARG.  One lane
 *     decodes one (lookup, chunk) item from the chunk's entry, with the checks of the section above: an entry must lie in
 *     [0, nbits_i] and not behind its predecessor; an item that ends on a chunk boundary or at n_i must use exactly the bits
 *     up to the next entry (nbits_i after the last chunk); one that ends inside a chunk is checked for null table entries
 *     and for running past nbits_i.
 *   - Without an index (the `.cm` files the reference writes), one lane walks the stream from bit 0 in context prev0, skips
 *     `begin` symbols and stores the rest.  Streams over MH_BATCH_WALK_MAX_BITS are MH_ERR_ARG for their lookups in the
 *     device calls (the host forms decode them through mh_decode).  A walk that reaches nbits_i before `end` ran past the
 *     stream's end: MH_ERR_ARG; running past nbits_i inside a code or a null table entry: MH_ERR_CORRUPT.  sym_off is
 *     optional here; when given, end > n_i is refused up front and a lookup that ends at n_i must end exactly at nbits_i
 *     (src/coding.cpp:124,158).
 *   - Per-lookup status: MH_OK, MH_ERR_ARG (stream >= n_streams, begin > end, nbits_i beyond the stream's payload bytes,
 *     non-monotone offsets of the stream, the cases above), MH_ERR_CAPACITY (output past out_cap: nothing written) or
 *     MH_ERR_CORRUPT, the first error kept.  A corrupt entry or payload of stream k fails only the lookups that read it.
 *     The workspace's status word (mh_dev_status) keeps one of the errors.
 *   - Only the offsets of the streams the lookups name are read: the device calls' cost does not depend on n_streams.
 *   - Lookup j writes end - begin bytes to d_out[d_out_at[j] ...); outputs of different lookups must not overlap.  Nothing
 *     is written outside the outputs of the lookups that are decoded; a lookup that fails while decoding (MH_ERR_CORRUPT,
 *     or an index-free walk that ends before `end`) may have written part of its own output.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_decode_batch_ranges_workspace(size_t n_lookups);
/* Under one shared model.  d_payload, d_out and d_ws 16-byte aligned; d_sym_off may be NULL only without d_index.  No host
 * synchronisation, no allocation. */
int mh_dev_decode_batch_ranges(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                               size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index,
                               uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                               uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                               int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream);
/* The same with stream i under the set's model i (n_streams == mh_model_set_size(s), else MH_ERR_ARG). */
int mh_dev_decode_each_ranges(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                              size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index,
                              uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                              uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                              int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream);
/* Host forms: payload (payload_bytes) and tables (tables_bytes) are whole host buffers, for example a mapped archive.
 * Before a device is touched every lookup is checked, with its stream's offsets against those lengths (a bad one is
 * MH_ERR_ARG for that lookup), and, for mh_decompress_each_ranges, its stream's table file is parsed: a malformed table
 * fails that stream's lookups with MH_ERR_BADTABLE; an untouched stream's table and payload are never read.  Outputs are
 * packed in lookup order: out_off[n_lookups + 1] is written, a refused lookup has length 0 (one that does not fit keeps its
 * length, MH_ERR_CAPACITY).  Only the touched streams are uploaded: their payloads, whole and compacted, and their index
 * slices re-based to the compacted sym_off; a touched stream of more than MH_EACH_DIRECT_BYTES of payload, or an index-free
 * one over MH_BATCH_WALK_MAX_BITS, goes through mh_decode_ranges on its slice (indexed) or mh_decode (index-free) instead.
 * lookup_status (may be NULL) as above; returns MH_OK or the first failing lookup's status. */
int mh_decode_batch_ranges(const mh_model *m, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off,
                           const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off,
                           const uint64_t *index, uint32_t chunk_symbols, const uint64_t *lookups, size_t n_lookups,
                           uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status);
int mh_decompress_each_ranges(const uint8_t *tables, uint64_t tables_bytes, const uint64_t *tab_off,
                              const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off,
                              const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off,
                              const uint64_t *index, uint32_t chunk_symbols, const uint64_t *lookups, size_t n_lookups,
                              uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status);
/* Diagnostic: payload bytes the calling thread's last mh_decode_batch_ranges / mh_decompress_each_ranges uploaded. */
uint64_t mh_last_batch_range_upload_bytes(void);

/* ---------------------------------------------------------------------------------------------------------------------
 * RANDOM ACCESS INTO ORDER-2 STREAMS (extension, parity unpinned) — the two sections above for order-2 models: byte ranges
 * of one indexed order-2 stream (mh_encode, mh_dev_encode_ctx*, mh_dev_build_index, a slice of mh_encode_batch_o2) and
 * lookups into a batch of mh_encode_batch_o2.  Every call mirrors its order-0/1 counterpart argument for argument, and the
 * contract is that of the sections above word for word, apart from these points:
 *   - Model.  These calls refuse any model whose mh_model_type is not 2 with MH_ERR_ARG before anything is launched; the
 *     order-0/1 calls keep refusing order 2.
 *   - Index entries are order-2 entries: (two context bytes) << 48 | bit offset (MH_INDEX2_BIT_MASK masks the offset; the
 *     host forms' window logic masks with it too).  Index-free batch streams are walked from bit 0 in context
 *     (prev0, prev0), under the MH_BATCH_WALK_MAX_BITS cap.
 *   - Fine index (mh_dev_decode_ranges_o2 only, optional): the order-2 form of the FINE INDEX note, written by
 *     mh_dev_encode_ctx_fine; chunk_symbols <= 1024 with a fine index (else MH_ERR_ARG), d_fine 4-byte aligned.  The work unit
 *     is then a piece of MH_FINE_SYMBOLS symbols.  A piece whose entry's low half is 0xFFFF is not used: its lane starts at
 *     the nearest earlier usable piece of the same chunk (or at the chunk's entry) and skips forward, and an item that ends
 *     at its start is checked as one that ends inside a unit.  A usable fine entry past the next chunk entry or past nbits
 *     makes every range that reads that piece (starts there, or ends at its start) MH_ERR_CORRUPT.
 *   - A range of mh_dev_decode_ranges_o2 whose decode reads past the payload window is MH_ERR_ARG.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_decode_ranges_o2_workspace(size_t n_ranges);
/* mh_dev_decode_ranges for an order-2 model (d_fine: the order-2 fine index or NULL).  No host synchronisation, no
 * allocation. */
int mh_dev_decode_ranges_o2(const mh_model *m, const uint8_t *d_payload, uint64_t payload_byte_base, uint64_t payload_bytes,
                            uint64_t nbits, const uint64_t *d_index, uint32_t chunk_symbols, uint64_t n_symbols,
                            const uint32_t *d_fine, const uint64_t *d_ranges, size_t n_ranges,
                            uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                            int32_t *d_range_status, void *d_ws, size_t ws_bytes, void *stream);
/* mh_decode_ranges for an order-2 model: the same window merging and segment cut; mh_last_range_upload_bytes reports its
 * upload. */
int mh_decode_ranges_o2(const mh_model *m, const uint8_t *payload, uint64_t nbits, const uint64_t *index,
                        uint32_t chunk_symbols, uint64_t n_symbols, const uint64_t *ranges, size_t n_ranges,
                        uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *range_status);
size_t mh_dev_decode_batch_o2_ranges_workspace(size_t n_lookups);
/* mh_dev_decode_batch_ranges for a shared order-2 model. */
int mh_dev_decode_batch_o2_ranges(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                                  size_t n_streams, uint8_t prev0, const uint64_t *d_sym_off, const uint64_t *d_index,
                                  uint32_t chunk_symbols, const uint64_t *d_lookups, size_t n_lookups,
                                  uint8_t *d_out, const uint64_t *d_out_at, uint64_t out_cap,
                                  int32_t *d_lookup_status, void *d_ws, size_t ws_bytes, void *stream);
/* mh_decode_batch_ranges for a shared order-2 model: only the touched streams are uploaded; a touched stream over
 * MH_EACH_DIRECT_BYTES, or an index-free one over MH_BATCH_WALK_MAX_BITS, goes through mh_decode_ranges_o2 on its slice
 * (indexed) or mh_decode (index-free).  mh_last_batch_range_upload_bytes reports the upload. */
int mh_decode_batch_o2_ranges(const mh_model *m, const uint8_t *payload, uint64_t payload_bytes, const uint64_t *pay_off,
                              const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off,
                              const uint64_t *index, uint32_t chunk_symbols, const uint64_t *lookups, size_t n_lookups,
                              uint8_t *out, size_t out_cap, uint64_t *out_off, int32_t *lookup_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * BANKS OF SHARED MODELS — the middle ground between one shared model (a table once, statistics that may not fit) and one
 * model per stream (an exact fit, a table per message): K shared models, K <= MH_BANK_MAX, and each stream coded under the
 * one that suits it best (the reference's "general-use Huffman tables stored in a shared manner", README.md:152-157).
 * No new format: every bank entry is an ordinary order-0/1 table file (`.eh` / `.e`), every stream's `.cm` is what
 * `markovhuffman msg -e bank_k.e -o msg.cm` writes, and the only side information is one entry number per stream.  Order 0
 * and order 1; order 2 is refused with MH_ERR_ARG before anything is launched.  in_off, prev0, packed payloads and the
 * closed-form index slices are those of the batch section above.
 *
 * A bank is an ordinary mh_model_set whose K "streams" are the shared models (mh_model_set_from_models,
 * mh_model_set_from_tables with K table files, or mh_dev_bank_train); mh_dev_model_set_tables on a bank writes its K tables.
 * --------------------------------------------------------------------------------------------------------------------- */
#define MH_BANK_MAX 64
#define MH_BANK_NONE 0xFFFFFFFFu

/* Selection: for every stream i and entry k, nbits(i, k) = the sum of the code lengths of the stream's symbols, each in its
 * context from prev0.  Entry k is eligible for stream i only when every (context, symbol) pair of the stream has a code in it
 * (the reference's NDEBUG build would silently drop a symbol without one).  d_choice[i] = the eligible entry with the fewest
 * bits, ties to the lowest k; MH_BANK_NONE when none is eligible (d_nbits[i] = UINT64_MAX then).  An empty stream costs 0
 * under every entry: entry 0.  d_nbits (may be NULL) = nbits(i, choice[i]), the nbits mh_encode writes for the message under
 * that entry.  The bank has 1 .. MH_BANK_MAX entries (else MH_ERR_ARG).  No allocation, no host synchronisation; bad
 * offsets: MH_ERR_ARG through mh_dev_status(d_ws).  d_ws 16-byte aligned, at least mh_dev_bank_select_workspace bytes. */
size_t mh_dev_bank_select_workspace(size_t n_entries, size_t n_streams, size_t total);
int mh_dev_bank_select(const mh_model_set *bank, const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total,
                       uint8_t prev0, uint32_t *d_choice, uint64_t *d_nbits, void *d_ws, size_t ws_bytes, void *stream);

/* The set view: a set of n_streams streams in which stream i's model is bank entry d_choice[i] (type, longest code and
 * context -> slot row copied; the slots are the bank's, shared: about 1 KiB per stream).  mh_dev_encode_each,
 * mh_dev_decode_each and mh_dev_decode_each_ranges take it as any set.  Allocates the view and synchronises `stream` once;
 * a choice >= K (MH_BANK_NONE included): MH_ERR_ARG and no view.  The view keeps the bank's device memory alive: freeing the
 * bank first is legal.  mh_model_set_size(view) = n_streams, mh_model_set_slots and mh_model_set_code_lens give the bank's
 * values; mh_dev_model_set_tables(view) is MH_ERR_ARG (write the bank's tables instead). */
int mh_dev_model_set_pick(const mh_model_set *bank, const uint32_t *d_choice, size_t n_streams, void *stream, mh_model_set **out);

/* Training.  Seed: the shared model of all streams (mh_dev_histogram_o1_batch / _o0_batch + mh_dev_model_from_counts);
 * streams stable-sorted by their bits per byte under it (compared exactly, nbits_i x len_j against nbits_j x len_i; an empty
 * stream counts 0 bits per byte), ties by stream index, cut into min(K, n) groups of equal count.  Then up to max_iters
 * (>= 1) iterations, stopping early when no choice changes: (1) one model per group, trained on the summed counts of its
 * streams, each stream from prev0 (the streams are sorted by group and gathered, and the batch histogram runs over each
 * group); (2) selection under the new models.  Result: the bank of the last (1), without the entries whose group held no
 * symbol (K' <= K entries, at least 1), and the choices of the (2) that followed, numbered in that bank; *iters_run (may be
 * NULL) = the iterations run.  Neither step can raise sum_i nbits_i: a Huffman code is optimal for its group's counts and a
 * stream's old entry stays eligible.  Deterministic.  Allocates the bank and synchronises `stream` a number of times that
 * depends on K and the iterations, not on n.  n_streams == 0 or total == 0: a bank of one empty model, choices 0.
 * d_data 16-byte aligned or not; d_ws 16-byte aligned, at least mh_dev_bank_train_workspace bytes. */
size_t mh_dev_bank_train_workspace(size_t n_streams, size_t total, uint32_t k);
int mh_dev_bank_train(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, int order, uint8_t prev0,
                      uint32_t k, uint32_t max_iters, uint32_t *d_choice, int *iters_run, void *d_ws, size_t ws_bytes, void *stream,
                      mh_model_set **bank);

/* Host forms.  Offsets and choices are checked before a device is touched.
 *   mh_bank_train: the device training on a host batch; choice[n] is written to host memory.
 *   mh_encode_bank_bound: the exact worst case of the packed payloads, sum_i ceil(len_i x maxlen(choice_i) / 8) + n + 16
 *     (0 for a null argument or a choice >= K).
 *   mh_encode_bank: stream i under entry choice[i]: out_off[n + 1], nbits[n], payloads, and the index slices when index is not
 *     NULL (mh_batch_index_capacity entries; gap entries keep their values).  A cap below what the payloads need:
 *     MH_ERR_CAPACITY.  Device footprint: input + payloads + 1 KiB per stream + the index + mh_dev_encode_each_workspace.
 *   mh_decode_bank: the inverse, in the style of mh_decode_batch (sym_off input with an index, output without;
 *     stream_status may be NULL; returns the first stream's error).  Index-free streams over MH_BATCH_WALK_MAX_BITS are
 *     decoded by mh_decode under their entry, parsed from the bank's table. */
int mh_bank_train(const uint8_t *data, const uint64_t *in_off, size_t n_streams, int order, uint8_t prev0, uint32_t k,
                  uint32_t max_iters, uint32_t *choice, int *iters_run, mh_model_set **bank);
size_t mh_encode_bank_bound(const mh_model_set *bank, const uint32_t *choice, const uint64_t *in_off, size_t n_streams);
int mh_encode_bank(const mh_model_set *bank, const uint8_t *data, const uint64_t *in_off, size_t n_streams, uint8_t prev0,
                   const uint32_t *choice, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *nbits, uint64_t *index,
                   uint32_t chunk_symbols);
int mh_decode_bank(const mh_model_set *bank, const uint32_t *choice, const uint8_t *payload, const uint64_t *pay_off,
                   const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint8_t *out, size_t out_cap, uint64_t *sym_off,
                   const uint64_t *index, uint32_t chunk_symbols, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * SEARCH IN BATCHES — which streams of a batch contain which byte strings, and where, without writing the decoded bytes:
 * the batch decoders hold every decoded byte in a register for one step, and here that byte feeds a matcher instead of a
 * store.  No buffer for the original data is needed; the workspace is a few bytes per chunk.  Order 0 and order 1; an
 * order-2 model is MH_ERR_ARG before any launch (its batches are searched by mh_dev_find_batch_o2, section ORDER 2 IN
 * SEARCH AND RE-CODING).  The batch is described exactly as for mh_dev_decode_batch /
 * mh_dev_decode_each (payload layout, pay_off, nbits, prev0, sym_off and the index slices of mh_batch_index_base, the same
 * alignment rules and up-front checks with the same statuses); a bank view of mh_dev_model_set_pick is a set.
 *   - A pattern set is a host object (no device needed): up to MH_FIND_MAX_POSITIONS bytes of patterns in all, pattern j =
 *     bytes[pat_off[j] .. pat_off[j+1]), any byte values.  MH_ERR_ARG for n_patterns == 0, an empty pattern, pat_off[0] != 0,
 *     decreasing offsets, a total over MH_FIND_MAX_POSITIONS, unknown flag bits, null pointers.  Equal patterns may appear
 *     twice; each reports its own hits.  With MH_FIND_FOLD_ASCII 'A'..'Z' and 'a'..'z' match each other, in the pattern and
 *     in the data; no other byte is folded.  The matcher is Shift-And over one 64-bit word: pattern j owns len_j bits.
 *   - A hit is an occurrence of pattern j at bytes [begin, end) of ONE stream's decoded message, end - begin = len_j, counted
 *     from the start of that stream.  Overlapping occurrences all count (`aa` occurs three times in `aaaa`).  Nothing
 *     matches across a stream boundary; a stream shorter than a pattern has no hit of it.
 *   - d_hit_off[n + 1] (written in full, also count-only and when the hits do not fit) is the exclusive scan of the streams'
 *     hit counts; d_hit_off[n] is the total.
 *   - Record r is d_hits[3r .. 3r+2] = (stream, begin, end) and d_hit_pattern[r] = j (d_hit_pattern may be NULL); stream i's
 *     records are [d_hit_off[i], d_hit_off[i+1]).  The records are the lookups of mh_dev_decode_batch_ranges as they are.
 *     Their order is fixed: ascending (stream, end, pattern number), whatever chunk_symbols is, with or without an index.
 *     d_hits == NULL: count only.
 *   - Records with number >= hit_cap are not written, nothing is written at or beyond hit_cap records, and the workspace
 *     status is MH_ERR_CAPACITY; the records below hit_cap are the true prefix.
 *   - d_stream_status[n] (may be NULL): for every stream the verdict mh_dev_decode_batch / mh_dev_decode_each gives the same
 *     arguments (indexed: every chunk gives its symbols and ends exactly at the next entry, the last at nbits_i; index-free:
 *     the walk ends exactly at nbits_i with no null table entry; MH_ERR_ARG for nbits_i beyond its payload bytes and,
 *     index-free, over MH_BATCH_WALK_MAX_BITS).  A failed stream has zero hits in d_hit_off and writes no record; the other
 *     streams are unaffected.  mh_dev_status(d_ws) keeps one of the errors.
 *   - With an index, the hits are those of the bytes mh_dev_decode_batch / mh_dev_decode_each returns for the same
 *     arguments.  An entry's context field is taken as the symbol (order 2: the two symbols) in front of its chunk, as every
 *     index writer of this library writes it.  An entry whose context field is wrong but whose chunk still decodes to its
 *     end bit keeps its stream's verdict MH_OK, as in mh_dev_decode_batch, and its chunk decodes to other bytes: a hit across
 *     that seam is counted and reported as those bytes hold it (the lane in front decodes the symbols behind the seam from
 *     the entry's context field, as the chunk's own lane does), so the count and the records always agree.
 *   - Without d_index the call is index-free (one lane walks one stream): d_sym_off may be NULL and is neither read nor
 *     written, sym_total and chunk_symbols are ignored.  Long index-free streams: mh_dev_batch_states + mh_dev_batch_index
 *     first.
 * No allocation, no host synchronisation, a number of launches that does not depend on the data or on n_streams.
 * d_payload and d_ws 16-byte aligned; d_ws at least mh_dev_find_batch_workspace(n, sym_total, chunk_symbols) bytes
 * (chunk_symbols 0: index-free).
 * Host form mh_find_batch: arguments checked before a device is touched, the batch uploaded, the device call run once,
 * results copied back; returns the first stream's error, else MH_ERR_CAPACITY when the hits do not fit.  Index-free batches
 * with a stream over MH_BATCH_WALK_MAX_BITS are indexed by mh_index_batch first (chunk MH_CHUNK_DEFAULT) and searched with
 * that index, so a valid batch is never refused.
 * --------------------------------------------------------------------------------------------------------------------- */
typedef struct mh_pattern_set mh_pattern_set;
#define MH_FIND_MAX_POSITIONS 64          /* sum of the patterns' lengths */
#define MH_FIND_FOLD_ASCII    1u          /* 'A'..'Z' and 'a'..'z' match each other; no other byte is folded */
int mh_pattern_set_create(const uint8_t *bytes, const uint32_t *pat_off, size_t n_patterns, uint32_t flags,
                          mh_pattern_set **out);
size_t mh_pattern_set_size(const mh_pattern_set *ps);
int mh_pattern_set_max_len(const mh_pattern_set *ps);
void mh_pattern_set_free(mh_pattern_set *ps);
size_t mh_dev_find_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off,
                      const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                      const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                      uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                      int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
/* The same with stream i under the set's model i (n_streams == mh_model_set_size(s), else MH_ERR_ARG). */
int mh_dev_find_each(const mh_model_set *s, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off,
                     const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                     const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                     uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_find_batch(const mh_model *m, const mh_pattern_set *ps, const uint8_t *payload, const uint64_t *pay_off,
                  const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                  uint32_t chunk_symbols, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                  int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * RE-CODING BATCHES — a batch of compressed records moved to another model without a buffer for the decoded bytes: the
 * (prev, sym) histogram of a compressed batch (the training counts of the new model) and the batch coded again under a
 * destination model, both taken from each decoded symbol while it sits in a register.  Order 0 and order 1 on both sides,
 * independently; an order-2 model on either side is MH_ERR_ARG before any launch (the _o2 calls of section ORDER 2 IN
 * SEARCH AND RE-CODING serve every pair with an order-2 side).  The source batch is described exactly as
 * for mh_dev_decode_batch / mh_dev_decode_each (payload layout, pay_off, nbits, prev0, sym_off and the index slices of
 * mh_batch_index_base, the same alignment rules and up-front checks with the same statuses); a bank view of
 * mh_dev_model_set_pick is a set.  An index entry's context byte is taken as the symbol in front of its chunk, as every
 * index writer of this library writes it.
 *   - d_stream_status[n] (may be NULL): for every stream the verdict mh_dev_decode_batch / mh_dev_decode_each gives the same
 *     arguments (see SEARCH IN BATCHES).  mh_dev_status(d_ws) keeps one of the errors.
 *   - Histogram: `order` (0 or 1, else MH_ERR_ARG) is the order of the histogram, not of the source model; d_counts holds
 *     256 or 65 536 counts and is written in full: the summed counts of every stream that decodes, each starting in context
 *     prev0 — for an undamaged batch exactly what mh_dev_histogram_o1_batch / _o0_batch give the original messages.  A
 *     stream whose verdict is not MH_OK contributes nothing: a chunk counts as it decodes and takes its counts back when it
 *     fails, and a last pass takes back the chunks that passed inside a stream that failed.  The counters are exact 64-bit
 *     sums.  Index-free (d_index NULL): one lane walks one stream, d_sym_off may be NULL.
 *   - Re-code: for every stream whose verdict is MH_OK the output equals what mh_dev_encode_batch(dst, ...) produces from
 *     the decoded messages: d_out_off[n + 1] (byte-aligned packed payloads), d_out_nbits[n], the payload bytes and the index
 *     slices in d_out_index (may be NULL; mh_batch_index_base layout, the same chunk_symbols; gap entries untouched).  A
 *     (prev, sym) pair without a code under dst is skipped and the context advances (the reference's NDEBUG rule);
 *     d_dropped[n] (may be NULL) counts those symbols per stream, the stream's status stays MH_OK.
 *   - A stream whose verdict is not MH_OK gets nbits 0 and no payload byte (out_off[i + 1] == out_off[i]); its index slice
 *     is left untouched and its dropped count is 0.  The other streams are unaffected.
 *   - Nothing is written at or beyond min(cap, out_off[n]) bytes of d_out_payload.  A payload that does not fit: the
 *     workspace status is MH_ERR_CAPACITY, offsets, lengths, dropped counts and statuses are still written, payload and
 *     index are not.  d_out_payload == NULL: count only (cap ignored) — offsets, lengths, d_sym_off (index-free), dropped
 *     counts, statuses and, when d_out_index is given, the index; the caller sizes the payload from d_out_off[n].
 *   - Index-free source (d_index NULL): one lane walks one stream under MH_BATCH_WALK_MAX_BITS, d_sym_off[n + 1] is an
 *     output (required), chunk_symbols and d_out_index describe only the destination index, and sym_total is the number of
 *     symbols d_out_index was sized for (mh_batch_index_capacity(sym_total, n, chunk) entries): a batch that decodes to
 *     more is MH_ERR_CAPACITY with neither payload nor index written.  A batch the reference wrote comes out re-coded
 *     and indexed.
 * No allocation, no host synchronisation, a number of launches that does not depend on the data or on n_streams.
 * d_payload, d_out_payload and d_ws 16-byte aligned; d_ws at least the _workspace(n, sym_total, chunk_symbols) bytes
 * (chunk_symbols 0: index-free): per chunk number and per stream, never per payload or message byte.
 * Host form mh_recode_batch: arguments checked before a device is touched, the batch uploaded, the device call run once,
 * results copied back; sym_off is input with an index and output without; out_index (may be NULL) has
 * mh_batch_index_capacity(sym_off[n], n, chunk) entries with an index, and without one the same for the sum of
 * nbits_i / mh_model_min_code_len(src) symbols.  Index-free batches with a stream over MH_BATCH_WALK_MAX_BITS are indexed by
 * mh_index_batch first, so a valid batch is never refused.  Returns the first stream's error, else MH_ERR_CAPACITY.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_histogram_coded_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_histogram_coded_batch(const mh_model *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off,
                                 const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                                 const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                                 uint64_t *d_counts, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
/* The same with stream i under the set's model i (n_streams == mh_model_set_size(src), else MH_ERR_ARG). */
int mh_dev_histogram_coded_each(const mh_model_set *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off,
                                const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                                const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                                uint64_t *d_counts, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
size_t mh_dev_recode_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                        const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                        uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap,
                        uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
                        int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
/* The same with stream i under the set's model i (n_streams == mh_model_set_size(src), else MH_ERR_ARG). */
int mh_dev_recode_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                       const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                       uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, uint8_t *d_out_payload, size_t cap,
                       uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
                       int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_recode_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                    const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                    uint32_t chunk_symbols, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits,
                    uint64_t *out_index, uint64_t *dropped, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * ORDER 2 IN SEARCH AND RE-CODING (extension, parity unpinned) — the two sections above with an order-2 model: a batch of
 * order-2 streams is searched, an order-0/1 batch gives the training counts of an order-2 model and is coded again under
 * it (and back), all without a buffer for the decoded bytes.  The calls of those sections keep refusing an order-2 model.
 * Everything not said here is word for word SEARCH IN BATCHES and RE-CODING BATCHES: the batch description, alignment
 * rules and up-front checks with their statuses, d_stream_status, mh_dev_status(d_ws), the capacity rules, count-only
 * mode, the index-free walk under MH_BATCH_WALK_MAX_BITS, and "no allocation, no host synchronisation, a number of
 * launches that does not depend on the data or on n_streams".  Order-2 particulars are those of BATCHES OF ORDER-2
 * STREAMS: a stream starts in context (prev0, prev0), index entries of an order-2 model carry two context bytes in bits
 * 48..63 (MH_INDEX2_BIT_MASK), a pair without a code is skipped while the context advances.
 *   - mh_dev_find_batch_o2 / mh_find_batch_o2: arguments and results of mh_dev_find_batch / mh_find_batch with the same
 *     mh_pattern_set; the model must be order 2, else MH_ERR_ARG before any launch.  The record order (stream, end,
 *     pattern) does not depend on the chunk size or on the index; verdicts are those mh_dev_decode_batch_o2 gives the same
 *     arguments.  The workspace is mh_dev_find_batch_workspace's for the same arguments.
 *   - mh_dev_histogram_coded_batch_o2: `src` is a shared model of any order and `order` is 0, 1 or 2; at least one of the
 *     two is 2, anything else is MH_ERR_ARG (mh_dev_histogram_coded_batch serves it).  d_counts holds 256, 65 536 or
 *     1 << 24 counts and is written in full; for an undamaged batch they are exactly what mh_dev_histogram_o0_batch /
 *     _o1_batch / _o2_batch give the original messages (order 2: each stream's first symbol counted in (prev0, prev0), its
 *     second in (prev0, first byte)).  A stream whose verdict is not MH_OK contributes nothing.  The workspace keeps
 *     nothing per chunk; the caller owns the 128 MiB of order-2 counters.
 *   - mh_dev_recode_batch_o2 / mh_recode_batch_o2: `src` and `dst` are shared models of any order, at least one of
 *     order 2, else MH_ERR_ARG.  For every MH_OK stream the output is byte for byte what mh_dev_encode_batch_o2(dst)
 *     (order-2 dst) or mh_dev_encode_batch(dst) (order-0/1 dst) writes for the decoded message: offsets, nbits, payload
 *     and the index slices in the DESTINATION's entry format.  d_dropped counts the symbols without a code under dst.  A
 *     failed stream gets nbits 0, no payload byte, an untouched index slice and dropped 0.  Verdicts are those of
 *     mh_dev_decode_batch (order-0/1 src) or mh_dev_decode_batch_o2 (order-2 src).  The workspace is at most 24 bytes
 *     per chunk number + 8 per stream + 4 KiB: never per payload or message byte.
 *   - With an order-0/1 source and an index, the first symbol of chunk k is priced, coded and counted by the lane of chunk
 *     k - 1, which decodes it behind its own chunk in the context of the symbols it decoded (an order-0/1 entry does not
 *     carry the symbol two in front).  As in RE-CODING BATCHES, an entry's context byte is taken as the symbol in front of
 *     its chunk, as every index writer of this library writes it.  An entry whose context byte is wrong but whose chunk
 *     still decodes to its end bit keeps its stream's verdict MH_OK, as in mh_dev_decode_batch; that one symbol's code and
 *     count are then those of the neighbour's decode, not of the chunk's own.  Writes stay in bounds either way: the length
 *     and the emit pass make the same decode.
 *   - Host forms check their arguments before a device is touched and never refuse a valid batch.  An order-0/1
 *     index-free source with a stream over MH_BATCH_WALK_MAX_BITS is indexed by mh_index_batch first.  An order-2 source
 *     is not yet moved onto its batch index builder (mh_index_batch_o2, a follow-up): such a stream is handled alone, as
 *     mh_decode_batch_o2 does — mh_decode, then the host-side automaton over its bytes (search) or mh_encode under dst
 *     (re-code), the result spliced into place in stream order.
 * Not part of this family: model sets (`_each`) — sets are order 0/1, and a set source with an order-2 destination is a
 * follow-up; an LDS image of the live contexts for the order-2 decoder; the command-line tool, which keeps refusing
 * --order2 with --find and --recode.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_find_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_find_batch_o2(const mh_model *m, const mh_pattern_set *ps, const uint8_t *d_payload, const uint64_t *d_pay_off,
                         const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                         const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                         uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                         int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_find_batch_o2(const mh_model *m, const mh_pattern_set *ps, const uint8_t *payload, const uint64_t *pay_off,
                     const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                     uint32_t chunk_symbols, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                     int32_t *stream_status);
size_t mh_dev_histogram_coded_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_histogram_coded_batch_o2(const mh_model *src, int order, const uint8_t *d_payload, const uint64_t *d_pay_off,
                                    const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                                    const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                                    uint32_t chunk_symbols, uint64_t *d_counts, int32_t *d_stream_status, void *d_ws,
                                    size_t ws_bytes, void *stream);
size_t mh_dev_recode_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_recode_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                           const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                           uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, uint8_t *d_out_payload,
                           size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
                           int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_recode_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                       const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                       uint32_t chunk_symbols, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits,
                       uint64_t *out_index, uint64_t *dropped, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * DIGESTS OF BATCHES — the CRC-32 of every stream's decoded message without writing the decoded bytes.  A Huffman stream
 * re-synchronises after damage and then ends where it should, so most single-bit flips of a payload pass every check the
 * decoders can make and decode, with status MH_OK, to other bytes.  A digest kept beside the data catches them, and here it
 * is taken from each decoded byte while it sits in a register: no buffer for the original data, and a workspace that holds
 * nothing per chunk or per byte.  The checksum is CRC-32 as zlib, gzip and PNG define it (reflected polynomial 0xEDB88320,
 * initial value and final XOR 0xFFFFFFFF): crc32 of zlib gives the same value for the same bytes.
 * The batch is described exactly as for mh_dev_find_batch / mh_dev_find_each (payload layout, pay_off, nbits, prev0, sym_off
 * and the index slices of mh_batch_index_base, the same alignment rules and up-front checks with the same statuses); a bank
 * view of mh_dev_model_set_pick is a set.  mh_dev_crc_batch takes an order-0/1 model and refuses an order-2 model with
 * MH_ERR_ARG, mh_dev_crc_batch_o2 (extension, parity unpinned; a stream starts in context (prev0, prev0), index entries in
 * the order-2 format) takes an order-2 model and refuses any other the same way, both before any launch.
 *   - d_crc[n] is written in full: entry i is the CRC-32 of stream i's decoded message; an empty stream gives 0.  The chunks
 *     of a stream are digested independently and meet in d_crc[i] by XOR (crc(A || B) follows from the digests of A and B and
 *     the length of B), which is exact in any order: two calls on the same input give identical buffers.
 *   - d_len[n] (may be NULL): entry i is the number of decoded symbols — with an index sym_off[i+1] - sym_off[i], index-free
 *     what the walk counted, so the call also reports the lengths of streams the reference wrote.
 *   - d_stream_status[n] (may be NULL): for every stream the verdict mh_dev_decode_batch / mh_dev_decode_each /
 *     mh_dev_decode_batch_o2 gives the same arguments (see SEARCH IN BATCHES).  A failed stream has crc 0 and len 0; the
 *     other streams are unaffected.  mh_dev_status(d_ws) keeps one of the errors.
 *   - Without d_index the call is index-free (one lane walks one stream): d_sym_off may be NULL and is neither read nor
 *     written, sym_total and chunk_symbols are ignored; a stream over MH_BATCH_WALK_MAX_BITS is MH_ERR_ARG, as in the search.
 *   - A CRC that differs from an expected one is not a device verdict: the caller compares two arrays.
 * No allocation, no host synchronisation, a number of launches that does not depend on the data or on n_streams.  d_payload
 * and d_ws 16-byte aligned; d_ws at least mh_dev_crc_batch_workspace(n, sym_total, chunk_symbols) bytes (chunk_symbols 0:
 * index-free; the one function serves all three calls): 4 bytes per stream and 1.5 KiB.
 * Host forms mh_crc_batch / mh_crc_batch_o2: arguments checked before a device is touched, the batch uploaded, the device
 * call run once, results copied back; returns the first stream's error.  Index-free batches with a stream over
 * MH_BATCH_WALK_MAX_BITS are indexed by mh_index_batch / mh_index_batch_o2 first (chunk MH_CHUNK_DEFAULT) and digested with
 * that index, so a valid batch is never refused.
 * mh_dev_crc_raw_batch gives the same digest for uncompressed messages, laid out as mh_dev_encode_batch takes them (d_data
 * may start anywhere, in_off[n + 1] checked on the device: MH_ERR_ARG through mh_dev_status(d_ws)), so a store gets its
 * digests on the device when it encodes.  Not a hot path: one lane per KiB.
 * mh_crc32_combine is host arithmetic, no device: the CRC-32 of A || B from those of A and B and the length of B in bytes.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_crc_batch_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_crc_batch(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                     size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                     const uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len,
                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
/* The same with stream i under the set's model i (n_streams == mh_model_set_size(s), else MH_ERR_ARG). */
int mh_dev_crc_each(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                    size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                    const uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len,
                    int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_crc_batch_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                        size_t n_streams, uint64_t pay_total, uint8_t prev0, const uint64_t *d_sym_off, uint64_t sym_total,
                        const uint64_t *d_index, uint32_t chunk_symbols, uint32_t *d_crc, uint64_t *d_len,
                        int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_crc_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                 uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols, uint32_t *crc,
                 uint64_t *len, int32_t *stream_status);
int mh_crc_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                    size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index, uint32_t chunk_symbols,
                    uint32_t *crc, uint64_t *len, int32_t *stream_status);
size_t mh_dev_crc_raw_batch_workspace(size_t n_streams, size_t total);
int mh_dev_crc_raw_batch(const uint8_t *d_data, const uint64_t *d_in_off, size_t n_streams, size_t total, uint32_t *d_crc,
                         void *d_ws, size_t ws_bytes, void *stream);
uint32_t mh_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* ---------------------------------------------------------------------------------------------------------------------
 * DICTIONARY SEARCH IN BATCHES (extension, parity unpinned) — SEARCH IN BATCHES with thousands of patterns in one pass: the
 * matcher is an Aho-Corasick automaton turned into a full DFA instead of Shift-And over one word, so a call is not limited
 * to MH_FIND_MAX_POSITIONS pattern bytes.  Everything not said here is word for word SEARCH IN BATCHES (and, for the _o2
 * calls, the search part of ORDER 2 IN SEARCH AND RE-CODING): the batch description, alignment, the up-front checks,
 * d_hit_off, the records and their order (ascending (stream, end, pattern number)), hit_cap, count-only mode,
 * d_stream_status with the batch decoders' verdicts, index-free mode under MH_BATCH_WALK_MAX_BITS, no allocation, no host
 * synchronisation, a launch count that does not depend on the data, and the order each call refuses: mh_dev_find_dict_batch
 * and mh_find_dict_batch an order-2 model, the _o2 calls an order-0/1 model (MH_ERR_ARG before any launch);
 * mh_dev_find_dict_each takes a set or a bank view.
 *   - A dictionary is built on the host (mh_dict_create needs no device): pattern j = bytes[pat_off[j] .. pat_off[j+1]), any
 *     byte values; bytes, pat_off, n_patterns and flags as for mh_pattern_set_create, MH_FIND_FOLD_ASCII the only flag
 *     (patterns are lowered at build time, 'A'..'Z' in the data take the class of their lower-case twin).  Equal patterns
 *     may appear twice; each reports its own hits.  MH_ERR_ARG for n_patterns == 0, an empty pattern, pat_off[0] != 0,
 *     decreasing offsets, unknown flag bits, null pointers, a pattern over MH_DICT_MAX_LEN bytes, more than
 *     MH_DICT_MAX_PATTERNS patterns, an automaton of more than MH_DICT_MAX_STATES states (trie nodes, root included) and
 *     more than MH_DICT_MAX_OUTPUTS flattened outputs (the sum over the states of the patterns that end there, a state's
 *     suffix patterns included).
 *   - The automaton: states numbered breadth-first (root 0); bytes mapped to classes (class 0: the bytes of no pattern);
 *     a transition is 16 bits, the target state and bit 15 when the target has outputs; per state the depth and a list of
 *     (pattern, length) sorted by pattern number.  mh_dict_states / _classes / _size / _max_len say what was built;
 *     mh_dict_device_bytes the size of its device image (0 for NULL).
 *   - When a usable device exists mh_dict_create also uploads the image to the current device, as building a model does:
 *     allocating and synchronous, the only place that is.  Without a device the object is valid for the queries and for
 *     mh_dict_find_bytes, and the device calls return MH_ERR_NO_DEVICE.  A dictionary is immutable, may be shared by
 *     threads, and must outlive the work enqueued with it.
 *   - mh_dict_find_bytes is the host matcher, no device: the hits of one uncompressed message in (end, pattern) order;
 *     *n_hits is the total, hits[2r], hits[2r+1] = begin, end and hit_pattern[r] are written for r < hit_cap (either may be
 *     NULL); MH_ERR_CAPACITY when an output is asked for and the hits do not fit, MH_ERR_ARG for null d or n_hits.
 *   - A hit's length is its pattern's; a pattern is at most MH_DICT_MAX_LEN = 255 bytes < MH_CHUNK_MIN, so a hit spans at
 *     most two chunks, which is all the indexed search relies on.
 *   - The workspace is mh_dev_find_batch_workspace's for the same arguments.
 * Host forms mh_find_dict_batch / mh_find_dict_batch_o2: as mh_find_batch / mh_find_batch_o2; a valid batch is never
 * refused (index-free streams over the walk cap: order 0/1 indexed by mh_index_batch first, order 2 decoded alone and
 * searched by mh_dict_find_bytes, the records spliced in stream order).
 * --------------------------------------------------------------------------------------------------------------------- */
typedef struct mh_dict mh_dict;
#define MH_DICT_MAX_LEN      255u         /* one pattern; < MH_CHUNK_MIN, which the seam argument needs */
#define MH_DICT_MAX_STATES   32768u       /* automaton states, root included */
#define MH_DICT_MAX_PATTERNS 65536u
#define MH_DICT_MAX_OUTPUTS  (1u << 20)   /* flattened output lists */
int mh_dict_create(const uint8_t *bytes, const uint32_t *pat_off, size_t n_patterns, uint32_t flags, mh_dict **out);
void mh_dict_free(mh_dict *d);
size_t mh_dict_size(const mh_dict *d);
int mh_dict_max_len(const mh_dict *d);
size_t mh_dict_states(const mh_dict *d);
int mh_dict_classes(const mh_dict *d);
size_t mh_dict_device_bytes(const mh_dict *d);
int mh_dict_find_bytes(const mh_dict *d, const uint8_t *data, size_t n, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                       uint64_t *n_hits);
size_t mh_dev_find_dict_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_find_dict_batch(const mh_model *m, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off,
                           const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                           const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                           uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                           int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_find_dict_each(const mh_model_set *s, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off,
                          const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                          const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                          uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                          int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_find_dict_batch_o2(const mh_model *m, const mh_dict *d, const uint8_t *d_payload, const uint64_t *d_pay_off,
                              const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0,
                              const uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols,
                              uint64_t *d_hit_off, uint64_t *d_hits, uint32_t *d_hit_pattern, uint64_t hit_cap,
                              int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_find_dict_batch(const mh_model *m, const mh_dict *d, const uint8_t *payload, const uint64_t *pay_off,
                       const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                       uint32_t chunk_symbols, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                       int32_t *stream_status);
int mh_find_dict_batch_o2(const mh_model *m, const mh_dict *d, const uint8_t *payload, const uint64_t *pay_off,
                          const uint64_t *nbits, size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                          uint32_t chunk_symbols, uint64_t *hit_off, uint64_t *hits, uint32_t *hit_pattern, uint64_t hit_cap,
                          int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * EDITING BATCHES (extension, parity unpinned) — a length-preserving edit while re-coding: inside given spans of each
 * record every byte b is replaced by map[b] (a constant map is a mask byte), and the record is coded under dst, which may be
 * the source model itself.  The bytes are never written.  Order 0 and order 1 on both sides, independently; an order-2 model
 * on either side is MH_ERR_ARG before any launch (order 2 and its seam bookkeeping are not built, nor the refreshing of digests stored elsewhere;
 * deletions and replacements of another length, which move chunk boundaries, are SPLICING BATCHES below).
 *   - A span list: d_span_off[n + 1], the exclusive scan of the spans per stream, and d_spans[2r], d_spans[2r + 1] =
 *     (begin, end), byte positions counted from the start of that stream's decoded message.  Within a stream the spans ascend
 *     and are disjoint: begin < end <= next begin.  The part of a span at or beyond the stream's length is ignored (an
 *     index-free caller does not know the length).  d_span_off == NULL: every byte of every stream is inside (case folding,
 *     a charset map); d_spans is then ignored.  d_span_off[0] != 0 or decreasing offsets: MH_ERR_ARG through
 *     mh_dev_status(d_ws) and nothing else is written, as for d_pay_off.
 *   - d_map: 256 bytes on the device.
 *   - Contract.  Let x be stream i's message as mh_dev_decode_batch / mh_dev_decode_each returns it for the same arguments,
 *     and y[p] = map[x[p]] when p lies in one of the stream's spans, else x[p].  For every stream whose verdict is MH_OK the
 *     output equals what mh_dev_encode_batch(dst) writes for y: d_out_off, d_out_nbits, the payload bytes and the index
 *     slices, an index entry's context byte being y[start - 1] (prev0 in a stream's first chunk).  A pair (y[p-1], y[p])
 *     without a code under dst is skipped while the destination context advances to y[p], and is counted in d_dropped[i].
 *   - Verdicts: the batch decoders', and ONE more, the only verdict this call adds to theirs: a stream whose span list
 *     breaks the rule above gets MH_ERR_ARG in d_stream_status and the output of a failed stream (nbits 0, no payload byte,
 *     index slice untouched, dropped 0); mh_dev_status(d_ws) keeps the error; the other streams are unaffected.
 *   - Everything else is word for word RE-CODING BATCHES: failed streams, the capacity rule and nothing written at or beyond
 *     min(cap, out_off[n]), count-only mode, the index-free walk with its d_sym_off output, the workspace rule
 *     (mh_dev_recode_edit_workspace), alignment, no allocation, no host synchronisation and a number of launches that does not
 *     depend on the data.  With an empty span list, or the identity map, the output is mh_dev_recode_batch's byte for byte.
 *   - mh_dev_recode_edit_each: stream i under the set's model i (n_streams == mh_model_set_size(src), else MH_ERR_ARG); a
 *     bank view of mh_dev_model_set_pick is a set.
 *   - Host form mh_recode_edit_batch: arguments checked before a device is touched (span_off as any offsets), spans and map
 *     taken from host memory, the rest as mh_recode_batch (index-free streams over MH_BATCH_WALK_MAX_BITS are indexed first).
 * Spans from search records.  mh_spans_from_hits (host, no device) and mh_dev_spans_from_hits take the records of any find
 * call of this library — d_hit_off[n + 1], d_hits[3r ..] = (stream, begin, end) and the same hit_cap, in the documented order,
 * ascending (stream, end, pattern) — and write the union of each stream's intervals as maximal spans, overlapping or touching
 * records merged: d_span_off[n + 1] in full and at most hit_cap pairs in d_spans.  Begins are not monotonic in that order (a
 * longer pattern that ends later may begin earlier); with M(r) the least begin over the stream's records r' >= r, records
 * r - 1 and r lie in different spans exactly when end(r - 1) < M(r), and a span is (M(first), end(last)).
 *   - d_hit_off[n] > hit_cap: the search overflowed and a redaction from it would be silently incomplete: MH_ERR_CAPACITY
 *     (device form: through mh_dev_status(d_ws)), d_span_off all zeros, no span written.
 *   - Device form: no allocation, no host synchronisation, a fixed number of launches whose grids are sized from hit_cap and
 *     n_streams; d_ws 16-byte aligned, at least mh_dev_spans_from_hits_workspace(n, hit_cap) bytes (per record).  Bad offsets
 *     or a record of a stream >= n: MH_ERR_ARG through mh_dev_status(d_ws).
 * --------------------------------------------------------------------------------------------------------------------- */
int mh_spans_from_hits(const uint64_t *hit_off, const uint64_t *hits, uint64_t hit_cap, size_t n_streams, uint64_t *span_off,
                       uint64_t *spans);
size_t mh_dev_spans_from_hits_workspace(size_t n_streams, uint64_t hit_cap);
int mh_dev_spans_from_hits(const uint64_t *d_hit_off, const uint64_t *d_hits, uint64_t hit_cap, size_t n_streams,
                           uint64_t *d_span_off, uint64_t *d_spans, void *d_ws, size_t ws_bytes, void *stream);
size_t mh_dev_recode_edit_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
int mh_dev_recode_edit_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                             const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                             uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                             const uint64_t *d_spans, const uint8_t *d_map, uint8_t *d_out_payload, size_t cap,
                             uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
                             int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_recode_edit_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                            const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                            uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                            const uint64_t *d_spans, const uint8_t *d_map, uint8_t *d_out_payload, size_t cap,
                            uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_index, uint64_t *d_dropped,
                            int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_recode_edit_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                         const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                         uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans, const uint8_t *map,
                         uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index,
                         uint64_t *dropped, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * SPLICING BATCHES (extension, parity unpinned) — an edit that changes lengths while re-coding: every span of a record is
 * deleted or replaced by one replacement string of any length up to MH_SPLICE_MAX_REP, and the record is coded under dst,
 * which may be the source model itself.  The bytes are never written.  Order 0 and order 1 on both sides, independently; an
 * order-2 model on either side is MH_ERR_ARG before any launch.
 *   - Span lists are exactly EDITING BATCHES': d_span_off[n + 1] and (begin, end) pairs, ascending and disjoint within a
 *     stream (begin < end <= next begin; touching spans are legal).  d_span_off == NULL is MH_ERR_ARG: "everything inside"
 *     has no meaning for a splice.  A malformed list fails its stream alone with MH_ERR_ARG, bad offsets stop the call, as there.
 *   - Replacement: d_rep, rep_len bytes on the device, rep_len 0 .. MH_SPLICE_MAX_REP (more: MH_ERR_ARG).  0 deletes, and
 *     d_rep may then be NULL (NULL with rep_len > 0: MH_ERR_ARG).  One replacement serves the whole call.
 *   - Edited message.  Let x be stream i's message as the batch decoder returns it.  y is x with every span whose
 *     begin < len(x) replaced by rep, the span's end clipped to len(x).  A span that begins at or beyond the length is
 *     ignored (an index-free caller does not know the length).
 *   - Output.  For every stream whose verdict is MH_OK the output equals what mh_dev_encode_batch(dst) writes for y with the
 *     same chunk_symbols: d_out_off, d_out_nbits, the payload bytes; d_dropped (pairs of y without a code under dst are
 *     skipped while the context advances, pairs inside or at the edges of the replacement included); d_out_sym_off[n + 1]
 *     (required), the exclusive scan of len(y); and, when d_out_index is given, the index slices at entry
 *     (out_sym_off[i] >> log2 chunk) + i + k, one per started chunk of y, with context byte y[start - 1] (prev0 first) and
 *     the stream-relative bit: mh_batch_index_base(out_sym_off[i], i, chunk).  Gap entries are untouched.  A stream that
 *     becomes empty has nbits 0 and no entry.
 *   - Failed streams (the batch decoders' verdicts, plus MH_ERR_ARG for a bad list) have len(y) = 0, nbits 0, no payload
 *     byte, no index entry and dropped 0.  Index-free: the source's d_sym_off is written as mh_dev_recode_batch writes it;
 *     sym_total is ignored (index_cap bounds the destination index).
 *   - Capacity.  out_off[n] > cap, or a d_out_index with (out_sym_off[n] >> log2 chunk) + n > index_cap entries needed:
 *     MH_ERR_CAPACITY through mh_dev_status(d_ws); nothing is written at or beyond the caps, neither payload nor index is
 *     written, and the offsets, bit counts, dropped counts and out_sym_off are valid, so the caller can size a second call.
 *     d_out_payload == NULL: count only (cap ignored).
 *   - With an empty span list the payload, offsets, bit counts, dropped counts and index are mh_dev_recode_batch's byte for
 *     byte, and out_sym_off == sym_off.
 *   - No allocation, no host synchronisation; the number of launches depends on rep_len == 0 and on indexed versus
 *     index-free, never on the data.  d_ws 16-byte aligned, at least mh_dev_recode_splice_workspace(n, sym_total,
 *     chunk_symbols, n_spans) bytes (chunk_symbols 0: index-free): per chunk number, per stream and, for the deletion's
 *     look-back, per span.  A deletion (rep_len 0) of an indexed batch with more spans than the workspace was sized for is
 *     MH_ERR_CAPACITY through mh_dev_status(d_ws).
 *   - mh_dev_recode_splice_each: stream i under the set's model i (n_streams == mh_model_set_size(src), else MH_ERR_ARG).
 *   - Host form mh_recode_splice_batch: arguments checked before a device is touched, spans and rep taken from host memory,
 *     out_index (may be NULL) with index_cap entries, the rest as mh_recode_edit_batch (index-free streams over
 *     MH_BATCH_WALK_MAX_BITS are indexed first).
 * Left out of this call: order 2; pure insertions (begin == end); a replacement per span or per pattern.  The last two are
 * SPLICING WITH A REPLACEMENT TABLE below (this call keeps refusing begin == end); order 2 is built in neither.
 * --------------------------------------------------------------------------------------------------------------------- */
#define MH_SPLICE_MAX_REP 255u
size_t mh_dev_recode_splice_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, uint64_t n_spans);
int mh_dev_recode_splice_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                               const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                               uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                               const uint64_t *d_spans, const uint8_t *d_rep, uint32_t rep_len, uint8_t *d_out_payload,
                               size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_sym_off,
                               uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped, int32_t *d_stream_status,
                               void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_recode_splice_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload, const uint64_t *d_pay_off,
                              const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off,
                              uint64_t sym_total, const uint64_t *d_index, uint32_t chunk_symbols, const uint64_t *d_span_off,
                              const uint64_t *d_spans, const uint8_t *d_rep, uint32_t rep_len, uint8_t *d_out_payload,
                              size_t cap, uint64_t *d_out_off, uint64_t *d_out_nbits, uint64_t *d_out_sym_off,
                              uint64_t *d_out_index, uint64_t index_cap, uint64_t *d_dropped, int32_t *d_stream_status,
                              void *d_ws, size_t ws_bytes, void *stream);
int mh_recode_splice_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                           const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                           uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans, const uint8_t *rep,
                           uint32_t rep_len, uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits,
                           uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap, uint64_t *dropped,
                           int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * SPLICING WITH A REPLACEMENT TABLE (extension, parity unpinned) — the splice with a replacement per span, chosen by a tag,
 * and with insertions: `<EMAIL>` where one pattern hit, `<IP>` where another did, a third deleted, in one pass.  The
 * arguments are mh_dev_recode_splice_batch's with d_rep, rep_len replaced by d_span_tag, d_rep_off, d_rep_bytes, n_reps.
 *   - Table.  Replacement k is d_rep_bytes[d_rep_off[k] .. d_rep_off[k + 1]), 0 .. MH_SPLICE_MAX_REP bytes; length 0 deletes.
 *     d_rep_off has n_reps + 1 entries (required); d_rep_bytes may be NULL when d_rep_off[n_reps] is 0.  d_rep_off[0] != 0,
 *     decreasing offsets, an entry longer than MH_SPLICE_MAX_REP, or n_reps == 0 together with a non-empty span list:
 *     MH_ERR_ARG through mh_dev_status(d_ws) and the call stops with nothing else written, as for bad d_pay_off.
 *   - Tags.  d_span_tag[r] (required), parallel to d_spans, names span r's replacement.  A span whose tag is >= n_reps fails
 *     its stream alone with MH_ERR_ARG, as a malformed list does.
 *   - Span rule.  In this call: begin <= end <= next begin.  begin == end is an insertion in front of x[begin].  Several
 *     insertions at one position, and an insertion touching a span on either side, are legal; they take effect in list
 *     order.  (p, q), (p, p) with q > p is malformed.  An insertion with an empty replacement is a no-op.  A span or an
 *     insertion with begin >= len(x) is ignored.
 *   - Edited message.  y is x with every span that begins inside the message replaced by its tagged replacement, the end
 *     clipped to len(x).
 *   - Everything else is SPLICING BATCHES word for word: the output is byte for byte what mh_dev_encode_batch(dst) writes for
 *     y; d_dropped (pairs inside and at the edges of every replacement included), d_out_sym_off and the index slices by
 *     output position; failed streams, both capacity limits, count-only mode, index-free sources through the one-lane walk;
 *     order 0 and 1 on both sides, a shared source or a model set (_each); order 2 is MH_ERR_ARG before any launch; no
 *     allocation, no host synchronisation.
 *   - Launches.  The host does not know which table entries are empty, so an indexed call always runs the deletion's
 *     look-back: the number of launches depends on indexed versus index-free alone, never on the data or the table.  d_ws:
 *     at least mh_dev_recode_splice_table_workspace(n, sym_total, chunk_symbols, n_spans, n_reps) bytes, 8 more per
 *     replacement than the splice's; an indexed batch with more spans than the workspace was sized for is MH_ERR_CAPACITY
 *     through mh_dev_status(d_ws).
 *   - Equivalence.  With every tag 0, a one-entry table and no insertion every output equals mh_dev_recode_splice_batch's
 *     with that replacement, byte for byte.
 *   - Host form mh_recode_splice_table_batch: all of the table's rules (n_reps == 0 with spans included) are checked before
 *     a device is touched and are MH_ERR_ARG; spans, tags and table taken from host memory; the rest as
 *     mh_recode_splice_batch.
 * Tagged spans.  mh_spans_from_hits_tagged, mh_dev_spans_from_hits_tagged (workspace: _tagged_workspace, the untagged
 * call's) take the arguments of the untagged calls and hit_pattern (required: NULL is MH_ERR_ARG), write span_off and spans
 * exactly as those do, and span_tag[r]: the LOWEST pattern number among the records merged into span r.  The caller sets
 * priority by pattern order (the CLI: the earlier line of the pattern file wins).  Overflow and bad offsets as untagged; the
 * device form keeps its guarantees (no allocation, no host synchronisation, a fixed number of launches).
 * Left out: order 2 on either side; appending at len(x) (a span that begins there is ignored); replacements longer than
 * MH_SPLICE_MAX_REP; back-references (a table computed from the matched bytes is TOKENS FROM MATCHED BYTES below).
 * --------------------------------------------------------------------------------------------------------------------- */
int mh_spans_from_hits_tagged(const uint64_t *hit_off, const uint64_t *hits, const uint32_t *hit_pattern, uint64_t hit_cap,
                              size_t n_streams, uint64_t *span_off, uint64_t *spans, uint32_t *span_tag);
size_t mh_dev_spans_from_hits_tagged_workspace(size_t n_streams, uint64_t hit_cap);
int mh_dev_spans_from_hits_tagged(const uint64_t *d_hit_off, const uint64_t *d_hits, const uint32_t *d_hit_pattern,
                                  uint64_t hit_cap, size_t n_streams, uint64_t *d_span_off, uint64_t *d_spans,
                                  uint32_t *d_span_tag, void *d_ws, size_t ws_bytes, void *stream);
size_t mh_dev_recode_splice_table_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols, uint64_t n_spans,
                                            size_t n_reps);
int mh_dev_recode_splice_table_batch(const mh_model *src, const mh_model *dst, const uint8_t *d_payload,
                                     const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total,
                                     uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                                     uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans,
                                     const uint32_t *d_span_tag, const uint64_t *d_rep_off, const uint8_t *d_rep_bytes,
                                     size_t n_reps, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off,
                                     uint64_t *d_out_nbits, uint64_t *d_out_sym_off, uint64_t *d_out_index, uint64_t index_cap,
                                     uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_recode_splice_table_each(const mh_model_set *src, const mh_model *dst, const uint8_t *d_payload,
                                    const uint64_t *d_pay_off, const uint64_t *d_nbits, size_t n_streams, uint64_t pay_total,
                                    uint8_t prev0, uint64_t *d_sym_off, uint64_t sym_total, const uint64_t *d_index,
                                    uint32_t chunk_symbols, const uint64_t *d_span_off, const uint64_t *d_spans,
                                    const uint32_t *d_span_tag, const uint64_t *d_rep_off, const uint8_t *d_rep_bytes,
                                    size_t n_reps, uint8_t *d_out_payload, size_t cap, uint64_t *d_out_off,
                                    uint64_t *d_out_nbits, uint64_t *d_out_sym_off, uint64_t *d_out_index, uint64_t index_cap,
                                    uint64_t *d_dropped, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_recode_splice_table_batch(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                                 const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off,
                                 const uint64_t *index, uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans,
                                 const uint32_t *span_tag, const uint64_t *rep_off, const uint8_t *rep_bytes, size_t n_reps,
                                 uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits,
                                 uint64_t *out_sym_off, uint64_t *out_index, uint64_t index_cap, uint64_t *dropped,
                                 int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * ORDER 2 IN EDITING AND SPLICING (extension, parity unpinned) — the masked re-code and the table splice with an order-2
 * model on a side, so that a store kept under order 2 is scrubbed as it is searched: compressed.  The contract is that of
 * mh_dev_recode_edit_batch and mh_dev_recode_splice_table_batch word for word, except for what follows.  x is stream i's
 * message as the source's batch decoder returns it (mh_dev_decode_batch_o2 for an order-2 source).
 *   - Orders.  Edit: source -> destination 2 -> 2, 2 -> 1, 2 -> 0, 1 -> 2, 0 -> 2.  Table splice: an order-2 source under any
 *     destination (2 -> 2, 2 -> 1, 2 -> 0).  Order 0/1 on both sides stays with the calls above and is MH_ERR_ARG here, as is
 *     a table splice of an order-0/1 source under an order-2 destination (left out: mh_dev_recode_batch_o2 to order 2 first
 *     is one call).  Shared models only: src and dst are `const mh_model *` members and the calls have no model-set
 *     parameter, so a set cannot be passed and there is no _each form.
 *   - Output.  For every stream whose verdict is MH_OK, byte for byte what mh_dev_encode_batch_o2(dst) writes for y under an
 *     order-2 dst and what mh_dev_encode_batch(dst) writes under an order-0/1 dst: offsets, bit counts, payload and index
 *     slices in dst's entry format, for the splice also d_out_sym_off and an index laid out by output positions.  An order-2
 *     entry carries (y[s - 2], y[s - 1]) of the OUTPUT; prev0 stands for every position in front of 0.
 *   - Drops.  A symbol whose (context, symbol) has no code under dst is skipped and counted in d_dropped[i] while the
 *     destination context advances; the bytes of a replacement and both of its edges are included.
 *   - Equivalence.  With an empty span list or the identity map every output equals mh_dev_recode_batch_o2's byte for byte.
 *   - A single replacement is a one-entry table with every tag 0: there is no separate single-replacement call.
 *   - Everything else is the calls' above: the batch decoders' verdicts and failed streams left empty; MH_ERR_ARG for a
 *     stream whose span list is malformed or whose tag is out of range, for that stream alone; both capacity rules and
 *     count-only mode; index-free sources through the one-lane walk, which writes d_sym_off; no allocation, no host
 *     synchronisation, and a number of launches that depends on indexed versus index-free alone.
 *   - Workspaces.  mh_dev_recode_edit_batch_o2_workspace is mh_dev_recode_batch_o2_workspace: the edit call's and 8 bytes
 *     per chunk number for the seam of an order-0/1 source.  mh_dev_recode_splice_table_batch_o2_workspace is
 *     mh_dev_recode_splice_table_workspace: nothing new per chunk or per span.
 * The argument block.  The two device calls take one struct instead of thirty positional parameters: a call with more than
 * thirty positional pointers of a few types is the least safe thing in this header, and the declarations with a positional
 * `void *stream` are a closed, counted set whose stream order one test module drives; the calls that take a block are
 * counted and driven on a non-default stream by a module of their own.  The members are the positional calls' parameters
 * under the same names and in the same order, the batch's as one nested mh_coded_batch_args.  struct_size must equal
 * sizeof of the struct, else MH_ERR_ARG (the block can grow later); a NULL block is MH_ERR_ARG; without a device
 * MH_ERR_NO_DEVICE.  Order rules, struct_size, a NULL d_map and the required pointers are refused before any launch.
 * Host forms mh_recode_edit_batch_o2 and mh_recode_splice_table_batch_o2: positional, host pointers, the rules checked
 * before a device is touched, the rest as mh_recode_edit_batch and mh_recode_splice_table_batch, except that EVERY index-free
 * batch is indexed first (mh_index_batch_o2 for an order-2 source, mh_index_batch for an order-0/1 source; with the chunk
 * size of out_index when the call writes one) and edited as an indexed batch: sym_off is written as before, and a valid batch
 * is never refused for a stream over MH_BATCH_WALK_MAX_BITS.
 * Left out: the CLI (--order2 with --recode or --redact stays refused); model sets; the table splice of an order-0/1 source
 * under an order-2 destination; and everything the table splice leaves out: appending at len(x), replacements longer than
 * MH_SPLICE_MAX_REP, back-references (a table computed from the matched bytes is TOKENS FROM MATCHED BYTES below).
 * --------------------------------------------------------------------------------------------------------------------- */
typedef struct mh_coded_batch_args {
    const uint8_t *d_payload;
    const uint64_t *d_pay_off;
    const uint64_t *d_nbits;
    size_t n_streams;
    uint64_t pay_total;
    uint8_t prev0;
    uint64_t *d_sym_off;
    uint64_t sym_total;
    const uint64_t *d_index;
    uint32_t chunk_symbols;
} mh_coded_batch_args;
typedef struct mh_recode_edit_o2_args {
    uint32_t struct_size;
    const mh_model *src;
    const mh_model *dst;
    mh_coded_batch_args batch;
    const uint64_t *d_span_off;
    const uint64_t *d_spans;
    const uint8_t *d_map;
    uint8_t *d_out_payload;
    size_t cap;
    uint64_t *d_out_off;
    uint64_t *d_out_nbits;
    uint64_t *d_out_index;
    uint64_t *d_dropped;
    int32_t *d_stream_status;
    void *d_ws;
    size_t ws_bytes;
    void *stream;
} mh_recode_edit_o2_args;
typedef struct mh_recode_splice_o2_args {
    uint32_t struct_size;
    const mh_model *src;
    const mh_model *dst;
    mh_coded_batch_args batch;
    const uint64_t *d_span_off;
    const uint64_t *d_spans;
    const uint32_t *d_span_tag;
    const uint64_t *d_rep_off;
    const uint8_t *d_rep_bytes;
    size_t n_reps;
    uint8_t *d_out_payload;
    size_t cap;
    uint64_t *d_out_off;
    uint64_t *d_out_nbits;
    uint64_t *d_out_sym_off;
    uint64_t *d_out_index;
    uint64_t index_cap;
    uint64_t *d_dropped;
    int32_t *d_stream_status;
    void *d_ws;
    size_t ws_bytes;
    void *stream;
} mh_recode_splice_o2_args;
size_t mh_dev_recode_edit_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols);
size_t mh_dev_recode_splice_table_batch_o2_workspace(size_t n_streams, uint64_t sym_total, uint32_t chunk_symbols,
                                                     uint64_t n_spans, size_t n_reps);
int mh_dev_recode_edit_batch_o2(const mh_recode_edit_o2_args *a);
int mh_dev_recode_splice_table_batch_o2(const mh_recode_splice_o2_args *a);
int mh_recode_edit_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                            const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off, const uint64_t *index,
                            uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans, const uint8_t *map,
                            uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_index,
                            uint64_t *dropped, int32_t *stream_status);
int mh_recode_splice_table_batch_o2(const mh_model *src, const mh_model *dst, const uint8_t *payload, const uint64_t *pay_off,
                                    const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint64_t *sym_off,
                                    const uint64_t *index, uint32_t chunk_symbols, const uint64_t *span_off,
                                    const uint64_t *spans, const uint32_t *span_tag, const uint64_t *rep_off,
                                    const uint8_t *rep_bytes, size_t n_reps, uint8_t *out_payload, size_t cap,
                                    uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off, uint64_t *out_index,
                                    uint64_t index_cap, uint64_t *dropped, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * SELECTING RECORDS OF BATCHES (extension, parity unpinned) — a compressed batch is a record store, and these calls change
 * which records it holds without decoding one: keep the records a search hit (grep with compressed output), drop them, drop
 * the records whose verdict is not MH_OK, put the records in another order, append one batch to another.  Every stream of a
 * batch is byte-aligned and self-contained, so its payload bytes move as they are.  Its index slice cannot be moved by
 * hand: slice i sits at mh_batch_index_base(sym_off[i], i, chunk) = sym_off[i] / chunk + i, so moving, dropping or appending
 * one record shifts every slice behind it by an amount that depends on all symbol counts in front, and two batches' index
 * arrays laid end to end are silently wrong.  This section does that relocation.
 * Model-free: no model is passed and nothing is decoded, so the calls serve batches under a shared order-0/1 model, an
 * order-2 model, a model set or a bank view alike; index entries are copied as 64-bit words whatever their format.
 *   - Sources.  `sources` is a HOST array of n_sources = 1 .. MH_SELECT_MAX_SOURCES batch descriptions (their pointers are
 *     device pointers in the device call, host pointers in the host form); it is copied into the kernel arguments and may
 *     be freed when the call returns.  prev0 is ignored.  d_sym_off and d_index may be NULL per source; d_payload may be
 *     NULL when pay_total is 0 or nothing is gathered (count only).  0 sources or more than 8: MH_ERR_ARG.
 *   - Picks.  d_picks[n_picks]: pick j is (source << 56) | stream.  MH_SELECT_NONE (all ones) yields an empty output stream
 *     with status MH_OK.  Repeats and any order are allowed; n_picks may be 0.
 *   - Output.  The output batch is byte for byte what the batch encoder of the sources' model (mh_dev_encode_batch,
 *     mh_dev_encode_batch_o2, mh_dev_encode_each) writes for the picked messages in pick order: d_out_nbits[j] is copied,
 *     d_out_off[n_picks + 1] is the exclusive scan of ceil(nbits / 8), the payload is the first ceil(nbits / 8) bytes of
 *     the source stream, d_out_sym_off[n_picks + 1] is the scan of the symbol counts (written when every source has
 *     d_sym_off, else it must be NULL: MH_ERR_ARG), and slice j (ceil(m_j / chunk) entries) is copied to
 *     mh_batch_index_base(out_sym_off[j], j, chunk).  Index entries in the gaps between slices are left untouched.  No
 *     payload byte is written at or behind out_off[n_picks] rounded up to 16, or at or behind cap, whichever is smaller.
 *   - Index.  An index is written only when every source has d_sym_off and a d_index with this same chunk_symbols (the
 *     block's; a power of two in [MH_CHUNK_MIN, MH_CHUNK_MAX]); otherwise a non-NULL d_out_index is MH_ERR_ARG before any
 *     launch.  d_out_index == NULL: no index is written and chunk_symbols is ignored.
 *   - Checks on the device.  Every source's offsets are checked as the batch decoders check them (d_pay_off[0] == 0,
 *     [n] == pay_total, non-decreasing; the same of d_sym_off with sym_total when given): a failure is MH_ERR_ARG through
 *     mh_dev_status(d_ws) and the call stops.  A pick whose source or stream number is out of range gets MH_ERR_ARG in
 *     d_pick_status[j] (may be NULL) for that pick alone and an empty output stream; so does a pick whose nbits exceeds 8 x
 *     its payload bytes.  The other picks are unaffected; mh_dev_status(d_ws) keeps the first error.
 *   - Capacity.  out_off[n_picks] > cap, or mh_batch_index_capacity(out_sym_off[n_picks], n_picks, chunk) > index_cap with
 *     an index: MH_ERR_CAPACITY through mh_dev_status(d_ws); offsets, lengths and statuses are still written, neither payload
 *     nor index is.  d_out_payload == NULL: count only (cap ignored).
 *   - Pointer, size and n_sources rules are refused before any launch: a NULL block, struct_size other than sizeof of the
 *     struct (the block can grow later), NULL sources, d_picks (with n_picks > 0), d_out_off, d_out_nbits or d_ws, a source
 *     without d_pay_off, d_nbits or (when payload is gathered and pay_total > 0) d_payload, d_out_payload or d_ws not 16-byte
 *     aligned: MH_ERR_ARG; a workspace below mh_dev_select_batch_workspace: MH_ERR_CAPACITY.  Without a device:
 *     MH_ERR_NO_DEVICE.
 *   - The call allocates nothing and makes no host synchronisation; the number of launches depends only on count-only versus
 *     full and on whether an index is written.  All arithmetic is 64-bit.  The outputs must not overlap the sources.
 *   - Side information.  What the caller keeps per stream beside the batch — bank entry numbers for mh_dev_model_set_pick,
 *     CRCs, keys — is gathered by the caller with the same pick list.
 * mh_dev_picks_from_hits turns a per-stream predicate into a pick list without a host wait.  Stream i of n_streams is kept
 * iff d_hit_off (n + 1, from any find call; may be NULL) is NULL or the stream has at least one hit — with
 * MH_PICKS_WITHOUT_HITS in flags: has none — and d_stream_status (n, may be NULL) is NULL or d_stream_status[i] == MH_OK.
 * d_picks[n_streams] gets the kept streams in ascending order as picks of `source` (< MH_SELECT_MAX_SOURCES), then
 * MH_SELECT_NONE up to n; d_n_kept (one uint64) their number.  The trailing empty streams leave every prefix of the selected
 * batch a valid batch of n_kept streams, so the caller passes n_picks = n_streams at once and trims when it later reads
 * n_kept.  Unknown flag bits, NULL d_picks (n > 0), d_n_kept or d_ws: MH_ERR_ARG.
 * The launch context.  The declarations with a positional `void *stream` and the argument blocks with a `void *stream`
 * member are two closed, counted sets, each driven on a non-default stream by a test module of its own.  The calls of this
 * section take a block whose workspace and stream are one nested mh_launch, as the batch is a nested mh_coded_batch_args; a
 * third module counts and drives them.  The promise is the same: stream-ordered, no allocation, no synchronisation.
 * Host forms mh_select_batch and mh_picks_from_hits: positional, host pointers, plain C++ — no device is needed, as for
 * mh_spans_from_hits.  Results and verdicts are the device calls'; they return the first pick's error, else MH_ERR_CAPACITY.
 * Left out: the CLI; re-ordering the tables of a per-stream model set (the caller re-indexes its set); selecting in place;
 * sources whose index chunk sizes differ.
 * --------------------------------------------------------------------------------------------------------------------- */
#define MH_SELECT_MAX_SOURCES 8u
#define MH_SELECT_NONE        0xFFFFFFFFFFFFFFFFull
#define MH_PICKS_WITHOUT_HITS 1u
typedef struct mh_launch {
    void *d_ws;
    size_t ws_bytes;
    void *stream;
} mh_launch;
typedef struct mh_select_args {
    uint32_t struct_size;
    const mh_coded_batch_args *sources;
    uint32_t n_sources;
    const uint64_t *d_picks;
    size_t n_picks;
    uint8_t *d_out_payload;
    size_t cap;
    uint64_t *d_out_off;
    uint64_t *d_out_nbits;
    uint64_t *d_out_sym_off;
    uint64_t *d_out_index;
    uint64_t index_cap;
    uint32_t chunk_symbols;
    int32_t *d_pick_status;
    mh_launch launch;
} mh_select_args;
typedef struct mh_picks_args {
    uint32_t struct_size;
    const uint64_t *d_hit_off;
    const int32_t *d_stream_status;
    size_t n_streams;
    uint32_t source;
    uint32_t flags;
    uint64_t *d_picks;
    uint64_t *d_n_kept;
    mh_launch launch;
} mh_picks_args;
size_t mh_dev_select_batch_workspace(size_t total_source_streams, size_t n_picks);
int mh_dev_select_batch(const mh_select_args *a);
size_t mh_dev_picks_from_hits_workspace(size_t n_streams);
int mh_dev_picks_from_hits(const mh_picks_args *a);
int mh_select_batch(const mh_coded_batch_args *sources, uint32_t n_sources, const uint64_t *picks, size_t n_picks,
                    uint8_t *out_payload, size_t cap, uint64_t *out_off, uint64_t *out_nbits, uint64_t *out_sym_off,
                    uint64_t *out_index, uint64_t index_cap, uint32_t chunk_symbols, int32_t *pick_status);
int mh_picks_from_hits(const uint64_t *hit_off, const int32_t *stream_status, size_t n_streams, uint32_t source, uint32_t flags,
                       uint64_t *picks, uint64_t *n_kept);

/* ---------------------------------------------------------------------------------------------------------------------
 * TOKENS FROM MATCHED BYTES (extension, parity unpinned) — pseudonymisation: a replacement table whose entry for span r is
 * computed from the bytes the span matched, so that a store scrubbed with `<EMAIL:9f3a61c2d07b4e15>` can still be joined,
 * counted and de-duplicated by the redacted value: equal bytes give equal tokens under a secret key, and the key cannot be
 * recovered from the tokens.  The matched bytes never reach memory: a lane decodes a symbol into a register, absorbs it
 * and drops it.  The table is what mh_dev_recode_splice_table_batch, _each and _batch_o2 take.
 *   - Digest.  SipHash-2-4 (64-bit result, 128-bit key: k0, k1 are the key's two little-endian words) of
 *     x[begin, min(end, len(x))), x being stream i's message as the source's batch decoder returns it.  With MH_TOKEN_FOLD in
 *     flags, ASCII A-Z are absorbed as a-z.  Other flag bits: MH_ERR_ARG.  mh_span_token_digest is the same function of a
 *     byte string in host memory (plain C++, no device): the token of a known value, to query a scrubbed store.
 *   - Formats.  Format f is (prefix, hex digits, suffix): d_fmt_off has 2 * n_formats + 1 entries, the prefix is
 *     d_fmt_bytes[d_fmt_off[2f] .. d_fmt_off[2f + 1]), the suffix d_fmt_bytes[d_fmt_off[2f + 1] .. d_fmt_off[2f + 2]), and
 *     d_hex_digits[f] is 0 .. 16.  A format longer than MH_SPLICE_MAX_REP in all, decreasing offsets, d_fmt_off[0] != 0,
 *     more than 16 digits, or n_formats == 0 with a non-empty span list: MH_ERR_ARG through mh_dev_status(d_ws) and the call
 *     stops, as for bad d_pay_off.
 *   - Token.  Span r's entry is prefix, the first hex_digits characters of "%016x" of the digest, suffix, under format
 *     d_span_tag[r] (a NULL tag array: format 0).  hex_digits 0 gives a constant entry, an empty format a deletion, so one
 *     call serves a mixed policy.
 *   - Output.  A table of n_reps entries, n_reps being the caller's bound on the spans (the hit_cap of the search):
 *     d_rep_off[n_reps + 1], the exclusive scan of the entry lengths, entries behind the last span empty; d_rep_bytes, at
 *     most rep_cap bytes (d_rep_off[n_reps] > rep_cap: MH_ERR_CAPACITY through mh_dev_status(d_ws), no byte written, the
 *     offsets valid; NULL: count only); d_rep_tag[r] = r for r < n_reps, the tag array of the splice; d_stream_status[n]
 *     (required).  The splice is then called with d_rep_tag as d_span_tag and this n_reps.
 *   - Span lists are the table splice's: begin <= end <= next begin.  A list that breaks the rule, or a tag >= n_formats,
 *     fails its stream alone with MH_ERR_ARG.  Every entry of a failed stream is empty.  A span with begin >= len(x) gets
 *     its format with the digest of the empty string (the splice ignores it).  More spans than n_reps
 *     (d_span_off[n] > n_reps): MH_ERR_CAPACITY through mh_dev_status(d_ws) and the call stops.
 *   - Indexed source.  One lane per span.  The lane starts at the index entry of chunk begin / chunk_symbols, decodes and
 *     drops the symbols in front, absorbs the span's symbols, and decodes on over chunk boundaries.  At every boundary it
 *     reaches, and at len(x), its bit position must equal the next entry's (nbits at the end): else MH_ERR_CORRUPT.
 *   - Index-free source.  One lane per stream walks from bit 0 in prev0, digests the stream's spans in list order and walks
 *     on to nbits.  Streams over MH_BATCH_WALK_MAX_BITS: MH_ERR_ARG.  d_sym_off is neither read nor written.
 *   - Verdicts.  ONLY THE STREAMS WITH SPANS ARE DECODED: a stream without spans gets MH_OK, whatever its payload holds.
 *     An index-free stream with spans gets the verdict of the batch decoder's walk.  An indexed stream with spans is judged
 *     on the chunks its spans touch, by the batch decoder's rules (entries against each other and nbits, a code that does
 *     not end, the bit position at a boundary): damage in a chunk no span touches is not seen.  nbits beyond the payload of
 *     a stream with spans: MH_ERR_ARG.  Bad d_pay_off, d_sym_off (under an index) or d_span_off stop the call.
 *   - Models.  Exactly one of src (a shared model of order 0, 1 or 2) and src_set (stream i under the set's model i,
 *     n_streams == mh_model_set_size, a bank view included) is given, else MH_ERR_ARG.
 *   - The call makes no allocation and no host synchronisation; the number of launches is the same for every call.  d_ws:
 *     16-byte aligned, at least mh_dev_span_tokens_workspace(n_streams, n_reps) bytes (8 per entry), else MH_ERR_CAPACITY.
 *   - The declaration.  The block says what is done, the mh_launch where: a shape of its own, counted and driven on a
 *     non-default stream by a test module of its own.  struct_size must equal sizeof of the struct; a NULL block or launch,
 *     NULL d_span_off, d_rep_off, d_rep_tag (n_reps > 0), d_stream_status (n_streams > 0), d_fmt_off or d_hex_digits
 *     (n_formats > 0): MH_ERR_ARG before any launch.  Without a device: MH_ERR_NO_DEVICE.
 *   - Host form mh_span_tokens_batch: positional, host pointers, a shared model; every rule of the formats and the offsets
 *     is checked before a device is touched (MH_ERR_ARG); n_reps is span_off[n_streams]; rep_off is required, rep_bytes NULL
 *     counts; an index-free batch with a stream over MH_BATCH_WALK_MAX_BITS is indexed first, and a stream that this
 *     indexing fails keeps that verdict and has empty entries, as every failed stream.  Returns the first failed stream's
 *     error, else MH_ERR_CAPACITY when the table does not fit.
 * Known limit: one lane per span is correct for any length but serial: a span of 64 KiB takes one lane's time for 64 KiB.
 * Left out: back-references and capture groups; tokens over MH_SPLICE_MAX_REP (255) bytes; de-duplicating equal table entries.
 * --------------------------------------------------------------------------------------------------------------------- */
#define MH_TOKEN_FOLD 1u
typedef struct mh_span_tokens_args {
    uint32_t struct_size;
    const mh_model *src;
    const mh_model_set *src_set;
    mh_coded_batch_args batch;
    const uint64_t *d_span_off;
    const uint64_t *d_spans;
    const uint32_t *d_span_tag;
    uint8_t key[16];
    uint32_t flags;
    const uint64_t *d_fmt_off;
    const uint8_t *d_fmt_bytes;
    const uint8_t *d_hex_digits;
    size_t n_formats;
    size_t n_reps;
    uint64_t *d_rep_off;
    uint8_t *d_rep_bytes;
    size_t rep_cap;
    uint32_t *d_rep_tag;
    int32_t *d_stream_status;
} mh_span_tokens_args;
uint64_t mh_span_token_digest(const uint8_t *key, const uint8_t *bytes, size_t n, uint32_t flags);
size_t mh_dev_span_tokens_workspace(size_t n_streams, size_t n_reps);
int mh_dev_span_tokens_batch(const mh_span_tokens_args *a, const mh_launch *launch);
int mh_span_tokens_batch(const mh_model *src, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                         size_t n_streams, uint8_t prev0, const uint64_t *sym_off, const uint64_t *index,
                         uint32_t chunk_symbols, const uint64_t *span_off, const uint64_t *spans, const uint32_t *span_tag,
                         const uint8_t *key, uint32_t flags, const uint64_t *fmt_off, const uint8_t *fmt_bytes,
                         const uint8_t *hex_digits, size_t n_formats, uint64_t *rep_off, uint8_t *rep_bytes, size_t rep_cap,
                         uint32_t *rep_tag, int32_t *stream_status);

/* ---------------------------------------------------------------------------------------------------------------------
 * SEGMENT STATES OF INDEX-FREE ORDER-2 BATCHES (extension, parity unpinned) — the _o2 twins of the segment-state calls of
 * the next section, for a batch coded under one shared order-2 model (what mh_dev_encode_batch_o2 writes, stored without
 * its sidecar index).  Same arguments, layouts, workspace arithmetic, launch sequence and guarantees as the twins; what
 * differs:
 *   - prev0 stands for both context bytes: every stream starts in context (prev0, prev0).
 *   - an order-0/1 model is MH_ERR_ARG before any launch (and the twins keep refusing an order-2 model).
 *   - a segment state is (two context bytes) << 48 | stream-relative bit, the order-2 index-entry format
 *     (MH_INDEX2_BIT_MASK masks the position); the index slices equal, byte for byte, those mh_dev_encode_batch_o2 writes
 *     (gap entries untouched), emit writes what the index-free mh_dev_decode_batch_o2 writes, and nothing is written at or
 *     beyond index_cap / out_cap.
 *   - a workspace that holds the states of an order-0/1 call, or of another batch, is refused by mh_dev_batch_index_o2 /
 *     mh_dev_batch_emit_o2 with MH_ERR_ARG, and an order-2 workspace by the order-0/1 calls.
 *   - the speculation differs.  Most of the 65536 contexts have no codes, so a guessed context dies almost at once.  A
 *     segment's entry guess therefore decodes the whole segment in front of it (512 bits) from context (prev0, prev0) and
 *     recovers: in a context without codes it goes on, at the same bit, in the model's heaviest context that ends in the
 *     same byte (or, where there is none, in (prev0, prev0) one bit further); when the bits match no code of a context
 *     that has some, it skips one bit.  Segment 1 is warmed up from the stream's true start and is exact.  Correctness
 *     never rests on the guess: the repair launches, the one-lane walk and the proof kernel are the twins'.
 *   - per-stream statuses and call-wide errors as for the twins; a stream whose fallback walk would exceed
 *     MH_BATCH_WALK_MAX_BITS is refused alone (MH_ERR_ARG).
 * mh_index_batch_o2 is the host form: a stream the device refuses is indexed alone by mh_dev_build_index (for an order-2
 * model a one-lane walk) and its slice moved into the batch layout, so a valid batch is never refused.
 * mh_find_batch_o2, mh_recode_batch_o2 and mh_decode_batch_o2 keep their own fallbacks for refused streams; moving them
 * onto this builder is a follow-up.
 * mh_dev_batch_states_stats (read-only, any order; synchronises the stream) says how the last states call in d_ws settled:
 * repair_passes_run = the repair launches (of 8) that rewrote a record, streams_walked = the streams the one-lane fallback
 * walked (refused ones included).  Exact outputs cannot show a silent degradation to the one-lane walk; this can.
 * MH_ERR_ARG when d_ws holds no states.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_batch_states_o2_workspace(size_t n_streams, uint64_t pay_total);
int mh_dev_batch_states_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                           size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status,
                           void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_batch_index_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                          size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap,
                          uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_batch_emit_o2(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                         size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                         int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_index_batch_o2(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits,
                      size_t n_streams, uint8_t prev0, uint32_t chunk_symbols, uint64_t *sym_off, uint64_t *index,
                      uint64_t index_cap, int32_t *stream_status);
int mh_dev_batch_states_stats(const void *d_ws, void *stream, uint32_t *repair_passes_run, uint64_t *streams_walked);

/* ---------------------------------------------------------------------------------------------------------------------
 * SEGMENT STATES OF INDEX-FREE BATCHES — the batch counterpart of mh_dev_build_index: the `.cm` files the reference writes
 * carry no index, and without one the batch decoders above walk each stream with one lane.  Three device steps for a batch
 * of index-free streams under one shared model (mh_dev_batch_*) or a model set (mh_dev_each_*; a bank view of
 * mh_dev_model_set_pick is a set): STATES, then INDEX and/or EMIT.  Order 0 and order 1; an order-2 model is MH_ERR_ARG
 * before any launch (its calls are the _o2 twins of the section above).  Payload layout, prev0, nbits and the index layout are those of the batch sections above.
 *   - states: every stream's payload is cut into 512-bit segments (segment k of stream i is number
 *     pay_off[i] * 8 / 512 + i + k, so a workspace of mh_dev_batch_states_workspace(n, pay_total) bytes holds every one).
 *     Each segment is decoded from a guessed entry state, a fixed number of repair launches decodes again the segments
 *     whose entry differs from their predecessor's end, and one lane per stream walks what is still inconsistent.  A
 *     check kernel then proves entry(k) == end(k - 1), entry(0) == (prev0, bit 0) and an end exactly at nbits_i
 *     (src/coding.cpp:124,158) for every stream.  d_sym_off[n + 1] (written) is the exclusive scan of the decoded
 *     lengths — what mh_dev_decode_batch writes index-free; the settled states stay in d_ws.
 *   - index: the chunk-index slices (mh_batch_index_base(sym_off[i], i, chunk)) from the settled states, each equal to
 *     the slice mh_dev_encode_batch / mh_dev_encode_each writes for that message; gap entries are left untouched.
 *     index_cap below mh_batch_index_capacity(sym_off[n], n, chunk): MH_ERR_CAPACITY, nothing written.
 *   - emit: every stream decoded to d_out[sym_off[i] ...) (16-byte aligned), byte for byte what mh_dev_decode_batch /
 *     mh_dev_decode_each write index-free; a stream that does not fit out_cap is MH_ERR_CAPACITY and writes nothing.
 *   - index and emit take the same batch arguments as the states call and the same d_ws, untouched in between: a workspace
 *     that holds the states of another batch, model or stream count gives MH_ERR_ARG through mh_dev_status(d_ws).
 *   - per-stream status d_stream_status[n] (may be NULL; the first error is kept): MH_ERR_ARG for nbits_i beyond its
 *     payload bytes, or for a stream whose sequential fallback walk would exceed MH_BATCH_WALK_MAX_BITS (fixed-length
 *     "lattice" codes, e.g. uniform bytes, never re-synchronise); MH_ERR_CORRUPT for a null table entry on the true path
 *     or a stream that does not end exactly at nbits_i; MH_ERR_CAPACITY (emit).  A failed stream decodes to 0 symbols in
 *     sym_off and never disturbs another stream.  mh_dev_status(d_ws): one of the errors.
 *   - call-wide errors, found on the device, stop the call and give every stream's status that error, nothing else being
 *     written: bad offsets (states) and a workspace without the states of this batch (index, emit) are MH_ERR_ARG, an
 *     index_cap below the capacity is MH_ERR_CAPACITY.
 *   - the fallback walk is refused by its span, not by the kind of code: it runs from a stream's first inconsistent
 *     segment to past its last one, so a long stream with two far-apart unsettled spots after the repair launches is
 *     refused (MH_ERR_ARG) like a lattice when that span exceeds MH_BATCH_WALK_MAX_BITS.
 * No allocation, no host synchronisation, and a number of launches that does not depend on the data.  d_payload and d_ws
 * 16-byte aligned.
 * Host forms: the batch is uploaded, states and index run on the device, sym_off[n] is read once; a stream the device
 * refuses goes through mh_dev_build_index on its own (its group maps handle lattices), so a valid batch is never refused.
 * sym_off[n + 1] and stream_status[n] (may be NULL) are written; index (index_cap entries, at least
 * mh_batch_index_capacity(sym_off[n], n, chunk), else MH_ERR_CAPACITY) gets the slices, gap entries keep their values.
 * mh_index_each parses stream i's table file (bytes [tab_off[i], tab_off[i+1]) of `tables`) with
 * mh_model_set_from_tables.  Offsets, nbits and the chunk size are checked before a device is touched; returns the first
 * stream's error, if any.
 * --------------------------------------------------------------------------------------------------------------------- */
size_t mh_dev_batch_states_workspace(size_t n_streams, uint64_t pay_total);
int mh_dev_batch_states(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                        size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status,
                        void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_each_states(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                       size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_sym_off, int32_t *d_stream_status,
                       void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_batch_index(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                       size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap,
                       uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_each_index(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                      size_t n_streams, uint64_t pay_total, uint8_t prev0, uint64_t *d_index, uint64_t index_cap,
                      uint32_t chunk_symbols, int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_batch_emit(const mh_model *m, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                      size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                      int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_dev_each_emit(const mh_model_set *s, const uint8_t *d_payload, const uint64_t *d_pay_off, const uint64_t *d_nbits,
                     size_t n_streams, uint64_t pay_total, uint8_t prev0, uint8_t *d_out, uint64_t out_cap,
                     int32_t *d_stream_status, void *d_ws, size_t ws_bytes, void *stream);
int mh_index_batch(const mh_model *m, const uint8_t *payload, const uint64_t *pay_off, const uint64_t *nbits, size_t n_streams,
                   uint8_t prev0, uint32_t chunk_symbols, uint64_t *sym_off, uint64_t *index, uint64_t index_cap,
                   int32_t *stream_status);
int mh_index_each(const uint8_t *tables, const uint64_t *tab_off, const uint8_t *payload, const uint64_t *pay_off,
                  const uint64_t *nbits, size_t n_streams, uint8_t prev0, uint32_t chunk_symbols, uint64_t *sym_off,
                  uint64_t *index, uint64_t index_cap, int32_t *stream_status);

#ifdef __cplusplus
}
#endif
#endif
