/*
 * tamp_amd.h -- C ABI of libtamp_amd.so: the MI355X-native batch codec for the Tamp `.tamp` format.
 *
 * This is the drop-in boundary for the reference's hot path.  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root).  Plain pointers and
 * sizes only; no torch / C++ types cross this boundary.  Every codec call runs hand-written HIP
 * kernels on a gfx950 device: there is no CPU fallback -- without a device the calls return
 * TAMP_AMD_NO_DEVICE (-20) and compute nothing.
 *
 * Status codes are the reference's tamp_res values (tamp/_c_src/tamp/common.h:145-168).
 */
#ifndef TAMP_AMD_H
#define TAMP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: identical numbering to tamp_res (common.h:145-168) ---- */
enum {
    TAMP_OK = 0,
    TAMP_OUTPUT_FULL = 1,
    TAMP_INPUT_EXHAUSTED = 2,
    TAMP_ERROR = -1,
    TAMP_EXCESS_BITS = -2,
    TAMP_INVALID_CONF = -3,
    TAMP_OOB = -4,
    TAMP_IO_ERROR = -10, /* stream API, common.h:160-163 */
    TAMP_READ_ERROR = -11,
    TAMP_WRITE_ERROR = -12,
    /* library-level failures of this implementation (outside the reference's range) */
    TAMP_AMD_NO_DEVICE = -20, /* no HIP device / HIP runtime error: nothing was computed */
    TAMP_AMD_BAD_ARGUMENT = -21,
    TAMP_AMD_BAD_INDEX = -22, /* tamp_batch_read_ranges: the reset index does not hold up on the segments a range touches */
};
typedef int8_t tamp_res;

#define TAMP_AMD_WINDOW_BITS_EXACT 0x80 /* flag for tamp_batch_decompress's max_window_bits: no header pre-pass */

/* Unpacked twin of TampConf (common.h:170-182).  One configuration per batch launch. */
typedef struct TampAmdConf {
    uint8_t window;                /* 8..15 */
    uint8_t literal;               /* 5..8  */
    uint8_t use_custom_dictionary; /* `dictionary` argument holds 1<<window bytes shared by all streams */
    uint8_t extended;              /* library default of the reference is 1 (compressor.c:193-203) */
    uint8_t dictionary_reset;      /* sets header bit0 and emits the zero second header byte */
    uint8_t lazy_matching;         /* compressor.c:576-619; a bit over half the default mode's speed */
    uint8_t input_hint;            /* TAMP_AMD_HINT_*: which build of the compress kernel parses a batch of SHORT messages
                                      (same bytes either way).  Streams of 1 KiB and more -- max_in_len given, or computed
                                      from in_len for host memory, 0 = unknown -- always take the run-aware build (round 3:
                                      it was the faster one on every kind of text, so the lean 256-thread builds are gone);
                                      shorter ones take the lean one-wavefront build unless the hint says RUNS. */
    uint8_t reserved;
} TampAmdConf;

enum {
    TAMP_AMD_HINT_AUTO = 0,
    TAMP_AMD_HINT_PLAIN = 1, /* lean build: every buffer position in the bigram index, every extended match searched;
                                the faster one for short messages (256-byte telemetry) and for data that is mostly runs */
    TAMP_AMD_HINT_RUNS = 2,  /* run-aware build: long runs of one byte (indentation, rulers, padding) are listed once
                                instead of being indexed byte by byte, extended matches without a rival are settled
                                without a window search: faster on streams of 1 KiB and more (config 2 by 5 %, source
                                code by 40 %) */
};

/* Where the data pointers of a batch call live. */
enum {
    TAMP_AMD_MEM_HOST = 0,   /* host pointers: the library stages H2D / D2H itself, in overlapping chunks on its
                                own streams; pinned memory (tamp_amd_host_alloc) lets both copy directions run
                                asynchronously at link speed, pageable memory works at the runtime's staging speed */
    TAMP_AMD_MEM_DEVICE = 1, /* device pointers on `device`: zero-copy, kernels only */
};

/* `device` argument of tamp_batch_compress / tamp_batch_decompress with host memory: cut the batch into one contiguous
 * range of streams per visible HIP device (balanced by input bytes) and run the ranges concurrently, one host thread
 * and one device each.  Streams are independent: no data moves between devices. */
#define TAMP_AMD_ALL_DEVICES (-1)

/* Page-locked host memory for TAMP_AMD_MEM_HOST calls, for callers that do not link the HIP runtime themselves
 * (cgo / JNI / ctypes).  Not in the reference: its buffers never leave the CPU.  NULL when the allocation fails. */
void *tamp_amd_host_alloc(size_t bytes);
void tamp_amd_host_free(void *p);

/* ---- host helpers (no device needed) -------------------------------------------------------- */

/* Replaces tamp_initialize_dictionary (common.h:395, common.c:37-52). */
void tamp_initialize_dictionary(unsigned char *buffer, size_t size, uint8_t literal);

/* Replaces tamp_compute_min_pattern_size (common.h:405, common.c:54-56). */
int8_t tamp_compute_min_pattern_size(uint8_t window, uint8_t literal);

/* Replaces tamp_window_copy (common.h:424, common.c:58-86): window[pos..pos+n) (wrapping with window_mask) <-
 * window[offset..offset+n) with memmove semantics; *window_pos advances.  Caller validates offset + n. */
void tamp_window_copy(unsigned char *window, uint16_t *window_pos, uint16_t window_offset, uint8_t match_size,
                      uint16_t window_mask);

/* Worst-case compressed size of an n-byte stream: header byte(s) + every byte a literal
 * (compressor.h flush table / SURVEY.md H7). */
size_t tamp_amd_compress_bound(size_t n, uint8_t literal, int dictionary_reset);

/* Number of visible HIP devices (0 when there is none), and the library version string. */
int tamp_amd_device_count(void);
const char *tamp_amd_version(void);

/* Text of the last HIP runtime failure seen by the calling thread ("" if none): what TAMP_AMD_NO_DEVICE meant. */
const char *tamp_amd_last_error(void);

/* How tamp_batch_compress would launch streams of up to `max_in_len` bytes (0 = unknown) at this window: positions matched
 * per epoch, LDS bytes per workgroup, threads per workgroup and the workgroups per CU its registers aim at (8 for the
 * run-aware builds, 6 lean, 5 lazy).  Pure host arithmetic -- no device needed; a diagnostics / capacity-planning call
 * (the reference has no counterpart: its state is the 16-byte ring + window of compressor.h:13-66).  It runs the launcher's own
 * planning code for a plain batch call with TAMP_AMD_HINT_AUTO (there is no hint parameter), so it honours the same tuning
 * variables as the launcher, TAMP_AMD_RUNS included.  Returns TAMP_OK or TAMP_AMD_BAD_ARGUMENT. */
int tamp_amd_compress_plan(uint8_t window_bits, uint32_t max_in_len, int lazy_matching, uint32_t *block_positions,
                           uint32_t *lds_bytes, uint32_t *threads, uint32_t *workgroups_per_cu);

/* Which build of the compress kernel a device batch call would take (host only, no GPU needed).  Whole-stream calls at
 * window 2^10, literal 8, default parse with 1,024-position blocks take a build with that geometry and the format compiled
 * in; ANY deviation -- and TAMP_AMD_FIXED_BUILD=0 in the environment -- takes the generic build.  Same bytes either way.
 * `call_flags`: what the call carries beyond a plain batch (TAMP_AMD_CALL_*); `dictionary_address`: the device address of
 * the custom dictionary (ignored without one).  -> TAMP_AMD_BUILD_*, or TAMP_AMD_BAD_ARGUMENT. */
enum {
    TAMP_AMD_CALL_STATE = 1,        /* a per-stream window state is passed (segment / piece calls) */
    TAMP_AMD_CALL_RESUME = 2,       /* ... and read at the start */
    TAMP_AMD_CALL_SAVE = 4,         /* ... and written back at the end */
    TAMP_AMD_CALL_FLUSH_TOKEN = 8,  /* the output ends with a FLUSH token */
    TAMP_AMD_CALL_PARTIAL = 16,     /* the call ends without a drain (piece calls) */
    TAMP_AMD_CALL_APPEND = 32,      /* FLUSH + padding lead the output instead of the plain header byte */
    TAMP_AMD_CALL_BLOCK_MODE = 64,  /* a handful of long v1 streams: each one's blocks over all workgroups */
    TAMP_AMD_CALL_DICT_TABLE = 128, /* a tamp_batch_compress_dicts call with dict_off: always a generic build (its table twin) */
};
enum { TAMP_AMD_BUILD_GENERIC = 0, TAMP_AMD_BUILD_FIXED_EXT = 1, TAMP_AMD_BUILD_FIXED_V1 = 2 };
int tamp_amd_compress_build(const TampAmdConf *conf, uint32_t max_in_len, uint32_t call_flags, uintptr_t dictionary_address);

/* Which decoder tamp_batch_decompress would take for a device batch and how it would size it (host only, no GPU needed: the CU
 * count is an input).  A diagnostics / capacity-planning call; it runs the launcher's own planning code -- the one reader of the
 * decode planning variables (TAMP_AMD_DECODER, TAMP_AMD_SPLIT_*, TAMP_AMD_SCRATCH_MB, TAMP_AMD_LONGDEC*) -- so it honours what
 * the launcher honours.  The caller supplies what the launcher learns on the device: the four words of the header pre-pass (read
 * only when the answer's `scan` is set), the free device memory and the bytes of split-decoder scratch the stream already holds.
 * Returns TAMP_OK or TAMP_AMD_BAD_ARGUMENT (a null pointer, no streams). */
typedef struct TampAmdDecodeQuery {
    uint64_t n_streams;
    uint8_t max_window_bits;   /* as passed to tamp_batch_decompress, TAMP_AMD_WINDOW_BITS_EXACT included */
    uint8_t has_dictionary;    /* a custom dictionary is passed */
    uint8_t exclude_split;     /* 1: the plan the launcher falls back to when the split decoder's scratch cannot be allocated */
    uint8_t free_known;        /* free_bytes holds the device's free memory (0: the runtime could not tell) */
    uint32_t cu_count;
    uint32_t scan_found;       /* pre-pass: largest window bits in the batch's headers, 0 = no valid header */
    uint32_t scan_longest_in;  /*           longest compressed stream */
    uint32_t scan_window_units; /*          sum of the streams' window sizes, in 256-byte units */
    uint32_t scan_max_out_cap; /*           largest out_cap */
    uint64_t free_bytes, held_bytes;
} TampAmdDecodeQuery;
enum { TAMP_AMD_DECODER_SPLIT = 0, TAMP_AMD_DECODER_WAVE = 1, TAMP_AMD_DECODER_LANE_LDS = 2, TAMP_AMD_DECODER_LANE_GLOBAL = 3 };
typedef struct TampAmdDecodePlan {
    /* the long-stream path (at most 16 streams): attempted at all; shortest stream it takes; extended streams; chained groups */
    uint32_t long_attempt, long_min_len, long_extended, long_chain;
    uint32_t scan;             /* the header pre-pass runs */
    uint32_t decoder;          /* TAMP_AMD_DECODER_* */
    uint32_t max_window_bits;  /* narrowed to the largest window the pre-pass found */
    uint32_t bulk;             /* streams of 512 compressed bytes and more (or unknown): the lane decoders' bulk builds */
    /* geometry of the chosen decoder; zeroes for the others */
    uint32_t split_tokcap, split_maxcap, split_wave_resolve, split_resolve_lds;
    uint32_t split_spw;        /* streams per parse wave in the first slice */
    uint32_t wave_waves, wave_lds, wave_groups; /* WAVE, and SPLIT (its leftovers): wavefronts per workgroup, LDS bytes, workgroups */
    uint32_t lane_lds_row, lane_lds, lane_per_cu, lane_grid;
    uint32_t global_slot, global_grid, global_bulk, global_lds;
    uint64_t split_slice, split_slab_bytes; /* streams per slice before any allocation failure halves it, scratch for that */
    uint64_t global_lanes, global_slab_bytes;
} TampAmdDecodePlan;
int tamp_amd_decompress_plan(const TampAmdDecodeQuery *query, TampAmdDecodePlan *plan);

/* ---- batch codec ---------------------------------------------------------------------------- */

/*
 * Compress n_streams independent streams.  Stream i's bytes are identical to what
 *     tamp_compressor_init(&c, &conf, window)                             (compressor.h:84)
 *     tamp_compressor_compress_and_flush(&c, out, cap, &w, in, n, &consumed, false)
 *                                                                         (compressor.h:280-286)
 * produce in the reference on a freshly initialised compressor -- the call every reference
 * benchmark times (tools/c-profiler/main.c:52-54, devices/common/tamp_bench.c:118-121) and that
 * tamp.compress() performs (tamp/_c_compressor.pyx:189-199).
 *
 *   in[in_off[i] .. in_off[i]+in_len[i])        input bytes of stream i
 *   out[out_off[i] .. out_off[i]+out_cap[i])    output slab of stream i
 *   out_len[i]                                  bytes produced.  Slab bytes behind out_len[i] are unspecified after
 *                                               the call when the slabs tile the output buffer back to back (host
 *                                               memory: the results come back in one transfer per chunk); with gaps
 *                                               between slabs or permuted offsets only the out_len[i] produced bytes
 *                                               of each slab are written, nothing else in the caller's buffer
 *   status[i]                                   TAMP_OK, TAMP_OUTPUT_FULL (slab too small), TAMP_EXCESS_BITS (a literal
 *                                               does not fit conf->literal bits, compressor.c:629-631; out_len[i] =
 *                                               whole bytes emitted before it), or TAMP_INVALID_CONF.
 *                                               TOO LITTLE ROOM, the rule of every build of the kernel -- this call,
 *                                               tamp_batch_compress_dicts, tamp_amd_compress and the segment / piece
 *                                               calls that finish a segment: let T be the stream's length and S
 *                                               its status with ample room (S = TAMP_EXCESS_BITS: T = the whole bytes
 *                                               in front of the offending literal).  Then
 *                                                 out_cap[i] <  T:  TAMP_OUTPUT_FULL, out_len[i] = out_cap[i], the
 *                                                                   slab holds the first out_cap[i] of the T bytes
 *                                                 out_cap[i] >= T:  S, out_len[i] = T, all T bytes
 *                                               -- room comes first: a stream with an offending literal behind more
 *                                               bytes than fit is TAMP_OUTPUT_FULL, and exact room (out_cap[i] == T)
 *                                               is enough.  Nothing is written at or behind
 *                                               out + out_off[i] + out_cap[i], in either memory kind.
 *                                               The REFERENCE with the same room is never more lenient and never
 *                                               ahead: whenever the rule says TAMP_OUTPUT_FULL so does it, its status
 *                                               is the rule's or TAMP_OUTPUT_FULL, and its bytes are a prefix of the
 *                                               bytes above.  But it gives up early: it asks for six free bytes before
 *                                               an extended-match token and one before every parse step, so with
 *                                               TAMP_OUTPUT_FULL it delivers up to 5 bytes fewer than min(out_cap[i],
 *                                               T), and it still reports TAMP_OUTPUT_FULL for out_cap[i] = T .. T + 3
 *                                               on some streams (also where S is TAMP_EXCESS_BITS).  From T + 4 on it
 *                                               and the rule agree (measured, tests/test_oracle_vs_reference.py; the
 *                                               bound is 8: its 32-bit bit buffer and one more token).
 *   dictionary                                  1<<window bytes shared by every stream when
 *                                               conf->use_custom_dictionary, else NULL (each stream starts from
 *                                               its own pristine copy)
 *   max_in_len                                  upper bound on in_len[] (sizes the per-workgroup LDS block); 0 = unknown:
 *                                               computed from in_len for host memory, 4096-position blocks for
 *                                               device memory (any length still works, in several epochs).  The bound
 *                                               ONLY sizes the block and picks the build: a stream longer than it is
 *                                               compressed to the same bytes, in more epochs (a device-memory call
 *                                               cannot check the bound, and a stale one costs speed, never bytes)
 *   mem                                         TAMP_AMD_MEM_HOST or TAMP_AMD_MEM_DEVICE: applies to ALL pointer
 *                                               arguments except conf
 *   device                                      HIP device ordinal
 *   stream                                      hipStream_t (as void*) to enqueue on, or NULL for the default
 *                                               stream.  With device memory the call is asynchronous on `stream`;
 *                                               with host memory the call is synchronous and runs on the
 *                                               library's own streams (`stream` is not used).
 *                                               ONE EXCEPTION to "asynchronous": a device-memory call of at most 64
 *                                               streams with max_in_len >= 256 KiB in the v1 format (extended = 0,
 *                                               literal = 8, default parse) reads the streams' table rows back and
 *                                               WAITS for `stream` once before it launches (block mode: one long
 *                                               stream over all workgroups) -- such a call cannot be captured in a
 *                                               hipGraph; the environment variable TAMP_AMD_BLOCK_MIN=0 turns block
 *                                               mode off and restores the asynchronous batch kernel for them.
 * Returns TAMP_OK when the batch was launched (per-stream results are in status[]), or a negative
 * library-level code.
 */
int tamp_batch_compress(const TampAmdConf *conf, const uint8_t *dictionary, const uint8_t *in, const uint64_t *in_off,
                        const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                        uint32_t *out_len, int8_t *status, size_t n_streams, uint32_t max_in_len, int mem, int device,
                        void *stream);

/*
 * Decompress n_streams independent `.tamp` streams.  Stream i's bytes and status are identical to
 *     tamp_decompressor_init(&d, NULL, window, max_window_bits)           (decompressor.h:83)
 *     tamp_decompressor_decompress(&d, out, cap, &w, in, n, &consumed)    (decompressor.h:128)
 * i.e. the configuration is read from each stream's own header (window 8..15 may differ per stream),
 * normal completion is TAMP_INPUT_EXHAUSTED (2) (decompressor.h:125-126), a full output slab with
 * work left is TAMP_OUTPUT_FULL (1), and malformed input yields TAMP_OOB / TAMP_INVALID_CONF
 * (decompressor.c:232-236,284,311,540-544) -- never a crash.
 *
 *   dictionary / dictionary_len   custom dictionary for streams whose header has the custom bit
 *                                 (>= 1<<window bytes, prefix used; such a stream with dictionary == NULL gets
 *                                 TAMP_INVALID_CONF, where the Python surface raises ValueError,
 *                                 tamp/_c_decompressor.pyx:63-64)
 *   max_window_bits               streams whose header asks for more get TAMP_INVALID_CONF (decompressor.c:311).  When it
 *                                 is above 8 the call first reads the headers of the batch (one tiny kernel and a
 *                                 4-byte copy, which waits for `stream`) to size the on-chip windows for the largest
 *                                 one actually present; OR in TAMP_AMD_WINDOW_BITS_EXACT to skip that and stay fully
 *                                 asynchronous (windows are then sized for max_window_bits itself)
 *   in_consumed                   optional (may be NULL): compressed bytes consumed per stream
 *   out_cap[i], TOO LITTLE ROOM   the rule of every batch decoder (wave, LDS lanes, slab lanes, split and what it hands back),
 *                                 and through it of tamp_batch_decoded_size with limit = out_cap: let (S, X, K) be the stream's
 *                                 status, bytes and in_consumed with ample room and N the length of X.  Then
 *                                   out_cap[i] <  N:  TAMP_OUTPUT_FULL, out_len[i] = out_cap[i], the slab holds the first
 *                                                     out_cap[i] bytes of X (a match, an RLE run or an extended match that
 *                                                     straddles the slab's end is delivered as far as it fits)
 *                                   out_cap[i] >  N:  exactly (S, X, K)
 *                                   out_cap[i] == N:  all of X, with status S or TAMP_OUTPUT_FULL: the reference asks whether
 *                                                     the output is full BEFORE it looks at the next token, so a stream that
 *                                                     ends in TAMP_OOB reports TAMP_OUTPUT_FULL here, and so does a clean
 *                                                     stream with pad bits left in its last byte; one whose last token ends
 *                                                     on a byte reports S
 *                                 in_consumed[i] never decreases as out_cap[i] grows, and never exceeds K.  All of it is the
 *                                 reference's own behaviour, capacity by capacity (tests/test_oracle_vs_reference.py).
 *   out, WHAT IS WRITTEN          nothing in front of a slab and nothing at or behind out + out_off[i] + out_cap[i], in either
 *                                 memory kind; only the out_len[i] produced bytes of a slab are written -- slab bytes behind
 *                                 out_len[i], gaps between slabs and whatever surrounds them keep their contents.  ONE
 *                                 EXCEPTION, as for tamp_batch_compress: a host-memory call whose slabs tile the output
 *                                 buffer back to back brings each chunk's extent home in one transfer and leaves the slab
 *                                 bytes behind out_len[i] unspecified; with gaps between slabs or permuted offsets only the
 *                                 produced bytes arrive.  (tests/test_gpu_tight_decode.py: every capacity 0 .. N + 2 of a
 *                                 stream at every slab alignment, the buffer compared whole, on every build of every decoder.)
 *   in_len[i]                     below 2^29 bytes (512 MiB) per stream: the decoders count bits in 32-bit registers;
 *                                 a longer stream gets status TAMP_AMD_BAD_ARGUMENT and produces nothing.  Feed longer
 *                                 streams in pieces through tamp_batch_decompress_resume, which looks at 2^28 bytes per
 *                                 call at most and reports what it consumed.
 */
int tamp_batch_decompress(const uint8_t *dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t *in,
                          const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                          const uint32_t *out_cap, uint32_t *out_len, int8_t *status, uint32_t *in_consumed,
                          size_t n_streams, int mem, int device, void *stream);

/*
 * How large would the output be?  A `.tamp` stream does not record the length of its plain text; this call finds it -- or refuses
 * to look further than `limit` -- without decoding a byte.  The contract in one sentence: the call returns, per stream, exactly
 * the out_len, status and in_consumed that tamp_batch_decompress returns for the same call with out_cap[i] = limit[i]
 * (limit == NULL: 0xFFFFFFFF for every stream), and writes no output bytes.  So a stream that ends normally gets
 * TAMP_INPUT_EXHAUSTED (2) and its full size, one that would outgrow its limit gets TAMP_OUTPUT_FULL (1) with
 * decoded_size[i] == limit[i] (a decompression bomb is refused at the price of parsing up to the limit: an RLE token is 241
 * bytes in 14 bits), malformed input TAMP_OOB / TAMP_INVALID_CONF and a stream of 2^29 bytes or more TAMP_AMD_BAD_ARGUMENT.
 * Room that is used up exactly still reports TAMP_OUTPUT_FULL when padding bits are left, as the reference does: decode with
 * out_cap[i] = decoded_size[i] + 1 to see the end status.
 *
 *   dictionary_len      length of the custom dictionary the decode call will pass (0: none).  Its bytes are not needed: a
 *                       stream whose header has the custom bit and asks for more than dictionary_len gets TAMP_INVALID_CONF
 *   max_window_bits     as for tamp_batch_decompress; TAMP_AMD_WINDOW_BITS_EXACT is accepted and ignored (no pre-pass exists)
 *   limit               optional (may be NULL): per-stream bound on decoded_size
 *   in_consumed         optional (may be NULL)
 *   mem, device, stream as for tamp_batch_decompress.  With TAMP_AMD_MEM_DEVICE the call is one kernel on `stream` and waits
 *                       for nothing.  With TAMP_AMD_MEM_HOST the compressed bytes are staged as for a decode call and only the
 *                       three tables come back.
 */
int tamp_batch_decoded_size(size_t dictionary_len, uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off,
                            const uint32_t *in_len, const uint32_t *limit /* may be NULL */, uint32_t *decoded_size,
                            int8_t *status, uint32_t *in_consumed /* may be NULL */, size_t n_streams,
                            int mem, int device, void *stream);

/* ---- dictionary tables: one launch, one custom dictionary PER STREAM ---------------------------------
 *
 * A feed with several message types carries one trained dictionary per type.  The three calls below take a BUFFER of
 * dictionaries and a per-stream selector instead of one dictionary:
 *
 *   dictionaries / dictionaries_len   the buffer: any number of dictionaries, laid out as the caller likes
 *   dict_off[i]                       byte offset of stream i's dictionary in the buffer, a multiple of 16.  A table of K
 *                                     equal dictionaries of D bytes is dict_off[i] = k_i * D (D a multiple of 16).  Lives
 *                                     where the other tables live (`mem`); ALL_DEVICES and the launches of very large batches
 *                                     slice it together with in_off
 *
 * Stream i behaves exactly as the plain call would with dictionary = dictionaries + dict_off[i].  With dict_off == NULL each call
 * IS its plain twin (which is how the plain calls are implemented).  Everything else -- tables, status codes, mem / device /
 * stream, block mode, the long-stream decoder -- is as documented above.
 *
 * The compress kernel's table builds are twins of the generic builds, compiled apart from them: the plain calls run the code they
 * ran before the table existed.  A table call never takes a fixed-geometry build (tamp_amd_compress_build: TAMP_AMD_CALL_DICT_TABLE).
 *
 * tamp_batch_compress_dicts: conf->use_custom_dictionary must be set when dict_off is given (the custom bit sits in the one header
 *   byte the launch shares), else the call returns TAMP_AMD_BAD_ARGUMENT.  A stream whose row is not a multiple of 16, or with
 *   dict_off[i] + (1 << window) > dictionaries_len, gets status TAMP_AMD_BAD_ARGUMENT and out_len = 0; nothing of it is read and
 *   nothing written, and the rest of the batch is unaffected.
 * tamp_batch_decompress_dicts: a stream whose header lacks the custom bit ignores its row.  One that has it starts from
 *   dictionaries + dict_off[i]; if dict_off[i] + (1 << its own window) > dictionaries_len it gets TAMP_INVALID_CONF (what too
 *   short a shared dictionary gets), and a row that is not a multiple of 16 gets TAMP_AMD_BAD_ARGUMENT.  Nothing outside the
 *   buffer is ever read.
 * tamp_batch_decoded_size_dicts: only the lengths matter; per stream exactly the out_len, status and in_consumed of
 *   tamp_batch_decompress_dicts with out_cap = limit.
 */
int tamp_batch_compress_dicts(const TampAmdConf *conf, const uint8_t *dictionaries, size_t dictionaries_len,
                              const uint64_t *dict_off, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                              uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                              int8_t *status, size_t n_streams, uint32_t max_in_len, int mem, int device, void *stream);
int tamp_batch_decompress_dicts(const uint8_t *dictionaries, size_t dictionaries_len, const uint64_t *dict_off,
                                uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                                int8_t *status, uint32_t *in_consumed, size_t n_streams, int mem, int device, void *stream);
int tamp_batch_decoded_size_dicts(size_t dictionaries_len, const uint64_t *dict_off, uint8_t max_window_bits,
                                  const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                  const uint32_t *limit /* may be NULL */, uint32_t *decoded_size, int8_t *status,
                                  uint32_t *in_consumed /* may be NULL */, size_t n_streams, int mem, int device,
                                  void *stream);

/* ---- one long buffer as dictionary-reset segments --------------------------------------------------
 *
 * A stream whose header has the dictionary_reset bit may hold RESETS (tamp_compressor_reset_dictionary, compressor.c:847-881;
 * decoder: decompressor.c:501-513): two FLUSH tokens, after which the output is byte aligned and the window is the seeded
 * dictionary again.  The pieces between resets do not depend on each other, so a buffer cut every reset_interval bytes is a
 * BATCH, and the whole device compresses ONE stream of the default (extended) format -- which tamp_batch_compress gives to one
 * workgroup.  The price is compression ratio: every segment starts from the seeded window (profiles/reset_segments_ratio.txt).
 * This is NOT a parallel form of the un-segmented stream: tamp.compress(data) without resets stays one workgroup, and its bytes
 * differ from this call's.
 *
 * With K = ceil(in_len / reset_interval) segments (K = 1 for an empty input) the output is byte for byte what ONE reference
 * object writes for
 *     tamp_compressor_init(&c, &conf, window)                                   (conf.dictionary_reset = 1)
 *     K - 1 times:  tamp_compressor_compress(reset_interval bytes) ... ; tamp_compressor_reset_dictionary(&c, ...)
 *     tamp_compressor_compress(the rest) ... ; tamp_compressor_flush(&c, ..., write_token = false)
 * -- K - 1 resets, none behind the last segment, no FLUSH token at the end -- an ordinary `.tamp` stream for any decoder.
 *
 *   conf            dictionary_reset must be 1 and use_custom_dictionary 0 (a reset restores the SEEDED window); window, literal,
 *                   extended and lazy_matching as for tamp_batch_compress
 *   in, in_len      the buffer; in_len <= 0xFFFFFFFF, and the worst case of ONE segment (2 + 9/8 of min(reset_interval, in_len) bytes at
 *                   literal 8) must fit 32 bits: reset_interval above ~3.8e9 on a buffer that long is TAMP_AMD_BAD_ARGUMENT
 *   reset_interval  >= 1: input bytes per segment
 *   out, out_cap    room for the stream; tamp_amd_compress_resets_bound() bytes always suffice
 *   out_len, status one element each.  TAMP_OK and the stream's length; or -- two deviations from the reference, on failure only --
 *                   TAMP_EXCESS_BITS when any segment holds a byte that does not fit conf->literal bits, TAMP_OUTPUT_FULL when
 *                   the stream is longer than out_cap (the reference would leave a prefix): out_len = 0 in both cases, the
 *                   bytes of out[0 .. out_cap) are unspecified and nothing is written at or behind out + out_cap
 *   reset_off       optional (may be NULL): K - 1 offsets into the stream, the byte behind each reset (where the next segment's
 *                   tokens begin)
 *   mem, device, stream   as for tamp_batch_compress: every pointer but conf lives where `mem` says; a device-memory call is
 *                   asynchronous on `stream` and waits for nothing, a host-memory call is synchronous (`stream` is not used)
 * Returns TAMP_OK when the call was launched, TAMP_AMD_BAD_ARGUMENT for a call outside the contract above (nothing is written),
 * TAMP_AMD_NO_DEVICE.
 *
 * The segments' outputs are gathered from slabs of tamp_amd_compress_resets_slab() bytes each in scratch memory kept per HIP
 * stream (tamp_amd_trim releases it); a call whose slabs outgrow a quarter of the free device memory (8 GiB at most) runs in
 * slices of at most 2^20 segments.  TAMP_AMD_RESETS_SCAN_TILE segments are scanned per step of the one workgroup that places them.
 */
#define TAMP_AMD_RESETS_SCAN_TILE 1024
int tamp_amd_compress_resets(const TampAmdConf *conf, const uint8_t *in, uint64_t in_len, uint32_t reset_interval, uint8_t *out,
                             uint64_t out_cap, uint64_t *out_len, int8_t *status, uint64_t *reset_off /* may be NULL */,
                             int mem, int device, void *stream);
/* Host only.  Worst-case length of that stream: per segment the 2-byte lead, every byte a literal and the FLUSH token. */
size_t tamp_amd_compress_resets_bound(size_t n, uint32_t reset_interval, uint8_t literal);
/* DIAGNOSTICS, host only; this function and TAMP_AMD_RESETS_SCAN_TILE describe the implementation's geometry and may change or go
 * between releases.  Stride of the segments' slabs in the call's scratch (segment k of a slice is gathered from byte k * slab of a
 * 256-byte aligned buffer): diagnostics, and what the tests compute the gather's source alignments from. */
size_t tamp_amd_compress_resets_slab(size_t n, uint32_t reset_interval, uint8_t literal);

/*
 * The batch form: EVERY stream of a batch cut into segments of reset_interval bytes, one interval for the whole call.  The segments of
 * all streams are the units of work, each about as long as the next, so a ragged batch with a few long streams no longer waits for
 * its longest stream on one workgroup.  Stream i, with K_i = max(1, ceil(in_len[i] / reset_interval)) segments, is byte for byte
 * what tamp_amd_compress_resets returns for that buffer alone (the script above); an empty stream is one empty segment.
 *
 *   conf, reset_interval   as above: dictionary_reset 1, use_custom_dictionary 0, reset_interval >= 1, and the worst case of ONE
 *                   segment of reset_interval bytes must fit 32 bits; otherwise TAMP_AMD_BAD_ARGUMENT and nothing is written
 *   in .. status, n_streams, max_in_len, mem, device, stream   the tables of tamp_batch_compress, with its meaning of every one;
 *                   TAMP_AMD_ALL_DEVICES is not taken.  n_streams == 0: TAMP_OK, nothing is done
 *   max_in_len      a hint, as there: it sizes the compress kernel's block (for segments: min(reset_interval, max(max_in_len, 16))
 *                   positions), and a stale one costs speed, never bytes -- the slabs are sized from in_len[] itself.  0 = unknown:
 *                   the longest stream of the tables stands in.  A host-memory call reads the tables and ignores the hint
 *   out_cap[i]      tamp_amd_compress_resets_bound(in_len[i], reset_interval, conf->literal) bytes always suffice
 *   out_len[i], status[i]   TAMP_OK and the stream's length; TAMP_EXCESS_BITS when any of its segments holds a byte outside
 *                   conf->literal bits, TAMP_OUTPUT_FULL when its stream is longer than out_cap[i]: out_len[i] = 0 for both, the bytes
 *                   of its slab are unspecified, nothing is written in front of out + out_off[i] or at or behind
 *                   out + out_off[i] + out_cap[i], and no other stream is affected
 * A host-memory call is synchronous and writes exactly the produced bytes and the two result tables.  A device-memory call runs on
 * `stream` and WAITS once, early, for one 16-byte record it reads back -- how many segments the batch has and how long its longest
 * stream is, which size its scratch (the slabs of tamp_amd_compress_resets, per HIP stream, in slices by the same rule); everything
 * behind that is asynchronous.
 */
int tamp_batch_compress_resets(const TampAmdConf *conf, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                               uint32_t reset_interval, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                               uint32_t *out_len, int8_t *status, size_t n_streams, uint32_t max_in_len,
                               int mem, int device, void *stream);

/*
 * The same call, and the same bytes, with a RESET INDEX on top: where every reset of every stream lies.  The compressor knows
 * these positions (they are what places its segments); a reader that has them need not search the stream for its resets.
 *   reset_first     n_streams + 1 entries, may be NULL: reset_first[i] = sum of K_j - 1 over j < i, so stream i's K_i - 1 entries are
 *                   reset_off[reset_first[i] .. reset_first[i + 1]) and reset_first[n_streams] is their number in the whole batch
 *   reset_off       one entry per reset: the offset, from out + out_off[i], of the byte behind it -- where the next segment's tokens
 *                   begin, the values tamp_amd_compress_resets gives for that stream alone.  The entries of a stream whose
 *                   status is not TAMP_OK are unspecified.  NULL (with reset_cap 0): no index, which is tamp_batch_compress_resets
 *   reset_cap       the entries reset_off has room for.  A batch with more resets than that is refused with TAMP_AMD_BAD_ARGUMENT
 *                   before anything is written: sum max(1, ceil(in_len[i] / reset_interval)) - 1 over the streams always suffices
 * Both tables lie where `mem` says.  A host-memory call writes them with the results; n_streams == 0 writes nothing at all.
 */
int tamp_batch_compress_resets_index(const TampAmdConf *conf, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                     uint32_t reset_interval, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                     uint32_t *out_len, int8_t *status, size_t n_streams, uint32_t max_in_len,
                                     int mem, int device, void *stream, uint64_t *reset_first, uint32_t *reset_off,
                                     uint64_t reset_cap);

/*
 * Reading such a stream back with the whole device.  For ONE stream whose header has the dictionary_reset bit and no custom bit the
 * call returns out_len, status and in_consumed exactly as tamp_batch_decompress does for that stream with the given max_window_bits
 * and out_cap -- and, with out == NULL, exactly as tamp_batch_decoded_size does with limit = out_cap, writing no bytes.  The resets are
 * found on the device (the token grammar does not depend on them), the segments between them are decoded as a batch of independent
 * streams into `out`.  That fast path is taken only when everything is clean: a stream shorter than TAMP_AMD_RESETS_MIN bytes
 * (environment, default 262144, at least 64) or of 2^29 - 512 bytes and more, without the reset bit, with the custom bit, with a window
 * above max_window_bits, with an offset out of its window, with more than four resets inside 512 (extended format: 128) compressed
 * bytes, with a segment that does not end byte aligned at normal completion, or whose size reaches out_cap is handed to the exact
 * path BEFORE anything is written -- same results, the speed of tamp_batch_decompress.  tamp_batch_decompress itself is unchanged.
 *   in, out              where `mem` says; out_len, status, in_consumed (may be NULL): HOST memory, one element each
 *   mem, device, stream  device memory: the kernels run on `stream`, and the call WAITS for them (it reads tables back as it goes)
 *                        host memory: the device staging buffer for the output is out_cap bytes -- ask for the size first
 *                        (out = NULL) and pass a little more than it, as tamp_amd.decompress() does, not a generous bound
 * Returns TAMP_OK, TAMP_AMD_BAD_ARGUMENT, TAMP_AMD_NO_DEVICE -- or TAMP_ERROR, the one case in which bytes were written and no answer is
 * given: the batch decode of a segment did not produce the size the size pass found for it (the two passes disagree: a defect of
 * the library, never a property of the stream; out_len / status / in_consumed are not written).
 */
int tamp_amd_decompress_resets(uint8_t max_window_bits, const uint8_t *in, uint32_t in_len, uint8_t *out /* NULL: the size only */,
                               uint32_t out_cap, uint32_t *out_len, int8_t *status, uint32_t *in_consumed /* may be NULL */,
                               int mem, int device, void *stream);

/*
 * Reading a BATCH of such streams back, the segments of all streams as the units of work, with the reset index of
 * tamp_batch_compress_resets_index as a HINT.  For every stream out_len[i], status[i], in_consumed[i] and the bytes
 * out[out_off[i] .. + out_len[i]) are exactly what tamp_batch_decompress gives for it with no dictionary, the same max_window_bits
 * and the same out_cap[i] -- and, with out == NULL, what tamp_batch_decoded_size gives with limit = out_cap -- for ANY contents of
 * the index; nothing is written outside [out_off[i], out_off[i] + out_cap[i]).  The index is verified on the device: a stream is
 * SPLIT into its segments only when its header has the reset bit, no custom bit and a window of at most max_window_bits, when it
 * has at least one entry, its entries are strictly increasing, behind the header and at or before in_len[i], when walking every
 * segment token by token from its start ends exactly at its boundary behind two FLUSH tokens (the last segment: as a stream ends)
 * with no offset out of the window, and when the stream's size stays below out_cap[i].  Every other stream is decoded WHOLE, as
 * tamp_batch_decompress decodes it.  There is no minimum length and no environment switch.
 *   reset_first     n_streams + 1 entries, a running sum from 0 (a table that is none: the call goes without an index)
 *   reset_off       reset_first[n_streams] entries; may be NULL when there are none
 *   out_cap         required with and without `out`; the other tables as for tamp_batch_decompress; in_consumed may be NULL
 *   mem, device, stream   as there, TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS once, early, for one 16-byte
 *                   record (how many entries the batch has, how many bytes it may stage); everything behind that is asynchronous on
 *                   `stream`.  A host-memory call is synchronous and writes exactly the produced bytes and the result tables.
 * The segments are staged in scratch kept per HIP stream (a quarter of the free device memory at most, 8 GiB at most; streams are
 * split in stream order until it is full).  With TAMP_AMD_RESETS_DEBUG set the call writes one line to stderr:
 * "[tamp_amd resets] batch decode: <n> streams, <s> split into <u> units, <w> whole" (and waits for the device to say so).
 * status[i] = TAMP_ERROR: a segment of stream i did not decode to the size the walk found -- a defect of the library.
 * Returns TAMP_OK, TAMP_AMD_BAD_ARGUMENT (a null required table, a bad memory kind, n_streams >= 2^32), TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_decompress_resets(uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                 const uint64_t *reset_first, const uint32_t *reset_off,
                                 uint8_t *out /* NULL: sizes only */, const uint64_t *out_off, const uint32_t *out_cap,
                                 uint32_t *out_len, int8_t *status, uint32_t *in_consumed /* may be NULL */,
                                 size_t n_streams, int mem, int device, void *stream);

/*
 * Reading byte RANGES of such streams without decoding the rest: random access.  The compressor cuts every stream into segments of
 * reset_interval decoded bytes that do not depend on each other and its index says where each one's tokens start, so decoded byte b
 * of a stream lies in segment b / reset_interval.  Range q asks for the decoded bytes [range_begin[q], range_begin[q] + range_len[q])
 * of stream i = range_stream[q]; they go to out + out_off[q], where the room is exactly range_len[q] bytes (there is no capacity
 * table).  Only the segments a range touches are looked at: k0 = begin / N through k1 = min((begin + len - 1) / N, E) for a stream
 * with E index entries (segments 0 .. E, the last one open; E = 0: the whole stream is one open segment), all in 64 bits.  Ranges
 * may come in any order, repeat, overlap and share segments; each is answered on its own, and a segment two ranges touch is
 * decoded twice (nothing is de-duplicated).
 *   in, in_off, in_len      the streams, as for tamp_batch_decompress_resets
 *   reset_first, reset_off  their reset index (tamp_batch_compress_resets_index); reset_off may be NULL only when reset_first[n_streams]
 *                           is 0 (a host-memory call refuses the call otherwise, a device-memory call the ranges of streams with entries)
 *   reset_interval          the N the streams were compressed with, > 0
 *   range_stream, range_begin, range_len, out_off   n_ranges entries each, where `mem` says; only read
 *   out_len[q], status[q]   per range, the first rule that applies:
 *       range_stream[q] >= n_streams ........................................ TAMP_AMD_BAD_ARGUMENT, 0
 *       range_len[q] == 0 .................................................... TAMP_OK, 0 (the stream is not looked at)
 *       the header has no reset bit, a non-zero second byte, the custom bit
 *       or a window above max_window_bits .................................... TAMP_INVALID_CONF, 0
 *       the stream's rows of reset_first are no running sum from 0 ........... TAMP_AMD_BAD_INDEX, 0
 *       k0 > E: the range starts behind the stream's last segment ............ TAMP_INPUT_EXHAUSTED, 0
 *       an offset out of the window in a touched segment ..................... TAMP_OOB, 0
 *       an entry a touched segment uses is out of range or order (inside the
 *       header, beyond in_len[i], not behind the one in front of it), a touched
 *       segment of 2^29 - 512 compressed bytes or more, a closed one that does not
 *       end exactly at its entry behind FLUSH, FLUSH or does not decode to exactly
 *       N bytes, the open one decoding to more than N .......................... TAMP_AMD_BAD_INDEX, 0
 *       the range alone outgrows the scratch budget (below) .................. TAMP_AMD_BAD_ARGUMENT, 0
 *       a segment did not decode to what the walk found (a defect of the library) TAMP_ERROR, 0
 *       otherwise: TAMP_OK and range_len[q] when all bytes were delivered, TAMP_INPUT_EXHAUSTED and the bytes delivered when
 *       the stream ended first
 *   Exactly out_len[q] bytes are written at out + out_off[q] and nothing else of `out`; a failing range writes nothing and affects
 *   no other range.  With the compressor's own index and interval the bytes are those of the whole stream decoded, sliced.
 * WHAT THE INDEX IS TRUSTED FOR.  Unlike tamp_batch_decompress_resets, which takes the index as a hint and checks every segment
 * from the header on, this call trusts it for POSITION: a segment's start is no longer token aligned by induction from the header.
 * The checks above are made on the touched segments only; the two size conditions are what make k * N an address, and they also
 * catch a call made with the wrong interval.  A forged index whose touched segments happen to parse can deliver other bytes, and a
 * range that touches only the open segment has no closed segment to check N against.  Memory safety holds for any contents of
 * every table (reset_off must have reset_first[n_streams] entries, as ever).
 *   mem, device, stream   TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS once, early, for one 16-byte record (how many
 *                   units the ranges come to and what they ask of the scratch); everything behind that is asynchronous on `stream`
 *                   (the decode step is tamp_batch_decompress's: without TAMP_AMD_WINDOW_BITS_EXACT in max_window_bits it waits for its
 *                   header pre-pass).  A host-memory call is synchronous; it copies ONLY the touched segments' compressed bytes to the
 *                   device -- sum of (segment + 2) over the touched segments, never the whole streams -- and writes exactly the
 *                   delivered bytes and the two result tables.
 * The touched segments are staged and decoded, each with its room trimmed to the last byte asked for, in scratch kept per HIP
 * stream (tamp_amd_trim releases it): a quarter of the free device memory at most, 8 GiB at most, TAMP_AMD_RANGES_SCRATCH_MB (environment)
 * instead of both.  Ranges are processed in slices, in range order, each of which fits that budget (a device-memory call that needs
 * more than one slice reads three more tables back to cut them).  With TAMP_AMD_RESETS_DEBUG set the call writes one line to stderr:
 * "[tamp_amd resets] read ranges: <r> ranges, <u> units, <s> slices, <b> bytes staged".
 * Returns TAMP_OK (n_ranges == 0: at once, nothing is touched); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null
 * in_off, in_len, reset_first, range_stream, range_begin, range_len, out_off, out_len or status, a null `in` with n_streams > 0, a
 * null `out` with n_ranges > 0, reset_interval == 0, a bad memory kind, TAMP_AMD_ALL_DEVICES, n_streams or n_ranges >= 2^32;
 * TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_read_ranges(uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                           const uint64_t *reset_first, const uint32_t *reset_off, uint32_t reset_interval,
                           const uint32_t *range_stream, const uint64_t *range_begin, const uint32_t *range_len,
                           uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int8_t *status,
                           size_t n_streams, size_t n_ranges, int mem, int device, void *stream);

/*
 * The table of SEGMENT ENDS of a batch whose reset segments differ in size: streams a reference Compressor(dictionary_reset) wrote
 * with reset_dictionary() calls of its own, append-mode logs, streams compressed with different intervals.  From what
 * tamp_batch_index_resets returns (reset_first, closed_size, open_size) it makes ONE uint64 table with an entry per segment, not per
 * reset: stream i with E = reset_first[i + 1] - reset_first[i] resets has E + 1 segments, its entries lie at
 * segment_end[reset_first[i] + i + k] for k = 0 .. E, and the table has reset_first[n_streams] + n_streams entries, which is the
 * room `segment_end` must have.  Entry k is the decoded size of the stream's segments 0 .. k: non-decreasing, the last one the
 * stream's decoded size.  Segment k covers the decoded bytes [B(k), B(k + 1)) with B(0) = 0 and B(k) = entry k - 1; segments of no
 * bytes (two resets in a row, an append marker at an empty file) are legal.  A size of 0xFFFFFFFF ("2^32 - 1 or more") makes its
 * entry and every later entry of its stream 2^64 - 1.  Rows of reset_first that are no running sum add nothing; nothing is read
 * or written outside the four tables whatever they hold.
 *   mem, device, stream   device memory: a per-stream running sum over the rows of the whole batch, a lane per row, in two launches on
 *                   `stream`; NOTHING is read back and the stream is never waited for, so index -> table -> ranges stays on the
 *                   device.  Host memory: the same sum on the host; no device is looked for.
 * Returns TAMP_OK (n_streams == 0: at once); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null reset_first or
 * segment_end, a null open_size with n_streams > 0, a null closed_size (host memory: with reset_first[n_streams] != 0; device
 * memory: with n_streams > 0), a bad memory kind, TAMP_AMD_ALL_DEVICES, n_streams >= 2^32; TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_segment_ends(const uint64_t *reset_first, const uint32_t *closed_size, const uint32_t *open_size,
                            uint64_t *segment_end, size_t n_streams, int mem, int device, void *stream);

/*
 * tamp_batch_read_ranges for segments of ANY size: `segment_end` (tamp_batch_segment_ends) in place of reset_interval.  The segment
 * of a byte is found by a search in the stream's entries where that call divides; everything behind that -- stage, walk, decode,
 * gather -- the result tables, the scratch budget, the slices, the debug line and the memory-kind rules are that call's.  Per range
 * with range_len[q] > 0 on an eligible stream (the rules up to the reset_first one are unchanged), `total` the stream's last entry:
 *       range_begin[q] >= total .............................................. TAMP_INPUT_EXHAUSTED, 0 (from the table alone: no units)
 *   otherwise end = min(begin + len, total), the sum saturating in 64 bits; k0 = the number of entries <= begin among the stream's
 *   first E (empty segments are stepped over), k1 = the number <= end - 1.  The units are segments k0 .. k1: every one but the last
 *   is asked for its whole size, the last for end - B(k1); the scratch is end - B(k0) -- true sizes, the open segment's too -- and
 *   the range's bytes start begin - B(k0) bytes into it.  end - begin bytes are delivered: TAMP_OK when that is range_len[q], else
 *   TAMP_INPUT_EXHAUSTED.
 * WHAT THE TABLE IS TRUSTED FOR.  Position, as the index is: the table says which segment holds a byte, and it is verified on what
 * a range touches.  Each of these is TAMP_AMD_BAD_INDEX and 0 bytes for the range, and affects no other: B(k0) <= begin < B(k0 + 1)
 * does not hold behind the search (a table that is not sorted); a touched entry below the one in front of it; a touched segment
 * whose table size is 2^32 - 1 or more; a touched segment, closed OR open, that does not decode to exactly its table size; and, as
 * before, a closed segment that does not end at its entry behind FLUSH, FLUSH, and an entry of reset_off out of range or order.  An
 * offset out of the window stays TAMP_OOB.  The search is memory safe for any contents of the table: its bounds come from
 * reset_first (segment_end must have reset_first[n_streams] + n_streams entries).  A forged table AND index whose touched segments
 * happen to parse to the forged sizes can deliver other bytes.
 * Returns as tamp_batch_read_ranges, with a null segment_end in place of reset_interval == 0.
 */
int tamp_batch_read_ranges_grid(uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                                const uint64_t *reset_first, const uint32_t *reset_off, const uint64_t *segment_end,
                                const uint32_t *range_stream, const uint64_t *range_begin, const uint32_t *range_len,
                                uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int8_t *status,
                                size_t n_streams, size_t n_ranges, int mem, int device, void *stream);

/*
 * A SEEK INDEX: byte ranges of streams that have NO dictionary resets -- the output of tamp_batch_compress without a reset
 * interval, of a connection of compressor objects, of a reference Compressor.  The stream is decoded once and a CHECKPOINT of the
 * decoder is kept every `interval` decoded bytes; a later read starts at the nearest one (what zran does for deflate).
 * A checkpoint is a decoder object as tamp_batch_decompress_resume carries it between calls: checkpoint k (k >= 1) is the
 * reference's object, initialised without a configuration, after k calls of tamp_decompressor_decompress that were each offered
 * all input not yet consumed and exactly `interval` bytes of room (each returns TAMP_OUTPUT_FULL with `interval` bytes), and next
 * to it in_pos, the sum of their consumed counts.  Its decoded position is exactly k * interval -- inside an RLE run (token_state
 * 1), an extended match (3) or a plain match (token_state 0, skip_bytes > 0) if that is where the room ran out.  A stream that
 * decodes to S bytes (what tamp_batch_decompress delivers: the bytes in front of the first error) has C = 0 checkpoints for
 * S == 0 and (S - 1) / interval otherwise: one for every k >= 1 with k * interval < S.  The state in front of the first byte is not
 * stored.
 *   dictionary, dictionary_len, max_window_bits, in, in_off, in_len   as for tamp_batch_decompress (one custom dictionary for the
 *                   call; TAMP_AMD_WINDOW_BITS_EXACT is not taken)
 *   interval        decoded bytes between checkpoints, > 0
 *   ckpt_first      n_streams + 1 entries, only read: the running sum of how many rows each stream has ROOM for (from a size
 *                   query: tamp_batch_decoded_size); row r of stream i is row ckpt_first[i] + r of the two tables below
 *   ckpt_in         uint32 per row: in_pos
 *   ckpt_state      rows of state_stride bytes, 16-byte aligned: TampAmdDecoderState (window_bits_max = max_window_bits), then
 *                   the window; state_stride >= tamp_amd_decoder_state_size(max_window_bits), a multiple of 16.  A stream with a
 *                   smaller window uses the first 1 << w window bytes of its rows
 *   decoded_size[i], status[i]   S as 64 bits, and what tamp_batch_decompress reports for the stream with unlimited room
 *                   (TAMP_INPUT_EXHAUSTED for one that ends normally); TAMP_AMD_BAD_ARGUMENT for a stream of 2^29 - 512 compressed
 *                   bytes or more
 * Stream i writes its first min(C, room) rows and never a row outside its own; when decoded_size[i] says that more exist than it
 * had room for, call again with more.  (A stream with the dictionary-reset bit whose decoded size is an exact multiple of the
 * interval and that ends in a reset may write the row behind its last one where it has room for it.)
 * A device-memory call is one asynchronous launch on `stream`: nothing is allocated, nothing read back.  A host-memory call is
 * synchronous and copies back the two result tables and exactly the rows written.
 * Returns TAMP_OK; TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null in_off, in_len, ckpt_first, decoded_size or
 * status, a null `in` with n_streams > 0, interval == 0, max_window_bits outside 8..15, a state_stride or ckpt_state that is not as
 * above, a bad memory kind, TAMP_AMD_ALL_DEVICES, n_streams >= 2^32, (host memory) a ckpt_first that is no running sum or null row
 * tables where it has room; TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_seek_index(const uint8_t *dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t *in,
                          const uint64_t *in_off, const uint32_t *in_len, uint32_t interval, const uint64_t *ckpt_first,
                          uint32_t *ckpt_in, void *ckpt_state, size_t state_stride, uint64_t *decoded_size, int8_t *status,
                          size_t n_streams, int mem, int device, void *stream);

/*
 * EXTENDING such an index when its streams have GROWN, without building it again.  Precondition: every stream's old bytes -- the
 * ones its rows were made from -- are a PREFIX of its bytes now (a connection that wrote another message, a log that was
 * appended to).  The call does not and cannot check that; an index of other bytes gives rows of no use, within memory safety.
 * The result is, byte for byte, what tamp_batch_seek_index gives for the grown streams: rows, in_pos, decoded_size and status.
 *   ckpt_first, ckpt_in, ckpt_state, state_stride, decoded_size, status, and all in front of them: tamp_batch_seek_index's.
 *                   ckpt_first is the running sum of each stream's ROOM, as there
 *   ckpt_have       uint32 per stream, only read: how many of stream i's rows already hold its old checkpoints, in their places
 *                   at the front of its room
 * Continuing from a stream's last row would be wrong: the calls that made the last rows may have met the old end of the input,
 * and a refill that the end cut short leaves a smaller bit_buffer, bit_buffer_pos and in_pos than the same call leaves with
 * more input behind it.  Such rows are exactly those whose in_pos is the old in_len, and several rows can share it.  The old
 * in_len is not recorded, and the rule does without it:
 *   The RESTART ROW of a stream that holds `have` rows is the last of them whose in_pos is smaller than the in_pos of row
 *   have - 1; if there is none the stream restarts from its header with a fresh object.  Rows up to and including the restart
 *   row are final and only read.  Every row behind it is decoded again and written again.
 * (Every row in front of the restart row has an in_pos smaller still, so below the old in_len: final.)  Per stream:
 *   rows 0 .. restart are read; rows restart + 1 .. min(C, room) - 1 are written, and nothing else of the tables
 *   have == 0 ........ a build, exactly tamp_batch_seek_index
 *   have == room ..... writes no row it did not have and is the size query: decoded_size says C; call again with more
 *   have > room, or a restart row that does not hold up -- tamp_batch_read_ranges_seek's checks of a row a unit starts at (its
 *   conf byte is not the stream's header byte, the configured flag is missing, token_state is not 0, 1 or 3, window_pos or a
 *   pending token lies outside the window, in_pos lies inside the header, beyond in_len[i] or below the row's in front of it),
 *   a row between it and the last one whose in_pos lies beyond in_len[i], or a token at the restart row's place that is not
 *   the one the row names ... TAMP_AMD_BAD_INDEX and decoded_size 0 for that stream; it writes no row and affects no other stream
 *   The stream's own verdicts (no bytes, a bad header, TAMP_AMD_BAD_ARGUMENT for its length) come first, as the build gives them.
 * The index is TRUSTED FOR POSITION, as in the read; memory safety holds for any contents of every table (ckpt_in and ckpt_state
 * must have ckpt_first[n_streams] rows).
 * A device-memory call is one asynchronous launch on `stream`: nothing is allocated, nothing read back.  A host-memory call is
 * synchronous: the rule, the header and the restart row's checks run on the host, and per stream it uploads ONLY the restart row
 * and the compressed bytes from that row's in_pos to in_len (a restart from the header: the stream from byte 0), and copies back
 * only the rows written and the two result tables.
 * Returns as tamp_batch_seek_index; a null ckpt_have is a TAMP_AMD_BAD_ARGUMENT too, before a device is looked for.
 */
int tamp_batch_seek_index_extend(const uint8_t *dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t *in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint32_t interval, const uint64_t *ckpt_first,
                                 const uint32_t *ckpt_have, uint32_t *ckpt_in, void *ckpt_state, size_t state_stride,
                                 uint64_t *decoded_size, int8_t *status, size_t n_streams, int mem, int device, void *stream);

/*
 * Reading byte ranges through such an index.  The range tables, the output and the result tables are tamp_batch_read_ranges's;
 * the index tables are tamp_batch_seek_index's, with the stream's ROWS in ckpt_first (R rows of stream i: checkpoints 1 .. R) and
 * ckpt_first[n_streams] rows in each table.  A range is cut at the checkpoints it crosses and every piece is a UNIT of its own,
 * one wavefront: unit (q, k), k = min(begin / interval, R) .. min((begin + len - 1) / interval, R), loads row k (k == 0: a fresh
 * object and the stream's header), picks up the token the checkpoint lies in, drops the bytes in front of max(begin, k * interval),
 * and decodes the bytes up to min(end, (k + 1) * interval) -- the last unit: up to end -- straight to their place in
 * out + out_off[q].  With fewer rows than checkpoints (R < C) the last row serves everything behind it.
 *   out_len[q], status[q]   per range, the first rule that applies:
 *       range_stream[q] >= n_streams, or a stream of 2^29 - 512 compressed bytes or more ... TAMP_AMD_BAD_ARGUMENT, 0
 *       range_len[q] == 0 ............................................................. TAMP_OK, 0 (the stream is not looked at)
 *       in_len == 0, or less than the header .......................................... TAMP_INPUT_EXHAUSTED, 0
 *       a non-zero second header byte, a window above max_window_bits, the custom bit
 *       without a dictionary of 1 << w bytes ........................................... TAMP_INVALID_CONF, 0
 *       the stream's rows of ckpt_first are no running sum inside ckpt_first[n_streams] . TAMP_AMD_BAD_INDEX, 0
 *       a row a unit starts at does not hold up: its conf byte is not the stream's header
 *       byte, the configured flag is missing, token_state is not 0, 1 or 3, window_pos or
 *       a pending token lies outside the window, in_pos lies inside the header, beyond
 *       in_len[i] or below the row's in front of it ..................................... TAMP_AMD_BAD_INDEX, 0
 *       an offset out of the window on the way ........................................ TAMP_OOB and the bytes in front of it
 *       otherwise: TAMP_OK and range_len[q] when all bytes were delivered, TAMP_INPUT_EXHAUSTED and the bytes delivered when
 *       the stream ended first
 *   Exactly out_len[q] bytes are written at out + out_off[q] and nothing else of `out`; a range with a bad row writes nothing, and
 *   none affects another.  The index is only read: any number of units may start at the same row.
 * The index is TRUSTED FOR POSITION, as tamp_batch_read_ranges trusts its own: a forged row that passes the checks delivers other
 * bytes.  Memory safety holds for any contents of every table (ckpt_in and ckpt_state must have ckpt_first[n_streams] rows).
 *   mem, device, stream   TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS once, early, for one 8-byte record (how
 *                   many units the ranges come to); everything behind that is asynchronous on `stream`.  A host-memory call is
 *                   synchronous: it plans on the host and copies ONLY the touched rows (each once) and the touched units'
 *                   compressed spans [ckpt_in[k], ckpt_in[k + 1]) -- the last one to in_len -- to the device, never the whole
 *                   streams, and writes exactly the delivered bytes and the two result tables.
 * The per-range tables and the unit table (40 bytes a unit) live in scratch kept per HIP stream (tamp_amd_trim releases it).
 * Returns TAMP_OK (n_ranges == 0: at once); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null in_off, in_len,
 * ckpt_first, range_stream, range_begin, range_len, out_off, out_len or status, a null `in` with n_streams > 0, a null `out` with
 * n_ranges > 0, interval == 0, max_window_bits outside 8..15, a state_stride or ckpt_state that is not as above, a bad memory kind,
 * TAMP_AMD_ALL_DEVICES, n_streams or n_ranges >= 2^32; TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_read_ranges_seek(const uint8_t *dictionary, size_t dictionary_len, uint8_t max_window_bits, const uint8_t *in,
                                const uint64_t *in_off, const uint32_t *in_len, uint32_t interval, const uint64_t *ckpt_first,
                                const uint32_t *ckpt_in, const void *ckpt_state, size_t state_stride,
                                const uint32_t *range_stream, const uint64_t *range_begin, const uint32_t *range_len,
                                uint8_t *out, const uint64_t *out_off, uint32_t *out_len, int8_t *status,
                                size_t n_streams, size_t n_ranges, int mem, int device, void *stream);

/*
 * WRITING byte ranges into such streams: the other half of random access.  Write q replaces the decoded bytes
 * [write_begin[q], write_begin[q] + write_len[q]) of stream write_stream[q] with src[src_off[q] .. + write_len[q]).  Only the segments
 * a write touches are decoded (by tamp_batch_read_ranges' own steps), patched and compressed again; every other segment keeps its
 * compressed bytes and is copied to its new place, and the index is shifted.  A stream's decoded size never changes: a write that
 * reaches beyond the end is refused, it does not extend the stream.  Not in the reference.
 *   conf                    how the touched segments are compressed: dictionary_reset = 1, use_custom_dictionary = 0, and window, literal
 *                           and extended as in every written stream's header; lazy_matching is the caller's choice, as for compress
 *   in, in_off, in_len, reset_first, reset_off, reset_interval   the streams and their index, as for tamp_batch_read_ranges; only read
 *   write_stream, write_begin, write_len, src_off   n_writes entries each, where `mem` says; only read.  SORTED by (write_stream,
 *                           write_begin) and, within a stream, NOT OVERLAPPING: checked on the device, write q against q - 1.  That is
 *                           what makes patching free of races with one unit of work per write, and the touched segments of the batch
 *                           a flag array and a scan.  Two writes in one segment make ONE unit, compressed once; a write of length 0
 *                           touches nothing (its stream is not looked at), but it stands in the order like any other
 *   src                     the source bytes, where `mem` says; only read
 *   out, out_off, out_cap   the new stream i comes back in out[out_off[i] ..), out_cap[i] bytes of room
 *   new_reset_off           optional, parallel to reset_off: the new streams' index.  The new stream has the old one's header and as many
 *                           resets, so reset_first holds for it unchanged.  Entries of a failing stream mean nothing
 *   out_len[i], status[i]   per stream.  Of the stream's writes the one with the lowest q that fails decides, and of the rules the
 *                           first that applies to it:
 *       write_stream[q] >= n_streams .......................................... the write is ignored: it has no stream to fail
 *       write q lies in front of write q - 1 (a lower stream, or the same stream
 *       and a begin in front of the predecessor's end) .......................... TAMP_AMD_BAD_ARGUMENT
 *       (write_len[q] == 0: nothing more is asked of it)
 *       the header has no reset bit, a non-zero second byte, the custom bit, a
 *       window above max_window_bits, or window / literal / extended other than
 *       conf's ................................................................ TAMP_INVALID_CONF
 *       the stream's rows of reset_first are no running sum from 0 ............ TAMP_AMD_BAD_INDEX
 *       the write begins or ends behind the stream's decoded end (the open
 *       segment's size is known once it is walked; a write that touches closed
 *       segments only needs no look at the open one) ........................... TAMP_INPUT_EXHAUSTED
 *       an offset out of the window in a touched segment ...................... TAMP_OOB
 *       a touched segment whose index entries do not hold: the conditions of
 *       tamp_batch_read_ranges (out of range or order, a closed segment that does
 *       not end at its entry behind FLUSH, FLUSH or does not decode to exactly
 *       reset_interval bytes, the open one decoding to more) ................... TAMP_AMD_BAD_INDEX
 *       a touched segment that did not decode to what the walk found (a defect
 *       of the library) ........................................................ TAMP_ERROR
 *       a source byte that does not fit conf->literal bits .................... TAMP_EXCESS_BITS
 *     and, of the stream as a whole: its touched segments alone outgrow the scratch budget (below): TAMP_AMD_BAD_ARGUMENT, in front of
 *     every rule above; an untouched segment whose entries lie outside the stream or out of order: TAMP_AMD_BAD_INDEX; the new stream
 *     longer than out_cap[i]: TAMP_OUTPUT_FULL, behind every rule above.
 *     A failing stream has out_len[i] = 0 and unspecified bytes in its slab; nothing is ever written outside [out_off[i], out_off[i] +
 *     out_cap[i]), and no other stream is affected.  A stream no write touches (none, or writes of length 0 only) is copied unchanged,
 *     whatever it holds, with TAMP_OK (TAMP_OUTPUT_FULL when it does not fit), and its entries are copied with it.
 * THE RESULT, bit for bit: every untouched segment keeps its compressed bytes exactly; every touched segment is what
 * tamp_batch_compress_resets writes for that segment's patched bytes under `conf`.  Hence, for streams tamp_batch_compress_resets_index
 * made under the same conf and reset_interval, the new streams and new_reset_off are byte for byte what that call returns for the
 * patched inputs.
 * WHAT THE INDEX IS TRUSTED FOR.  As in tamp_batch_read_ranges the index is trusted for POSITION and checked on the TOUCHED segments
 * only: an entry of an untouched segment that is moved but still in range and order is not noticed -- the bytes between the entries
 * are copied whichever tokens they hold -- and the new index carries the same displacement.  Memory safety holds for any contents of
 * every table (reset_off must have reset_first[n_streams] entries, as ever).
 *   mem, device, stream   TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS for the 8 bytes of reset_first[n_streams] (they
 *                   size its per-segment tables), for one 16-byte record (the units of the call), and once per slice inside the decode
 *                   step, which is tamp_batch_read_ranges' (its 16-byte record; see there for its header pre-pass); everything else is
 *                   asynchronous on `stream`.  A host-memory call is synchronous: the streams, the tables and the sources go up, the
 *                   result tables and exactly the produced bytes come back.
 * SCRATCH is kept per HIP stream (tamp_amd_trim releases it): 18 bytes per segment and 32 per stream of the batch, and per unit a staging
 * row of reset_interval bytes, a slab and 64 bytes of rows, within the budget of tamp_batch_read_ranges (a quarter of the free device
 * memory, 8 GiB at most, TAMP_AMD_RANGES_SCRATCH_MB instead of both); the decode step takes its own scratch by the same rule.  A call
 * whose units outgrow the budget runs in slices of whole streams (it then reads two tables of n_streams + 1 entries back to cut them).
 * With TAMP_AMD_RESETS_DEBUG set the call writes one line to stderr:
 * "[tamp_amd resets] write ranges: <w> writes, <u> units, <s> slices, <b> bytes staged" (b: the decoded bytes of the units).
 * Returns TAMP_OK (n_streams == 0: at once, nothing is done; n_writes == 0: every stream is copied and new_reset_off filled from
 * reset_off); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null conf, in_off, in_len, reset_first, out_off, out_cap,
 * out_len or status, a null write table, src or src_off with n_writes > 0, a null `in` or `out` with n_streams > 0, reset_interval == 0
 * or one whose worst-case segment does not fit 32 bits, a conf that tamp_batch_compress_resets refuses, a bad memory kind,
 * TAMP_AMD_ALL_DEVICES, n_streams or n_writes >= 2^32; TAMP_AMD_BAD_ARGUMENT for 2^32 - 1 touched segments or more; TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_write_ranges(const TampAmdConf *conf, uint8_t max_window_bits,
                            const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                            const uint64_t *reset_first, const uint32_t *reset_off, uint32_t reset_interval,
                            const uint32_t *write_stream, const uint64_t *write_begin, const uint32_t *write_len,
                            const uint8_t *src, const uint64_t *src_off,
                            uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int8_t *status,
                            uint32_t *new_reset_off /* may be NULL */,
                            size_t n_streams, size_t n_writes, int mem, int device, void *stream);

/*
 * APPENDING to such a batch so that it stays seekable.  A stream's size never changes under tamp_batch_write_ranges; this call makes
 * streams grow, and it KEEPS THE GRID: the closed segments of the new stream hold exactly reset_interval decoded bytes each, so that
 * tamp_batch_read_ranges and tamp_batch_write_ranges go on addressing byte b at segment b / reset_interval.  (The reference's own
 * append mode opens with a reset wherever the stream happened to end and loses that.)
 * Stream i has E index entries and an open segment of m decoded bytes, 0 <= m <= N = reset_interval, and receives L = src_len[i] bytes:
 *   - the old stream's bytes in front of its open segment (the header, the E closed segments with their resets) keep their place and
 *     value; they are copied and not looked at
 *   - the open segment's m bytes followed by the L source bytes are cut at every N bytes into U = max(1, ceil((m + L) / N)) segments;
 *     all but the last are closed, and each is what tamp_batch_compress_resets writes for those bytes under `conf`
 *   - the new index holds the old E entries and U - 1 new ones
 * Hence, for streams tamp_batch_compress_resets_index made under the same conf and reset_interval, the new streams and the new index
 * are byte for byte what that call returns for old data + appended data; and the new streams decode, with any decoder, to that.
 *   conf, max_window_bits, in .. reset_interval   as for tamp_batch_write_ranges
 *   src, src_off, src_len   ONE ROW PER STREAM: stream i receives src[src_off[i] .. + src_len[i]); src_len[i] == 0: nothing.  Any
 *                   alignment.  Every byte must fit conf->literal bits
 *   out, out_off, out_cap, out_len, status   the new streams, as for tamp_batch_write_ranges
 *   new_reset_first n_streams + 1 entries, always written: the running sum of E_i + U_i - 1.  A failing stream keeps E_i rows, which
 *                   are zeroed, so that the table stays a running sum (a stream whose rows of reset_first do not hold keeps none)
 *   WHEN A STREAM'S ROWS OF reset_first HOLD: they are in order and inside the table (reset_first[i] <= reset_first[i + 1] <=
 *                   reset_first[n_streams], reset_first[0] == 0), AND they start at or behind the end of every such pair in front
 *                   of them -- two pairs that are each in order may still claim the same entries ({0, 5, 3, 8}: streams 0 and 2; here
 *                   stream 0 holds, streams 1 and 2 do not) -- and reset_off is not NULL unless the stream has no entries.  The
 *                   entries of streams that hold are disjoint, so the bound below suffices whatever the table holds.  A stream whose
 *                   rows do not hold and that receives nothing is copied, without entries
 *   new_reset_off, new_reset_cap   the new entries.  U_i - 1 <= ceil(L_i / N) because m <= N, so reset_first[n_streams] + the sum of
 *                   ceil(src_len[i] / N) entries ALWAYS suffice, whatever the open segments hold; a smaller new_reset_cap is refused
 *                   with TAMP_AMD_BAD_ARGUMENT before anything is written (host tables: before a device is looked for)
 *   status[i]       the first rule that applies:
 *       (src_len[i] == 0: the stream is copied in one piece whatever it holds, its entries with it: TAMP_OK, or TAMP_OUTPUT_FULL)
 *       the stream's units alone (ceil(L / N) + 1 rows) outgrow the scratch budget TAMP_AMD_BAD_ARGUMENT
 *       the header is not what conf makes (tamp_batch_write_ranges' rule) ....... TAMP_INVALID_CONF
 *       the stream's rows of reset_first do not hold (above) ................... TAMP_AMD_BAD_INDEX
 *       an entry of the stream out of range or order ........................... TAMP_AMD_BAD_INDEX
 *       an offset of the open segment out of the window ....................... TAMP_OOB
 *       the open segment does not parse from the last entry, or decodes to more
 *       than reset_interval bytes .............................................. TAMP_AMD_BAD_INDEX
 *       the open segment did not decode to what the walk found (a defect of the
 *       library) ............................................................... TAMP_ERROR
 *       a source byte that does not fit conf->literal bits .................... TAMP_EXCESS_BITS
 *       whatever the compress kernel says of a unit
 *       the new stream longer than out_cap[i], or than 32 bits hold ........... TAMP_OUTPUT_FULL
 *     A failing stream has out_len[i] = 0 and unspecified bytes in its slab; nothing is ever written outside [out_off[i], out_off[i] +
 *     out_cap[i]), and no other stream is affected.
 * WHAT THE INDEX IS TRUSTED FOR.  Position, as in tamp_batch_read_ranges, and only the stream's LAST entry: the open segment alone is
 * walked and decoded.  The entries in front of it are checked for range and order and nothing else, so a stream with irregular closed
 * segments (one tamp_batch_index_resets found in a reference-made file) can be appended to; only the open segment is brought onto the
 * grid.  A stream that ends with a reset has an empty open segment (m = 0): nothing is decoded, its new segments follow its bytes.
 *   mem, device, stream   TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS for one 40-byte record (its rows, which are
 *                   sized from src_len alone: ceil(L / N) closed rows and one open row per appending stream, so that nothing waits for
 *                   m; reset_first[n_streams] and the bound of new_reset_off with them) and, where an open segment is decoded, once per
 *                   slice inside the decode step, which is tamp_batch_read_ranges'.  A host-memory call is synchronous and moves ONLY
 *                   the open segments, the tables and the sources of the streams that are appended to (packed: nothing that lies
 *                   between them in `src`) up and the new tails back; the closed segments never cross the link.
 * SCRATCH is kept per HIP stream (tamp_amd_trim releases it): 35 bytes per stream of the batch, 4 per entry of the new index, and per
 * row a staging row of reset_interval bytes, a slab and 80 bytes of tables, within the budget of tamp_batch_read_ranges
 * (TAMP_AMD_RANGES_SCRATCH_MB); a call whose rows outgrow it runs in slices of whole streams (it then reads two tables of n_streams + 1
 * entries back to cut them).  With TAMP_AMD_RESETS_DEBUG set the call writes one line to stderr:
 * "[tamp_amd resets] append: <a> appends, <u> units, <s> slices, <b> bytes staged" (u: the rows, b: the bytes of the units).
 * Returns TAMP_OK (n_streams == 0: at once, nothing is done); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null conf,
 * in_off, in_len, reset_first, src_off, src_len, out_off, out_cap, out_len, status or new_reset_first, a null `in`, `src` or `out` with
 * n_streams > 0, a null new_reset_off with new_reset_cap > 0, reset_interval == 0 or one whose worst-case segment does not fit 32 bits,
 * a conf that tamp_batch_compress_resets refuses, a bad memory kind, TAMP_AMD_ALL_DEVICES, n_streams >= 2^32; TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_append(const TampAmdConf *conf, uint8_t max_window_bits,
                      const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                      const uint64_t *reset_first, const uint32_t *reset_off, uint32_t reset_interval,
                      const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len,
                      uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int8_t *status,
                      uint64_t *new_reset_first, uint32_t *new_reset_off, uint64_t new_reset_cap,
                      size_t n_streams, int mem, int device, void *stream);

/*
 * FINDING the resets of streams that came without an index: a blob of tamp_amd_compress_resets, a file, a batch whose index was not
 * kept, anything a reference Compressor(dictionary_reset=True) wrote with reset_dictionary() calls of its own or in append mode.
 * The call returns the table tamp_batch_compress_resets_index writes, found on the device: the compressed bits of every stream are
 * cut into chunks of TAMP_AMD_INDEX_RESETS_CHUNK_BITS, and the chunks of ALL streams are the units of work (a lane each).
 *   in, in_off, in_len   the streams, as for tamp_batch_decompress_resets; only read
 *   reset_first          n_streams + 1 entries, ALWAYS written: the running sum of the streams' entry counts, from 0
 *   reset_off            reset_cap entries, or NULL with reset_cap == 0 (count only).  Stream i's entries are
 *                        reset_off[reset_first[i] .. reset_first[i + 1]): the offset of the byte behind each reset, counted in the
 *                        stream's own bytes, ascending.  A reset is a FLUSH token whose predecessor token is a FLUSH
 *                        (decompressor.c:501-513): three in a row are two resets with an empty segment between them, a lone one is none
 *   closed_size          optional, parallel to reset_off: the decoded bytes of the segment each reset closes
 *   open_size            optional, n_streams entries: the decoded bytes of each stream's last (open) segment; a stream's decoded size
 *                        is the sum of its closed sizes and this.  Sizes come from the token grammar alone -- the bytes every token
 *                        produces, summed between resets; one that does not fit 32 bits saturates at 0xFFFFFFFF
 *   status[i]            the first rule that applies:
 *       the stream is shorter than its header ................................. TAMP_INPUT_EXHAUSTED, no entries
 *       a header tamp_amd_read_header refuses, a window above max_window_bits .. TAMP_INVALID_CONF, no entries
 *       more than 2^29 - 513 bytes (32-bit bit positions) ...................... TAMP_AMD_BAD_ARGUMENT, no entries
 *       any token whose offset runs out of the window .......................... TAMP_OOB, entries and sizes still as the grammar says
 *       anything else, a stream that ends inside a token included (it is walked
 *       up to its last complete token) ......................................... TAMP_OK
 *     A header without the reset bit cannot hold resets: no entries, TAMP_OK, the whole size in open_size[i].  The custom-dictionary
 *     bit does not change where tokens lie: such a stream is indexed all the same (the calls that take the index refuse it themselves).
 * CAPACITY.  More entries than reset_cap holds: the call returns 1, reset_first, open_size and status are complete and no byte of
 * reset_off or closed_size is written; call again with room for reset_first[n_streams] entries.
 * WHAT THE RESULT IS CHECKED FOR.  Positions come from the grammar alone: nothing is decoded, no window is kept.  The consumers
 * verify -- tamp_batch_decompress_resets walks every segment from the header on, tamp_batch_read_ranges checks the segments it touches.
 *   mem, device, stream   TAMP_AMD_ALL_DEVICES is not taken.  A device-memory call WAITS for one 16-byte record (the chunks of the batch),
 *                   for a 4-byte changed-flag per round of the start search -- text settles in two or three; ceil(c / 64) + 2 at most for
 *                   a longest stream of c chunks, more is TAMP_ERROR, a defect -- and for the 8-byte entry count; everything else is
 *                   asynchronous on `stream`.  A host-memory call is synchronous: the streams go up once, the tables alone come back.
 * Scratch is kept per HIP stream (about 40 bytes per chunk, 8 per entry; tamp_amd_trim releases it).  With TAMP_AMD_RESETS_DEBUG set
 * the call writes one line to stderr: "[tamp_amd resets] index: <n> streams, <c> chunks, <r> rounds, <e> entries".
 * Returns TAMP_OK, 1 (above); TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null in_off, in_len, reset_first or status, a
 * null `in` with n_streams > 0, a null reset_off with reset_cap > 0, a bad memory kind, TAMP_AMD_ALL_DEVICES, n_streams >= 2^32 (and
 * for a batch of 2^32 chunks or more); TAMP_AMD_NO_DEVICE.
 */
#define TAMP_AMD_INDEX_RESETS_CHUNK_BITS 1024
int tamp_batch_index_resets(uint8_t max_window_bits, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                            uint64_t *reset_first, uint32_t *reset_off /* NULL with reset_cap == 0 */,
                            uint32_t *closed_size /* may be NULL */, uint32_t *open_size /* may be NULL */, uint64_t reset_cap,
                            int8_t *status, size_t n_streams, int mem, int device, void *stream);

/* ---- a batch's streams packed densely on the device -----------------------------------------------
 *
 * The batch calls return their streams in slabs of worst-case size (tamp_batch_compress: 1 + ceil(9n/8) bytes for n input bytes), of
 * which about half is data.  This call copies n_streams byte ranges of one device buffer back to back into another -- what a caller
 * ships off the device, or keeps instead of the slabs.  No codec work; not in the reference.  The decoders read streams at any
 * offset, so (dst, dst_off, src_len) is an input of tamp_batch_decompress / tamp_batch_decoded_size as it stands.
 *
 *   src, src_off, src_len   stream i is src[src_off[i] .. + src_len[i]); any order, gaps and overlaps are fine; only read
 *   dst, dst_cap            room for the packed bytes; dst may have any alignment.  dst == NULL with dst_cap == 0: the size query,
 *                           only dst_off is written
 *   dst_off                 n_streams + 1 entries, ALWAYS written: dst_off[0] = 0, dst_off[i + 1] = dst_off[i] + src_len[i] rounded
 *                           up to a multiple of `align`; dst_off[n_streams] is the packed size
 *   align                   a power of two in 1 .. 4096; offsets are aligned relative to dst
 * When dst_off[n_streams] <= dst_cap: dst[dst_off[i] .. + src_len[i]) holds stream i, the bytes from there to dst_off[i + 1] are
 * zero, and no other byte is written -- none in front of dst, none at or behind dst + dst_off[n_streams].  Otherwise no byte of dst
 * is written at all (the caller compares dst_off[n_streams] with dst_cap).
 * The ranges of src that are read and dst[0 .. dst_cap) MUST NOT OVERLAP: there is no in-place packing.
 * All pointers are device memory on `device`.  The call is asynchronous on `stream` (NULL: the default stream), waits for nothing
 * and reads nothing back; its one allocation is 8 KiB of scratch kept per HIP stream (tamp_amd_trim releases it).
 * Returns TAMP_OK when the kernels were launched; TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for a null src_off, src_len
 * or dst_off, a null src with n_streams > 0, a null dst with dst_cap > 0, n_streams >= 2^32 or a bad align; TAMP_AMD_NO_DEVICE.
 * n_streams == 0 stores dst_off[0] = 0 and nothing else.
 */
int tamp_batch_pack(const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len, uint8_t *dst, uint64_t dst_cap,
                    uint64_t *dst_off /* n_streams + 1 entries */, size_t n_streams, uint32_t align, int device, void *stream);

/* ---- resumable decoding: decoder OBJECTS that survive between calls ------------------------------
 *
 * What TampDecompressor is in the reference (decompressor.h:13-57): 16 bytes of state next to a window buffer,
 * advanced by tamp_decompressor_decompress (decompressor.h:93-128, decompressor.c:371-578) with whatever input and
 * output room one call has -- TAMP_OUTPUT_FULL / TAMP_INPUT_EXHAUSTED and pick up later, mid-token if need be.
 * Here the objects live in one array (host or device memory, like every other pointer of the call):
 *   object i = states + i * state_stride:  TampAmdDecoderState (16 B), then its window of 1 << window_bits_max bytes
 * state_stride >= tamp_amd_decoder_state_size(window_bits_max), a multiple of 16.  One call advances every object by
 * one step: object i sees in[in_off[i] .. +in_len[i]) and out_cap[i] bytes of room, and status / out_len /
 * in_consumed come back as from the reference's call.  Input that was not consumed must be offered again.
 * `mem` and `stream` as for tamp_batch_compress: with TAMP_AMD_MEM_HOST the library stages the objects, input and output
 * itself on its own streams (`stream` is not used) and writes nothing of out[] behind out_len[i].
 */
typedef struct TampAmdDecoderState {
    uint32_t bit_buffer;            /* bits pulled from the input and not yet decoded, left aligned */
    uint16_t window_pos;
    uint8_t bit_buffer_pos;         /* how many */
    uint8_t token_state;            /* 0 none, 1 RLE, 2 extended match, 3 extended match with its size known */
    uint16_t pending_window_offset; /* token cut short by a full output buffer: where it copies from (RLE: its count) */
    uint16_t pending_match_size;
    uint8_t conf;                   /* header byte 0 once the header has been seen */
    uint8_t skip_bytes;             /* bytes of the pending token already delivered (before the header is
                                       complete: its stashed first byte) */
    uint8_t flags;                  /* 1 configured, 2 first header byte stashed, 4 last token was FLUSH */
    uint8_t window_bits_max;        /* capacity of the window buffer behind this state */
} TampAmdDecoderState;

size_t tamp_amd_decoder_state_size(uint8_t window_bits_max); /* 16 + (1 << window_bits_max) */

/* Replaces tamp_decompressor_init (decompressor.h:83, decompressor.c:331-347) for an object in HOST memory (copy it
 * to the device afterwards if the array lives there).  conf == NULL: the header comes from the stream.  With a conf
 * the window is seeded here unless conf->use_custom_dictionary, in which case the caller fills the window bytes
 * (at state + 16) with the dictionary, as with the reference's window buffer. */
tamp_res tamp_amd_decoder_state_init(void *state, const TampAmdConf *conf, uint8_t window_bits_max);

int tamp_batch_decompress_resume(void *states, size_t state_stride, uint8_t window_bits_max, const uint8_t *in,
                                 const uint64_t *in_off, const uint32_t *in_len, uint8_t *out, const uint64_t *out_off,
                                 const uint32_t *out_cap, uint32_t *out_len, int8_t *status, uint32_t *in_consumed,
                                 size_t n_streams, int mem, int device, void *stream);

/*
 * Objects that stay on the device, advanced a selection at a time: the receiving side of tamp_batch_compress_pieces.
 *
 * tamp_batch_decompress_pieces is tamp_batch_decompress_resume on device memory with row r of every table acting on object
 * object_index[r] (NULL: on object r): in[in_off[r] .. +in_len[r]) and out_cap[r] bytes of room at out + out_off[r] go to that
 * object, and out_len[r], status[r], in_consumed[r] are its call's results.  An object no row names is neither read nor
 * written, state or window -- a round in which few connections received anything costs what those few cost.  NAMING ONE OBJECT
 * IN TWO ROWS OF ONE CALL IS THE CALLER'S ERROR: the rows run concurrently and the object is left undefined.
 *
 * tamp_batch_decoded_size_pieces answers, for row r, what tamp_batch_decompress_pieces would report for object object_index[r]
 * given the same input and out_cap = limit[r] (NULL: no limit below 2^32 - 1): decoded_size = out_len, status, in_consumed.  It
 * starts from whatever the object's last call left -- bits in the bit buffer, a header not yet complete, a token cut short --
 * reads the object's 16 state bytes and the input, never the window, and writes nothing to `states`, so any number of rows may
 * name the same object.  One kernel, one lane per row; nothing is allocated and nothing read back.
 *
 * Both: all pointers are device memory on `device`, the call is asynchronous on `stream` (NULL: the default stream) and waits
 * for nothing.  in_consumed may be NULL.  Returns TAMP_OK when the kernel was launched (n_rows == 0: nothing is); before a device
 * is looked for, TAMP_AMD_BAD_ARGUMENT for a null table with n_rows > 0 (in_off, in_len, the size / out_len table, status; the
 * decode call: out_off and out_cap as well), null states with n_rows > 0, n_rows >= 2^32, window_bits_max outside 8..15, a
 * state_stride that is not a multiple of 16 or below tamp_amd_decoder_state_size(window_bits_max), TAMP_AMD_ALL_DEVICES;
 * TAMP_AMD_NO_DEVICE.
 */
int tamp_batch_decompress_pieces(void *states, size_t state_stride, uint8_t window_bits_max,
                                 const uint32_t *object_index /* may be NULL */, const uint8_t *in, const uint64_t *in_off,
                                 const uint32_t *in_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                 uint32_t *out_len, int8_t *status, uint32_t *in_consumed, size_t n_rows, int device,
                                 void *stream);

int tamp_batch_decoded_size_pieces(const void *states, size_t state_stride, uint8_t window_bits_max,
                                   const uint32_t *object_index /* may be NULL: row r -> object r */, const uint8_t *in,
                                   const uint64_t *in_off, const uint32_t *in_len,
                                   const uint32_t *limit /* may be NULL: none below 2^32-1 */, uint32_t *decoded_size,
                                   int8_t *status, uint32_t *in_consumed, size_t n_rows, int device, void *stream);

/* ---- compressor objects below flush granularity -----------------------------------------------
 *
 * What TampCompressor is in the reference (compressor.h:13-66): a 16-byte input ring that is parsed only while it is
 * full, an RLE run / extended match that may still be growing, a lazily cached match, up to 31 pending output bits --
 * next to the window.  tamp_batch_compress_resume runs one of the reference's calls on every object of an array
 * (same layout rule as the decoder objects: state, then the window of 1 << window_bits_max bytes; state_stride a
 * multiple of 16 and >= tamp_amd_encoder_state_size):
 *   TAMP_AMD_OP_POLL                tamp_compressor_poll (compressor.h:142)            one parse step
 *   TAMP_AMD_OP_COMPRESS            tamp_compressor_compress_cb (compressor.h:227)     sink + poll while the ring fills
 *   TAMP_AMD_OP_FLUSH               tamp_compressor_flush (compressor.h:193)
 *   TAMP_AMD_OP_COMPRESS_AND_FLUSH  tamp_compressor_compress_and_flush_cb (compressor.h:259)
 * with the reference's results per object: status (TAMP_OK / TAMP_OUTPUT_FULL / TAMP_EXCESS_BITS), bytes written,
 * input bytes consumed -- including calls whose output buffer fills up.  Whole segments (everything between two
 * flush points, known up front) are the batch kernel's job: tamp_batch_compress / tamp_amd_compress_segment.
 * Host memory as for tamp_batch_decompress_resume: library streams, `stream` not used, nothing behind out_len[i] written.
 */
typedef struct TampAmdEncoderState {
    uint32_t bit_buffer;      /* pending output bits, left aligned (the header sits here after init) */
    uint16_t window_pos;
    uint8_t bit_buffer_pos;
    uint8_t input_size;       /* bytes in the ring (0..16) */
    uint8_t input_pos;        /* ring read position */
    uint8_t window;           /* conf: window bits */
    uint8_t literal;          /* conf: literal bits */
    uint8_t flags;            /* conf: 1 custom dictionary, 2 extended, 4 dictionary_reset, 8 append, 16 lazy_matching */
    uint8_t input[16];        /* the ring */
    int16_t cached_match_index; /* lazy matching: match found for the next position, -1 = none */
    uint16_t extended_match_position;
    uint8_t cached_match_size;
    uint8_t rle_count;
    uint8_t extended_match_count;
    uint8_t last_was_flush;
    uint32_t reserved;
} TampAmdEncoderState;

enum {
    TAMP_AMD_OP_POLL = 1,
    TAMP_AMD_OP_COMPRESS = 2,
    TAMP_AMD_OP_FLUSH = 3,
    TAMP_AMD_OP_COMPRESS_AND_FLUSH = 4,
};

size_t tamp_amd_encoder_state_size(uint8_t window_bits_max); /* 40 + (1 << window_bits_max) */

/* Replaces tamp_compressor_init (compressor.h:84, compressor.c:191-244) for an object in HOST memory: header (or the
 * append marker) into the bit buffer, window seeded unless conf->use_custom_dictionary (then the caller fills the
 * window bytes at state + 40).  `append` as TampConf.append (compressor.c:227-235). */
tamp_res tamp_amd_encoder_state_init(void *state, const TampAmdConf *conf, int append, uint8_t window_bits_max);

int tamp_batch_compress_resume(void *states, size_t state_stride, uint8_t window_bits_max, int op, int write_token,
                               const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                               const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int8_t *status,
                               uint32_t *in_consumed, size_t n_objects, int mem, int device, void *stream);

/* ---- single-stream one-shot entry points (the reference's own call shapes) ------------------- */

/*
 * One stream, host buffers: tamp_compressor_init + tamp_compressor_compress_and_flush(write_token=false)
 * (compressor.h:84,280-286) as a batch of one on `device`.  *output_written_size may be NULL.
 */
tamp_res tamp_amd_compress(const TampAmdConf *conf, const unsigned char *dictionary, unsigned char *output,
                           size_t output_size, size_t *output_written_size, const unsigned char *input,
                           size_t input_size, int device);

/*
 * One stream, host buffers: tamp_decompressor_init(conf=NULL) + tamp_decompressor_decompress
 * (decompressor.h:83,128) as a batch of one on `device`.
 */
tamp_res tamp_amd_decompress(const unsigned char *dictionary, size_t dictionary_len, unsigned char *output,
                             size_t output_size, size_t *output_written_size, const unsigned char *input,
                             size_t input_size, size_t *input_consumed_size, int device);

/*
 * One SEGMENT of a stream: the bytes between two flush points, with the window carried in and out.  It is what the
 * reference's streaming calls add up to between flushes -- tamp_compressor_init (compressor.h:84; header, or with
 * conf.append the FLUSH marker of compressor.c:227-235), any number of tamp_compressor_compress (compressor.h:244)
 * and one tamp_compressor_flush(write_token) (compressor.h:193; FLUSH rule compressor.c:776-794) -- and is what
 * tamp_amd.Compressor.write()/flush()/reset_dictionary() are built from.  A segment always ends byte aligned, so the
 * carried state is just the window (1<<window bytes, ring order) and window_pos.
 *   emit_header / append_marker   how the segment opens: header byte(s), the 2-byte FLUSH marker, or nothing
 *   resume                        0: fresh stream (window_state holds the custom dictionary if conf says so, else it is
 *                                 ignored on input); 1: continue from window_state / *window_pos
 *   flush_token                   write_token of tamp_compressor_flush; *token_written tells whether one was emitted
 * window_state / *window_pos are updated on TAMP_OK.  TAMP_OUTPUT_FULL leaves them byte-identical to what they were: the
 * output holds what fitted (the rule of tamp_batch_compress) and the same call with enough room gives the whole segment.
 * Host buffers, one stream, device `device`.
 */
tamp_res tamp_amd_compress_segment(const TampAmdConf *conf, int emit_header, int append_marker, int resume,
                                   int flush_token, unsigned char *window_state, uint16_t *window_pos,
                                   unsigned char *output, size_t output_size, size_t *output_written_size,
                                   const unsigned char *input, size_t input_size, int *token_written, int device);

/*
 * One PIECE of a stream -- a tamp_compressor_compress call on an object that lives on the host as (window_state,
 * *window_pos, *carry).  With finish = 0 the piece ends exactly as the reference's call does (compressor.c:681-722: every
 * byte is taken, parse steps run only while the 16-byte ring is full, whole output bytes leave, nothing is drained) and
 * *carry receives what the reference's object still holds: a run or extended match that is still growing
 * (compressor.h rle_count, extended_match_count / _position), up to 7 pending output bits, up to 15 unparsed input
 * bytes (16 when the last poll took none).  The next piece continues from it (resume = 1).  finish = 1 ends the segment like tamp_amd_compress_segment
 * (tamp_compressor_flush with write_token = flush_token) and clears the carry.  This is what bounded-memory writers are
 * built from: tamp_amd.Compressor.write() sends a piece whenever it has gathered enough and returns the bytes written,
 * as tamp/_c_compressor.pyx:74-118 does.  With conf->lazy_matching an unfinished piece also leaves a cached match behind
 * (compressor.c:576-619), for which TampAmdCarry has no field: this call answers finish = 0 of a lazy configuration with
 * TAMP_AMD_BAD_ARGUMENT, and tamp_amd_compress_piece_lazy below takes every configuration.
 * Give a piece tamp_amd_compress_bound(input_size + 271, ...) bytes of room;
 * TAMP_OUTPUT_FULL leaves window_state / *window_pos / *carry byte-identical to what they were, and a piece with finish = 0
 * then delivers nothing (*output_written_size = 0: offered again it emits all its bytes); exact room is enough.
 */
typedef struct TampAmdCarry {
    uint8_t rle_count;   /* bytes consumed by a run that has not ended yet */
    uint8_t ext_count;   /* bytes consumed by an extended match that has not ended yet ... */
    uint16_t ext_pos;    /* ... and its window position */
    uint8_t bit_count;   /* output bits not written yet: 0..7 on return; up to 31 accepted on entry (a reference object
                            sits on its last token's bits until the next poll, compressor.c:549-551) */
    uint8_t tail_len;    /* 0..16 input bytes taken but not parsed yet; 16 on return only when the call's last poll emitted
                            a run / extended match that could not grow and so took no byte (compressor.c:449-466,505-509) */
    uint16_t reserved;
    uint32_t bits;       /* the pending bits, left aligned: first one in bit 31 */
    uint8_t tail[16];
} TampAmdCarry;
tamp_res tamp_amd_compress_piece(const TampAmdConf *conf, int emit_header, int append_marker, int resume, int finish,
                                 int flush_token, unsigned char *window_state, uint16_t *window_pos, TampAmdCarry *carry,
                                 unsigned char *output, size_t output_size, size_t *output_written_size,
                                 const unsigned char *input, size_t input_size, int *token_written, int device);

/*
 * tamp_amd_compress_piece for every configuration, lazy matching included: the same parameters and the same contract, with
 * a carry that also holds the reference object's cached_match_index / cached_match_size (compressor.c:603-608) -- the match
 * the call's last poll found one position ahead when it put a literal in front of it.  The next piece's first poll starts
 * from it.  With a configuration without lazy matching the two fields stay 0 and the bytes are those of
 * tamp_amd_compress_piece.  finish = 1 clears them with the rest of the carry; TAMP_OUTPUT_FULL of an unfinished piece
 * leaves all 32 bytes as they came.  A cached match that comes in (cached_len != 0) goes with resume = 1 and a lazy
 * configuration, excludes a pending run or extended match (poll_extended_handling clears the cache whenever it consumes),
 * lies inside the window (cached_pos + cached_len <= 1 << window) and is no longer than the tail, whose leading bytes it
 * matches (the probe saw ring bytes only): anything else is TAMP_AMD_BAD_ARGUMENT, and nothing is written.
 */
typedef struct TampAmdLazyCarry {
    TampAmdCarry carry;  /* as for tamp_amd_compress_piece */
    uint16_t cached_pos; /* window index of the match cached by the last poll's probe ... */
    uint8_t cached_len;  /* ... and its length; 0: none (a zero-filled struct is a fresh object) */
    uint8_t reserved2;
} TampAmdLazyCarry;      /* 32 bytes */
tamp_res tamp_amd_compress_piece_lazy(const TampAmdConf *conf, int emit_header, int append_marker, int resume, int finish,
                                      int flush_token, unsigned char *window_state, uint16_t *window_pos,
                                      TampAmdLazyCarry *carry, unsigned char *output, size_t output_size,
                                      size_t *output_written_size, const unsigned char *input, size_t input_size,
                                      int *token_written, int device);

/*
 * Batch piece calls: MANY streaming compressors, each handed one bounded piece, advanced together by the batch compress
 * kernel -- tamp_amd_compress_piece_lazy for every object of an array at once.  For a server with thousands of open
 * streams: message k of a stream matches against its messages 0..k-1, and a write costs no launch of its own.
 *
 * An object is 48 bytes followed by its window (1 << conf->window bytes, ring order), `object_stride` bytes apart
 * (a multiple of 16, >= tamp_amd_piece_object_size(conf->window); device memory: `objects` itself 16-byte aligned).  A
 * zero-filled object is a fresh one.  With conf->use_custom_dictionary a fresh object's window bytes are the dictionary.
 *
 * ops[i] says what object i's piece is: TAMP_AMD_PIECE_HEADER / _APPEND_MARKER (emit_header / append_marker: what leads the
 * output), _RESUME (the object carries on; without it the object is fresh and its carry is ignored), _FINISH (the piece
 * ends with a flush; without it, the way tamp_compressor_compress ends a call), _FLUSH_TOKEN (with _FINISH: flush_token),
 * _SKIP (the object takes no part: neither it, its slab nor its result rows are written, and its input and slab are not
 * read; device memory: the object and its table rows are not read either, whereas the host-memory call copies the whole
 * object array and whole tables to the device, so they must be readable there).
 *
 * THE CONTRACT.  For every object whose op is not _SKIP, status[i], out_len[i], the bytes out[out_off[i] .. + out_len[i])
 * and the object afterwards -- window, window_pos, all 32 carry bytes, token_written -- are exactly what
 * tamp_amd_compress_piece_lazy gives for that object alone with the five flags taken from ops[i] (only the block-mode
 * shortcut of a whole fresh v1 stream is not taken; it produces the same bytes).  One field is tidier here: carry.ext_pos
 * is 0 whenever carry.ext_count is 0 -- the single call leaves a position of no meaning there that depends on how its launch
 * was laid out, and here nothing about an object may depend on the other objects of the call.  So: a piece without input on a resumed
 * object polls nothing and releases the whole bytes among its pending bits; TAMP_OUTPUT_FULL and TAMP_EXCESS_BITS leave the
 * object byte for byte as it came, an unfinished piece then delivers out_len[i] = 0 and a finishing one keeps
 * tamp_batch_compress's room rule; give a piece tamp_amd_compress_bound(in_len[i] + 271, ...) of room.  Per object
 * TAMP_AMD_BAD_ARGUMENT (out_len[i] = 0, object untouched): a carry that breaks the rules of tamp_amd_compress_piece(_lazy),
 * unknown op bits, _HEADER | _APPEND_MARKER together, in_len[i] > 0xFFFFFF00 (no byte of such an object's input or slab is
 * touched, whatever its offsets say; host memory: likewise an input or slab that would end beyond 2^64).  An unfinished piece under lazy matching is
 * accepted: the object has the cached-match fields.  Nothing is written outside [out_off[i], out_off[i] + out_cap[i]), no
 * object is affected by another's failure, and with host memory nothing behind out_len[i] is written.  Slabs must not overlap.
 *
 * The call returns TAMP_AMD_BAD_ARGUMENT, before a device is looked for, for: a bad memory kind, TAMP_AMD_ALL_DEVICES
 * (objects stay on one device), n_objects >= 2^32; and with n_objects > 0 for a null conf, objects, ops, in_off, in_len,
 * out_off, out_cap, out_len or status, a stride below the object size or not a multiple of 16, device-memory objects that
 * are not 16-byte aligned.  An invalid conf: TAMP_INVALID_CONF.  n_objects == 0: TAMP_OK, nothing is done.
 * `max_in_len` is a hint that may be 0; the call measures its pieces itself.
 *
 * HOW IT RUNS.  The objects are sorted by (what leads, how the piece ends) -- at most nine classes, ONE in the steady state
 * where every stream is mid-stream with the same kind of write -- and each class that occurs is one launch of the compress
 * kernel over staged rows.  Per object and call the window is copied once each way and the input once.  THE CALL WAITS
 * ONCE, early, for an 88-byte record of class counts (as tamp_batch_compress_resets and tamp_batch_read_ranges do);
 * everything behind that wait is asynchronous on `stream`, so results are valid once `stream` is.  The staging rows are
 * per-stream scratch (tamp_amd_trim releases them).  Host memory: objects, tables and input travel to the device and back
 * inside the call, which returns complete.
 */
typedef struct TampAmdPieceObject { /* 48 bytes; the window (1 << conf->window bytes, ring order) follows */
    TampAmdLazyCarry carry;         /* as for tamp_amd_compress_piece_lazy */
    uint16_t window_pos;
    uint8_t token_written;          /* out: this call's finishing flush wrote a FLUSH token */
    uint8_t reserved[13];
} TampAmdPieceObject;
size_t tamp_amd_piece_object_size(uint8_t window_bits); /* 48 + (1 << window_bits), host only */

enum {
    TAMP_AMD_PIECE_HEADER = 1,
    TAMP_AMD_PIECE_APPEND_MARKER = 2,
    TAMP_AMD_PIECE_RESUME = 4,
    TAMP_AMD_PIECE_FINISH = 8,
    TAMP_AMD_PIECE_FLUSH_TOKEN = 16,
    TAMP_AMD_PIECE_SKIP = 128
};

int tamp_batch_compress_pieces(const TampAmdConf *conf, void *objects, size_t object_stride, const uint8_t *ops,
                               const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
                               const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int8_t *status,
                               size_t n_objects, uint32_t max_in_len, int mem, int device, void *stream);
/* Where the time of the calling thread's most recent device-memory tamp_batch_compress_pieces call went, in milliseconds
 * (hipEvents on its stream, recorded while tamp_amd_set_timing(1) is on): out4[0] classify kernel and the wait,
 * [1] stage kernel, [2] the compress launches, [3] unstage kernel; -1 each where nothing was recorded (timing off, or the
 * call launched no compress kernel).  tamp_amd_last_kernel_ms() is the whole call.  Returns TAMP_OK, or
 * TAMP_AMD_BAD_ARGUMENT for a null pointer. */
int tamp_amd_pieces_phase_ms(float *out4);

/* Replaces tamp_decompressor_read_header (decompressor.h:67, decompressor.c:276-297): host-side header parse. */
tamp_res tamp_amd_read_header(TampAmdConf *conf, const unsigned char *input, size_t input_size,
                              size_t *input_consumed_size);

/* Timing hook for bench.py: duration in milliseconds of the most recent codec kernel launched by this
 * thread on `device`, measured with hipEvents on the stream the kernel ran on; < 0 if none recorded.
 * Enabled by tamp_amd_set_timing(1).  After tamp_amd_compress_resets: all kernels of the call, as one figure. */
void tamp_amd_set_timing(int enabled);
float tamp_amd_last_kernel_ms(void);

/* Releases the device scratch the library keeps between calls on `device`, one set per HIP stream that a call ever ran on:
 * the global-window decoder's slab (4 GiB at most), the split decoder's token records (up to a quarter of the free device
 * memory, 8 GiB at most), the block-mode tables of one long v1 stream (up to 3 bytes per input byte), the gathered tables of
 * the expensive-first ordering (37 bytes per stream of the batch), the slabs of tamp_amd_compress_resets, the tables, stage and scratch of tamp_batch_read_ranges, the tables, staging rows and slabs of tamp_batch_write_ranges, the tables, staged entries, staging rows and slabs of tamp_batch_append, the 8 KiB of tamp_batch_pack's scan, the tables, state rows and input rows of tamp_batch_compress_pieces and the long-stream decoder's chunk tables, tail maps and
 * lag lists -- and the staging buffers of the host-memory calls (pinned host memory sized by the largest
 * output extent ever staged, device chunk buffers, the object calls' state rows: the batch, resume, segment and piece calls
 * and the reference-named objects share them).  Synchronises those streams first.  Returns the bytes released or a negative TAMP_AMD_* code.
 * (The library itself falls back to decoders without scratch when an allocation fails; this call is for callers that
 * want the memory back.) */
long long tamp_amd_trim(int device);

#ifdef __cplusplus
}
#endif
#endif /* TAMP_AMD_H */
