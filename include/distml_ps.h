/*
 * distml_ps.h — C-ABI of the MI355X parameter-server push-reduce path.
 *
 * Drop-in boundary: this library replaces the body of DistML's server-side
 * plugin `abstract class DataStore` (reference: src/main/java/com/intel/distml/
 * util/DataStore.java:17-92) and its seven typed implementations under
 * util/store/. Every entry point names the reference method it replaces.
 * Plain C types only: a JNI shim, ctypes, or C++ can bind it.
 *
 * Threading: every call on one store is serialized by a mutex inside the store
 * (the reference calls a store from the PSAgent selector thread, Akka dispatcher
 * threads and the PSSync thread, PSAgent.java:278, PSActor.java:171-251,
 * PSSync.java:131). Each store owns one HIP stream on its device; every call
 * does hipSetDevice, so any host thread may call.
 *
 * Status codes map 1:1 to the exceptions the reference throws:
 *   DML_E_BAD_DESC          IllegalArgumentException  (DataStore.java:91)
 *   DML_E_KEY_OUT_OF_SHARD  ArrayIndexOutOfBoundsException (localData[indexOf(key)])
 *   DML_E_TRUNCATED         ArrayIndexOutOfBoundsException (readInt/readFloat past data.length)
 *   DML_E_NEGATIVE_COUNTER  IllegalStateException (IntMatrixStore.java:174-176, IntArrayStore.java:108-110)
 * After one of these four the store holds exactly the values the reference
 * store holds when its exception escapes handlePush (every add before the
 * failing position applied, nothing after it), and the error is recorded in
 * dml_store_error_state(). DML_E_* codes >= 16 are library/usage errors with
 * no reference counterpart.
 */
#ifndef DISTML_PS_H
#define DISTML_PS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* DataDesc constants (DataDesc.java:10-19). */
#define DML_DATA_TYPE_ARRAY   0
#define DML_DATA_TYPE_MATRIX  1
#define DML_KEY_TYPE_INT      0
#define DML_KEY_TYPE_LONG     1
#define DML_ELEMENT_TYPE_INT    0
#define DML_ELEMENT_TYPE_FLOAT  1
#define DML_ELEMENT_TYPE_LONG   2
#define DML_ELEMENT_TYPE_DOUBLE 3

/* Status codes. */
#define DML_OK                   0
#define DML_E_BAD_DESC           1
#define DML_E_KEY_OUT_OF_SHARD   2
#define DML_E_TRUNCATED          3
#define DML_E_NEGATIVE_COUNTER   4
#define DML_E_INVALID_ARG       16
#define DML_E_HIP               17
#define DML_E_NOMEM             18
#define DML_E_UNSUPPORTED       19
#define DML_E_CAPACITY          20

/* Store option flags (dml_store_create_range `flags`). */
/* FloatArrayStore reads records with VALUE_SIZE = 8 (FloatArrayStore.java:15)
 * although every writer emits key|f32 records (SparseArray.java:63-76). The
 * default follows the writer (stride keySize+4); this flag reproduces the
 * reference's stride keySize+8 read bit for bit (SURVEY.md defect 1). */
#define DML_FLAG_FLOAT_ARRAY_REF_STRIDE  0x1
/* Apply pushes asynchronously: dml_store_push returns once the bytes are
 * captured (staged); a deferred error surfaces at the next call. Default is
 * synchronous: the call returns after the apply, like the reference's ack
 * (PSAgent.java:278-281). */
#define DML_FLAG_ASYNC                   0x2
/* No identity speculation / slot reuse. By default a plain-sum
 * matrix store that receives full-range device pushes allocates a second shard
 * buffer (rows*cols values) on first use, when the device has that plus
 * max(1/8 of its memory, 4 GiB) free; this flag never allocates it. */
#define DML_FLAG_NO_SPECULATION          0x4

/* Mirrors the six big-endian int32s DataDesc puts on the wire, in wire order
 * (DataDesc.java:62-69). key/value sizes derive as in DataDesc.java:50-51. */
typedef struct dml_desc {
    int32_t data_type;
    int32_t key_type;
    int32_t value_type;
    int32_t dense_row;
    int32_t dense_column;
    int32_t ada_grad;
} dml_desc;

typedef struct dml_store dml_store; /* opaque; one per (matrix, shard) */

/* --- lifecycle --------------------------------------------------------- */

/* == DataStore.createStore(serverIndex, matrix) (DataStore.java:50-92) for a
 * KeyRange shard [first_key, last_key] (KeyRange.linearSplit, KeyRange.java:68-80),
 * followed by the store's init(keys[, cols]) (e.g. FloatMatrixStore.java:28-37):
 * the shard is zero-filled in HBM. `cols` is ignored for ARRAY stores. */
int dml_store_create_range(const dml_desc* desc, int64_t first_key, int64_t last_key,
                           int32_t cols, int32_t device, uint32_t flags, dml_store** out);
void dml_store_destroy(dml_store* s);

/* KeyRange.linearSplit(n) (KeyRange.java:68-80): shard i = [first_out[i], last_out[i]]. */
int dml_linear_split(int64_t first_key, int64_t last_key, int32_t n,
                     int64_t* first_out, int64_t* last_out);

/* --- the hot path: handlePush ------------------------------------------ */

/* == store.handlePush(format, data) (DataStore.java:30; FloatMatrixStore.java:200-238,
 * FloatArrayStore.java:110-122, IntMatrixStore.java:154-195, IntArrayStore.java:97-113,
 * FloatMatrixStoreAdaGrad.java:239-306, DoubleArrayStore.java:115-127,
 * DoubleMatrixStore.java:153-190). `data` is a host buffer BORROWED for the
 * call only (the JVM byte[]). Records use the store's own DataDesc
 * (PSAgent.java:279 passes the server-side format). */
int dml_store_push(dml_store* s, const uint8_t* data, int64_t len);

/* n sequential handlePush calls, bucket 0 first, applied as ONE ordered
 * multi-bucket reduce: each element is summed in push order, so the result is
 * bit-identical to calling handlePush n times. Host buffers, borrowed. */
int dml_store_push_batch(dml_store* s, const uint8_t* const* bufs, const int64_t* lens, int32_t n);

/* Same, for buckets already resident in device memory on the store's device
 * (the device-resident north-star path). Buffers must stay valid until the
 * next dml_store_flush (or any read call).
 *
 * Device push placement (this call, dml_reduce_buckets_dense, dml_prereduce_begin,
 * dml_prereduce_begin_ctx, dml_shard_split and the dml_group_push_* calls):
 * every dev_bufs[i] is 4-byte aligned, nothing more; a pointer that is not gets
 * DML_E_INVALID_ARG before anything is launched or any state changes. The group
 * calls check it with their other arguments, before the group's state moves and
 * before the rank joins the call's collective: like a null pointer it is a
 * caller's error that every rank must avoid, not a failure the collective
 * absorbs with zeros. A push is
 * read only inside [dev_bufs[i], dev_bufs[i] + lens[i]), and never written, so
 * pushes may lie back to back in one buffer (as the exchange path's receive
 * buffer holds them) or against other live data. */
int dml_store_push_batch_device(dml_store* s, const void* const* dev_bufs, const int64_t* lens, int32_t n);

/* Read barrier: every accepted push is applied; returns any deferred error. */
int dml_store_flush(dml_store* s);

/* Buffer release without a full flush (no reference counterpart: the JVM's
 * byte[] is always copied). Every push call (dml_store_push, _push_batch,
 * _push_batch_device) is numbered 1, 2, ...; dml_store_push_seq returns the
 * number of the last accepted one. dml_store_retire(s, seq) finishes every chunk
 * of the calls up to `seq` on the host (exact replays, int32 rollbacks, re-runs of
 * failed speculation: the reads of a push that may follow its device apply); when
 * it returns, those calls' device buffers are no longer read and may be reused or
 * freed. Returns the first error those chunks met (sticky, as for flush). */
int dml_store_push_seq(dml_store* s, uint64_t* seq);
int dml_store_retire(dml_store* s, uint64_t seq);

/* Pipeline counters since creation or the last reset (diagnostic): chunks
 * retired, speculative chunks and how many of them re-ran without speculation,
 * and per push how its records found their rows: identity (record r = row r,
 * verified in the reduce), reused (a kept slot-table column, verified), indexed
 * (the key index). Counted when a chunk retires: flush first. */
typedef struct dml_store_counters {
    int64_t chunks;
    int64_t spec_chunks;
    int64_t spec_reruns;
    int64_t identity_pushes;
    int64_t reused_pushes;
    int64_t indexed_pushes;
    int64_t sparse_big_chunks;  /* array chunks applied through the one-level partition (big leaves) */
    int64_t sparse_replays;     /* array chunks with leaves the exact replay applied */
    int64_t ident_launches;     /* chunks / pre-reduce pieces launched through the all-identity
                                   kernels (k_flat_ident, k_ada_ident) */
    int64_t sparse_counted_chunks; /* array chunks whose apply read the counted partition's layout: a
                                   bin, leaf or slice region of the single-pass partition overflowed,
                                   or compact records met a cutoff. 0 from
                                   dml_prectx_stats and dml_group_prereduce_stats */
} dml_store_counters;
int dml_store_stats(dml_store* s, dml_store_counters* out, int32_t reset);

/* First error the store has seen (sticky until dml_store_clear_error):
 * status code, the key and column the reference would report, 0 if none. */
int dml_store_error_state(dml_store* s, int64_t* bad_key, int32_t* bad_col);
void dml_store_clear_error(dml_store* s);

/* --- shard access ------------------------------------------------------ */

/* KeyRange size (KeyRange.java:92-94) and rowSize() (FloatMatrixStore.java:24-26;
 * 1 for arrays). */
int dml_store_shape(dml_store* s, int64_t* rows, int32_t* cols);
/* The store's DataDesc value type (DML_ELEMENT_TYPE_*) and whether it is an AdaGrad
 * store (DataDesc.java:21-42): the element type its rows hold for dml_store_read_rows
 * (the JNI snapshot checks the Java array it fills against it). */
int dml_store_value_type(dml_store* s, int32_t* value_type, int32_t* adagrad);

/* Raw row-major shard values (rows*cols elements of the store's value type)
 * to/from host memory; test/oracle access and initial load. */
int dml_store_read_dense(dml_store* s, void* host_dst, int64_t bytes);
int dml_store_write_dense(dml_store* s, const void* host_src, int64_t bytes);
/* Device pointer of the value array (rows*cols elements) as of this call; valid
 * until the next push (a speculative full-range batch writes the store's second
 * buffer and commits it) or destroy. */
int dml_store_device_ptr(dml_store* s, void** dev_ptr);
/* AdaGrad side arrays (FloatMatrixStoreAdaGrad.java:23-24), f32 row-major. */
int dml_store_read_adagrad(dml_store* s, float* alpha_dst, float* delta_dst, int64_t elems);
/* Local rows [row0, row0 + nrows) of the shard's values (which 0, the store's value
 * type), or of AdaGrad's alpha (1) / delta (2) (f32), row-major and native-endian,
 * after every accepted push: the snapshot behind the stores' Iter, which the
 * result-collect paths read (DoubleArrayStore.java:129-157, FloatMatrixStore.java:241-269,
 * FloatArrayStore.java:124-152, FloatMatrixStoreAdaGrad.java:308-337; called from
 * LogisticRegression.scala:290-291 and Word2Vec.scala:814-817). Row ranges let a JVM
 * fill its heap arrays in bounded chunks. */
int dml_store_read_rows(dml_store* s, int32_t which, int64_t row0, int64_t nrows, void* host_dst, int64_t bytes);

/* DataStore.rand() (DataStore.java:22; PSActor OP_RAND, PSActor.java:181-201).
 * DoubleMatrixStore: exactly the reference's values — java.util.Random(1L) on every
 * shard, |nextGaussian()| per element, each row divided by its L2 norm
 * (DoubleMatrixStore.java:192-207); `seed` is not used. Float matrices, AdaGrad
 * included, draw from an unseeded java.util.Random in the reference
 * (FloatMatrixStore.java:44, FloatMatrixStoreAdaGrad.java:60), which nothing can
 * reproduce: here (a/100f - 0.5f)/rowSize with a uniform a in 0..99, in float
 * arithmetic, from a counter-based generator seeded by `seed`. Other stores: no-op. */
int dml_store_rand(dml_store* s, uint64_t seed);
/* Fill every value with v: FloatMatrixStore.setValue (FloatMatrixStore.java:61-71), what
 * set(String) does on the float matrix stores (:53-55, FloatMatrixStoreAdaGrad.java:69-71).
 * The reference's zero() is a no-op on every store (DataStore.java:24; the float stores'
 * zero(String) is an overload OP_ZERO never calls) and set() a no-op on the others: the
 * DataStore mirrors (GpuDataStore.java, distml_amd/store.py) call this only where the
 * reference's store would change. */
int dml_store_fill(dml_store* s, double v);
/* FloatMatrixStoreAdaGrad.setAlpha(initialAlpha, minAlpha, factor) (:77-82). */
int dml_store_set_alpha(dml_store* s, float initial_alpha, float min_alpha, float factor);
/* maxDelta / maxDeltaRow / maxDeltaCol printed by AdaGrad handlePush (:246, :273-277). */
int dml_store_max_delta(dml_store* s, float* max_delta, int32_t* row, int32_t* col);

/* == handleFetch(format, rows), dense-column layout (FloatMatrixStore.java:113-174,
 * IntMatrixStore.java:81-140, FloatArrayStore.java:88-108, IntArrayStore.java:78-95,
 * DoubleArrayStore.java handleFetch, FloatMatrixStoreAdaGrad.java:146-213).
 * `keys` are the intersected keys in the caller's iteration order; every key
 * must lie in the shard. Writes the reference byte layout to `out`.
 * The check is by range (first <= key <= last as 64-bit values), not by indexOf's narrowed
 * index: any other key is refused with DML_E_KEY_OUT_OF_SHARD before anything is copied. */
int dml_store_fetch(dml_store* s, const int64_t* keys, int64_t nkeys,
                    uint8_t* out, int64_t cap, int64_t* out_len);
/* Same for a KeyRange request: keys first..last ascending (KeyRange.intersect). */
int dml_store_fetch_range(dml_store* s, int64_t first_key, int64_t last_key,
                          uint8_t* out, int64_t cap, int64_t* out_len);

/* == handleFetch for a worker whose buffers are in HBM (no reference counterpart: the
 * JVM's fetch returns a byte[]). The same bytes as dml_store_fetch / _fetch_range —
 * the dense-column layouts of all seven stores: matrices [K-byte key LE][cols x value LE]
 * (FloatMatrixStore.java:113-174, IntMatrixStore.java:81-140, DoubleMatrixStore.java:80-139),
 * AdaGrad [value][alpha] pairs in 8-byte slots (FloatMatrixStoreAdaGrad.java:146-213),
 * arrays [key][value] with FloatArrayStore's 8-byte slot and zero pad
 * (FloatArrayStore.java:88-108, IntArrayStore.java:78-95, DoubleArrayStore.java:93-113)
 * — encoded straight into device memory on the store's device, from int64 keys that
 * are in device memory too (_device) or for the keys of a KeyRange (_range_device,
 * clipped to the shard by KeyRange.intersect, KeyRange.java:124-136, as
 * dml_store_fetch_range clips; the range form reads no key array). For a plain store a
 * fetched record is byte for byte a push record, so the output can be handed to
 * dml_store_push_batch_device of another store of the same shape (standby, re-shard).
 *
 * Entry: like every read, the call first retires every accepted push and returns a
 * deferred error exactly as dml_store_fetch would.
 *
 * Arguments: *out_len = nkeys x record bytes is set on the host first (0 for an empty
 * intersection, which returns DML_OK with nothing launched, and for nkeys < 0).
 * DML_E_INVALID_ARG, with nothing launched and no store state changed: a null out_len,
 * nkeys < 0, a null dev_keys with nkeys > 0, dev_keys not 8-byte aligned, dev_out not
 * 4-byte aligned. DML_E_CAPACITY: cap < *out_len, or a null dev_out with *out_len > 0.
 * dev_out needs the alignment of a device push and nothing more (4 bytes), and only
 * [dev_out, dev_out + *out_len) is ever written, so a fetch can be written straight
 * into a packed send buffer, between other live data.
 *
 * Ordering: the encode is enqueued on the store's apply stream (dml_store_stream).
 * With a non-null `stream` (a hipStream_t of the store's device) the call does not
 * wait for it: it records an event behind the encode and makes `stream` wait for that
 * event, and the caller orders its own work on `stream`. stream == NULL makes the call
 * synchronous: it returns after the bytes are written. dev_keys and dev_out must stay
 * valid until then. Kernels of later pushes queue behind the fetch on the apply
 * stream, so a fetch sees every push accepted before it and none accepted after it,
 * with no flush in between (DESIGN.md §4.10 says why that holds for the second shard
 * buffer of speculative chunks).
 *
 * Keys are checked on the device, by range as 64-bit values (first <= key <= last) as
 * dml_store_fetch checks them. For a key outside the shard nothing is read from the
 * shard and no byte of that key's record is written; the lowest list index of such a
 * key is kept and comes home through a pinned word behind the encode. stream == NULL:
 * the call itself returns DML_E_KEY_OUT_OF_SHARD. Otherwise the flush, or the next
 * call into the store that finds the encode finished (a push does not wait for it; a
 * read does), returns it. Either way the store's error state holds that key and col -1,
 * sticky until dml_store_clear_error, as after the host fetch. The one difference from
 * the host call: dml_store_fetch refuses before anything is copied, while this call
 * has already written the records of the good keys.
 *
 * A group rank uses these calls on its dml_group_store handle after dml_group_flush,
 * like every other read of that handle. */
int dml_store_fetch_device(dml_store* s, const int64_t* dev_keys, int64_t nkeys,
                           void* dev_out, int64_t cap, int64_t* out_len, void* stream);
int dml_store_fetch_range_device(dml_store* s, int64_t first_key, int64_t last_key,
                                 void* dev_out, int64_t cap, int64_t* out_len, void* stream);
/* Output bytes of one wave instruction's 64 vectors and of one block's tile in the
 * device fetch's encode kernel (k_fetch_vec): the sizes its tests place stream ends at. */
#define DML_FETCH_WAVE_BYTES 1024
#define DML_FETCH_BLOCK_BYTES 4096

/* writeAll/readAll (FloatMatrixStore.java:74-91 etc.): big-endian row-major
 * values, the bytes DataOutputStream.writeFloat/writeInt/writeDouble emit.
 * read_all assigns the elements the stream holds before failing with
 * DML_E_TRUNCATED when it is short (readFloat's EOFException). */
int dml_store_write_all(dml_store* s, uint8_t* out_be, int64_t cap, int64_t* out_len);
int dml_store_read_all(dml_store* s, const uint8_t* in_be, int64_t len);
/* syncTo/syncFrom(stream, fromRow, toRow) (FloatMatrixStore.java:94-110,
 * IntArrayStore.java:64-75 etc.; called by PSSync.java:131,160): local rows
 * from..to inclusive, big-endian. to < from moves nothing; a negative from
 * fails before any byte; rows past the shard fail with DML_E_KEY_OUT_OF_SHARD
 * after the rows before them were moved (the reference's
 * ArrayIndexOutOfBoundsException). sync_from uses the intended row layout
 * (defect 5). */
int dml_store_sync_to(dml_store* s, int32_t from_row, int32_t to_row, uint8_t* out_be, int64_t cap,
                      int64_t* out_len);
int dml_store_sync_from(dml_store* s, int32_t from_row, int32_t to_row, const uint8_t* in_be, int64_t len);

/* Pinned host memory for callers that receive pushes or return fetches through
 * it (a JNI DirectByteBuffer over it lets NIO read a PushRequest straight into
 * DMA-able memory, PSAgent.java:27-62): pushes from it are DMA'd without
 * staging, fetch / write_all / sync_to into it skip the bounce buffers. */
int dml_host_alloc(int64_t bytes, void** host_ptr);
void dml_host_free(void* host_ptr);

/* --- stream / timing / device reduce building blocks ------------------- */

/* hipStream_t of the store, as void*. */
int dml_store_stream(dml_store* s, void** stream);
/* When enabled, the store brackets launches of its dominant reduce kernel with
 * HIP events on its stream: every launch for enable == 1, one matrix chunk in
 * `enable` for enable > 1 (events in every dispatch lengthen the boundary between
 * two reduces); dml_store_kernel_time returns the summed elapsed ms and the
 * number of timed launches since the last reset. */
int dml_store_set_timing(dml_store* s, int32_t enable);
int dml_store_kernel_time(dml_store* s, double* total_ms, int64_t* launches, int32_t reset);
/* The instantiation of that dominant kernel as last launched, in rocprof's
 * spelling without "void " and the parameter list (e.g.
 * "dml::k_reduce_rows<float, 0, 4, 4, true, true, 1, 4, 0>"); "" before any push.
 * bench.py reports a profile's counted HBM bytes only for the kernel that ran. */
int dml_store_kernel_name(dml_store* s, char* out, int32_t cap);

/* Elementwise shard += src for a dense device buffer of rows*cols values in the
 * store's layout (owner-side apply after a reduce-scatter). */
int dml_store_apply_dense_device(dml_store* s, const void* dev_src, int64_t elems);
/* shard = src for a dense device buffer of rows*cols values in the store's
 * layout, on the store's stream, ordered after every accepted push and before
 * every later one: the owner's commit of its slice when a chained
 * reduce-scatter (dml_group_push_chained) brings it home. The slice started
 * from the shard and every rank added its rows to it one IEEE rounding at a
 * time, so the assignment leaves what the reference's row[i] += v loops leave
 * (FloatMatrixStore.java:200-222, DoubleMatrixStore.java:153-190). Plain
 * dense-column matrices only (f32 / f64 / i32). Earlier pushes are retired
 * first, so the copy lands in the buffer the last of them wrote (a speculative
 * batch commits the store's second buffer); dml_store_device_ptr's validity
 * rule is unchanged. dev_src is read on the store's stream: keep it until that
 * stream has passed the copy (an event, or dml_store_flush). */
int dml_store_assign_dense_device(dml_store* s, const void* dev_src, int64_t elems);
/* The owner's commit of a chained AdaGrad slice (dml_group_push_chained on an
 * AdaGrad group), on the store's stream, ordered after every accepted push and
 * before every later one like dml_store_assign_dense_device. dev_data and
 * dev_delta hold rows*cols f32 each, dev_marks one uint32 per row (non-zero: some
 * rank's accepted push listed the row in this call), dev_maxdelta_record the
 * slice's travelling record (DML_MAXDELTA_RECORD_BYTES). shard data = dev_data,
 * shard delta = dev_delta; where the row's mark is set and delta > 1,
 * alpha = (float)(initialAlpha / (factor * sqrt((double)delta))), clamped to
 * minAlpha, with the store's own parameters (dml_store_set_alpha): inside one
 * call delta never falls, so that is the alpha the reference's last update of the
 * element leaves (FloatMatrixStoreAdaGrad.java:268-272). A row no push listed
 * keeps its alpha even where its delta is above 1 (setAlpha rewrites every
 * alpha). The store's running maxDelta (value, row, col) becomes the record's.
 * One divergence: an element whose delta is NaN (a NaN gradient reached it in
 * this call) keeps the alpha the store held, where the reference leaves the
 * alpha of its last non-NaN delta above 1; dml_group_push_exchange is the path
 * without it. The buffers are read on the store's stream: keep them until that
 * stream has passed the commit. */
#define DML_MAXDELTA_RECORD_BYTES 32
int dml_store_assign_adagrad_device(dml_store* s, const void* dev_data, const void* dev_delta, const void* dev_marks,
                                    const void* dev_maxdelta_record);
/* The owner's commit of a chained int32 slice (dml_group_push_chained_i32), on
 * the store's stream, ordered like dml_store_assign_dense_device: shard =
 * dev_src, and the slice's verdict record (DML_CHAIN_I32_RECORD_BYTES, 8-byte
 * aligned, device memory) is merged into the store's own device-resident record:
 * the first closed record to come home stays. The store's record is then copied
 * to pinned host memory; when the store next retires that work (a read,
 * dml_store_flush, a later push once the copy has finished) a closed record puts
 * it into its usual error state: sticky DML_E_NEGATIVE_COUNTER with the record's
 * key and col from dml_store_error_state, later pushes refused
 * (IntMatrixStore.java:174-176, PSAgent.java:188-191). A closed slice holds every
 * add up to and including the failing one and nothing after it, so the
 * assignment leaves what the reference's store holds when its exception escapes.
 * Dense int32 matrices only; other stores: DML_E_UNSUPPORTED. Both buffers are
 * read on the store's stream: keep them until that stream has passed the commit.
 * The record: [u64 pos][i64 key][i32 col][i32 ring step][u64 pad]; pos is all
 * ones while the slice is open, otherwise (push << 40) | byte offset of the
 * failing add in the closing rank's push. */
#define DML_CHAIN_I32_RECORD_BYTES 32
int dml_store_assign_dense_i32_device(dml_store* s, const void* dev_src, int64_t elems, const void* dev_record);
/* Two-moment AdaGrad owner apply: dev_src holds rows x [cols Σu |
 * cols Σu²] f32 (the reduce-scattered dml_prereduce_moments_piece output of the
 * shard's rows); data += Σu, delta += Σu², alpha = initialAlpha / (factor *
 * sqrt(delta)) clamped to minAlpha where delta ends above 1, maxDelta updated
 * (FloatMatrixStoreAdaGrad.java:262-277 for the summed update; ties of maxDelta
 * go to the first element in row-major order). Within 1e-6 of the sequential
 * reference, not bit-exact: the exact path is dml_group_push_exchange.
 * Arithmetic, as tests/moments_expect.py models it bit for bit: one fp32 add
 * each for data and delta; alpha = (float)((double)initialAlpha / ((double)factor
 * * sqrt((double)delta))) where the new delta is above 1; an element whose delta
 * rose strictly is a maxDelta candidate, the best one (largest delta, then lowest
 * row-major position) replaces the running record when strictly above it.
 * Known divergences from the reference:
 *  1. maxDelta ties: the first element in row-major order, not the first in push /
 *     record order (FloatMatrixStoreAdaGrad.java:273-277).
 *  2. NaN / Inf: an element whose delta ends NaN keeps its alpha and is no
 *     candidate; Inf gives minAlpha.
 *  3. setAlpha: dev_src carries no mark of the rows a push listed, so alpha is
 *     rewritten at every element whose delta ends above 1. The reference rewrites
 *     it only on elements of rows a push lists (:268-272): after
 *     dml_store_set_alpha with a new initialAlpha, a row with delta above 1 that
 *     this call's pushes do not list keeps initialAlpha there and gets f(delta)
 *     here (dml_store_assign_adagrad_device handles the same case with touched
 *     marks). Likewise an unlisted row's -0.0 data becomes +0.0 (-0.0 + +0.0).
 * dml_group_push_exchange and dml_group_push_chained are the paths without
 * these. */
int dml_store_apply_adagrad_moments_device(dml_store* s, const void* dev_src, int64_t rows);

/* Ordered reduce of n device-resident full-range buckets into a dense device
 * buffer `dev_out` (rows*cols values of `value_type`, row = key - first_key):
 * out = b0 + b1 + ... in push order (rows no bucket touches are zero).
 * The multi-GPU pre-reduce before the reduce-scatter. Runs on `stream`.
 * Pushes: 4-byte aligned, read inside [ptr, ptr + len) only, may be adjacent
 * (see dml_store_push_batch_device). */
int dml_reduce_buckets_dense(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols,
                             const void* const* dev_bufs, const int64_t* lens, int32_t n,
                             void* dev_out, void* stream);

/* Piecewise pre-reduce for pipelining with the reduce-scatter: _begin enqueues
 * the key index of the n (<= 64) full-range pushes on `stream`; each _piece
 * writes the ordered sum of rows r(t) = (t / row_block) * row_stride + row_off
 * + t % row_block, t < ntask_rows, to dev_out + t*cols (rows >= `rows`, the
 * padding of linearSplit's short last shard, are zeros); _end waits for the
 * index and every piece and reports key-out-of-matrix / repeated-row errors.
 * Each piece runs on its own `stream` argument (0 = the null stream), which may
 * differ from _begin's (the first such piece waits for the index on the host),
 * so the next call's index can overlap the current call's pieces. Opaque handle.
 * Pushes: 4-byte aligned, read inside [ptr, ptr + len) only, may be adjacent
 * (see dml_store_push_batch_device); a piece writes only its ntask_rows x cols
 * values at dev_out. */
typedef struct dml_prereduce dml_prereduce;
int dml_prereduce_begin(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols,
                        const void* const* dev_bufs, const int64_t* lens, int32_t n, void* stream,
                        dml_prereduce** out);
int dml_prereduce_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                        int64_t ntask_rows, void* dev_out, void* stream);
int dml_prereduce_end(dml_prereduce* p);
/* One step of a chained (ring-ordered) reduce-scatter, for plain fp32 / fp64
 * matrices: like _piece (same row map, stream rule, host wait for the index
 * when `stream` differs from _begin's, completion event for _stream_wait,
 * timing), but task row t starts from dev_base + t*cols instead of zero. The
 * handle's pushes' records of model row r(t) are added to it in push order,
 * one IEEE rounding per add, exactly as the store's own push adds them
 * (FloatMatrixStore.java:200-222, DoubleMatrixStore.java:153-190), and the row
 * is written to dev_out + t*cols. dev_out == dev_base (in place) is allowed.
 * A row no push lists is copied bit for bit: it gets no add of +0.0, which
 * would turn a -0.0 into +0.0. Padding rows (r(t) >= rows) are copied too. A
 * slice handed from rank to rank through one such piece each therefore holds
 * what one reference store holds after handlePush of the ranks' pushes in ring
 * order — an arrival order the reference's server may see (PSAgent.java:166-186).
 * Nothing unverified is written: a handle with no pushes, or whose index found a
 * key outside the matrix or a row listed twice in one push, copies dev_base to
 * dev_out (_end reports the error); ascending full-range pushes of a narrow-row
 * matrix are checked key by key before the first piece. DML_E_UNSUPPORTED for
 * int32 and AdaGrad descriptors (AdaGrad: dml_prereduce_chain_piece_ada; int32:
 * dml_group_push_exchange) and for a handle
 * begun in a speculative context (dml_prereduce_begin_ctx), whose verdict comes
 * after the piece has run. */
int dml_prereduce_chain_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                              int64_t ntask_rows, const void* dev_base, void* dev_out, void* stream);
/* _chain_piece for an AdaGrad matrix (a handle begun with the AdaGrad
 * descriptor, FloatMatrixStoreAdaGrad): the slice travels as two f32 planes,
 * data and delta, plus one uint32 touched mark per task row, and a travelling
 * maxDelta record of DML_MAXDELTA_RECORD_BYTES in device memory (at ring step 0:
 * the owner's running value, row, col, the rest zero). Row map, stream rule,
 * completion event and timing are _chain_piece's. Task row t starts from
 * base_data + t*cols and base_delta + t*cols; every push's record of its model
 * row is applied in push order as the reference applies it
 * (FloatMatrixStoreAdaGrad.java:249-284): data += g, delta += g*g, one IEEE
 * rounding each; both planes are written to out_data / out_delta (out == base
 * is allowed, plane by plane). All pushes of the handle go through one pass:
 * the planes are read once and written once whatever the push count. No alpha
 * is read or written here; the owner computes it once at its commit
 * (dml_store_assign_adagrad_device). A listed row of a good handle sets
 * out_marks[t]; other rows copy base_marks[t] (base_marks == NULL reads as all
 * clear). A row no push lists, a padding row, and every row of a handle whose
 * index failed are copied bit for bit in both planes. maxDelta: every element's
 * last strict rise of delta is a candidate; the candidates of this rank's pieces
 * over one slice merge (largest value, then earliest position in push, record,
 * column order) and, with last_piece != 0, are applied to the record with the
 * reference's strict > (FloatMatrixStoreAdaGrad.java:273-277), so an earlier rank
 * of the ring keeps a tie. Pass last_piece on the last piece of the rank's step
 * over the slice, and issue one slice's pieces of a handle on one stream.
 * DML_E_UNSUPPORTED for a plain-fp32 or int32 handle and for a speculative
 * context's handle. */
int dml_prereduce_chain_piece_ada(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, const void* base_data, const void* base_delta,
                                  const void* base_marks, void* out_data, void* out_delta, void* out_marks,
                                  void* maxdelta_record, int32_t last_piece, void* stream);
/* One piece of a ring step of the chained reduce-scatter of a dense int32 matrix
 * (IntMatrixStore, LightLDA's word-topic counts). Row map, stream rule, host
 * wait and completion event as dml_prereduce_chain_piece. Task row t starts
 * from dev_base + t*cols; the handle's pushes' records of its model row are
 * added in push order, each add wrapping mod 2^32 and checked: the earliest
 * position (push << 40 | byte offset) whose add left a counter negative is kept
 * in the handle's control block (an atomic minimum over every piece of the
 * step). Every add is made; dml_prereduce_chain_close_i32 undoes the later ones
 * once all pieces of the step have run. The row is written to dev_out + t*cols;
 * dev_out == dev_base works. Copied bit for bit, nothing added: every row when
 * dev_record (the slice's verdict record, DML_CHAIN_I32_RECORD_BYTES, 8-byte
 * aligned, read only) arrived closed; every row when the handle's index found a
 * key outside the matrix or a row listed twice in one push (_end reports it);
 * a row no push lists; a padding row.
 * DML_E_UNSUPPORTED for handles that are not dense int32 matrices and for a
 * speculative context's handle. */
int dml_prereduce_chain_piece_i32(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, const void* dev_base, void* dev_out, const void* dev_record,
                                  void* stream);
/* Closes the ring step its _piece_i32 calls made on `stream`: the row map is the
 * whole slice's (dev_slice + t*cols holds task row t, every row some piece of
 * the step wrote). One rollback launch undoes, mod 2^32 and in place, every add
 * of this handle past the step's first negative position (its waves leave at
 * once when there is none); then a one-wave kernel closes an open record with
 * that position, the key of the record that holds it, the column and ring_step
 * (IllegalStateException(key, col), IntMatrixStore.java:174-176), and hands the
 * control block's word back clear. The slice then holds every add up to and
 * including the failing one and nothing after it, and may leave the rank. */
int dml_prereduce_chain_close_i32(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                  int64_t ntask_rows, void* dev_slice, void* dev_record, int32_t ring_step,
                                  void* stream);
/* The two-moment piece of an AdaGrad matrix's pre-reduce (begun with its desc):
 * task row t's Σu and Σu·u over the pushes, in push order, written as
 * dev_out + t*2*cols = [cols Σu | cols Σu²] (f32; rows of whole 16-B vectors
 * under 4 KiB). A call whose index found a key outside the matrix or a repeated
 * row writes zeros (_end reports the error). */
int dml_prereduce_moments_piece(dml_prereduce* p, int64_t row_block, int64_t row_stride, int64_t row_off,
                                int64_t ntask_rows, void* dev_out, void* stream);
/* Make `stream` wait (device side) for the pieces enqueued so far, e.g. the
 * communication stream that reduce-scatters the piece just written. */
int dml_prereduce_stream_wait(dml_prereduce* p, void* stream);
/* Measurement: with every > 0, the pieces of one call in `every` carry
 * start/stop events in their dispatch packets and _end adds their elapsed time
 * to a process-wide total (bench.py's roofline of the sharded path; no
 * reference counterpart). 0 turns timing off. */
int dml_prereduce_timing(int32_t every);
int dml_prereduce_kernel_time(double* ms, int64_t* launches, int32_t reset);

/* Speculative pre-reduce (the sharded path's per-call cost). A
 * context holds a ring of three workspaces for one matrix (rows*cols, the
 * whole model) on `device`. _begin_ctx is _begin within the context: full-range
 * pushes whose sampled records say "record r holds row r", or that match a
 * permutation a call three before listed (kept slot-table columns, any
 * position), skip the key index, and the pieces verify every record's key.
 * dml_prereduce_verify waits for the pieces and reads their verdict; if a
 * record was not what the sample said, it re-runs the call exactly (fresh
 * table, full key index, every piece as launched) on the context's stream and
 * sets *rerun. Consume the partial (reduce-scatter) only after verify, behind
 * dml_prereduce_stream_wait; _end then reports the call's errors as before.
 * dml_prectx_stats counts calls as dml_store_stats counts chunks. At most three
 * calls of one context may be outstanding (begun and not yet ended): a fourth
 * _begin_ctx returns DML_E_INVALID_ARG instead of reusing a busy workspace.
 * Pushes: 4-byte aligned (DML_E_INVALID_ARG otherwise, before the context's
 * ring moves), read inside [ptr, ptr + len) only, may be adjacent. */
typedef struct dml_prectx dml_prectx;
int dml_prectx_create(const dml_desc* desc, int64_t first_key, int64_t rows, int32_t cols, int32_t device,
                      dml_prectx** out);
void dml_prectx_destroy(dml_prectx* ctx);
int dml_prectx_stats(dml_prectx* ctx, dml_store_counters* out, int32_t reset);
int dml_prereduce_begin_ctx(dml_prectx* ctx, const void* const* dev_bufs, const int64_t* lens, int32_t n,
                            void* stream, dml_prereduce** out);
int dml_prereduce_verify(dml_prereduce* p, int32_t* rerun);

/* --- per-shard split of device-resident pushes (multi-GPU exchange path) -- */

/* The client-side split of SparseMatrix.push / SparseArray.push
 * (SparseMatrix.java:46-60): the records of each of the n pushes `dev_bufs[b]`
 * (lens[b] bytes, whole records of the desc's wire layout; `cols` for matrices)
 * are partitioned by owner shard under KeyRange(0, total_rows-1).linearSplit(world)
 * (KeyRange.java:68-80), keeping each push's record order, and written to
 * `dev_out` dest-major: [dest 0: push 0's records, push 1's, ...][dest 1: ...].
 * counts[b*world + d] (host, n*world) receives the record count of push b for
 * dest d. Keys outside [0, total_rows) are dropped (the client's p.contains(k)).
 * Kernels run on `stream`; the call returns when dev_out is written.
 * DML_E_CAPACITY when out_cap is smaller than the kept bytes; world <= 64, n <= 64.
 * dev_out == NULL: counts only (nothing is copied).
 * Pushes and dev_out are 4-byte aligned (DML_E_INVALID_ARG otherwise, before any
 * launch); pushes are read inside [ptr, ptr + len) only and may be adjacent; only
 * the kept bytes at the head of dev_out are written, never a byte past out_cap. */
int dml_shard_split(const dml_desc* desc, int32_t cols, int64_t total_rows, int32_t world,
                    const void* const* dev_bufs, const int64_t* lens, int32_t n, void* dev_out,
                    int64_t out_cap, int64_t* counts, void* stream);

/* --- device record codec (the client's writeMap / readMap, in HBM) ------- */

/* The worker's side of the wire format, for tensors that are already in device memory:
 * SparseMatrix.writeMap / SparseArray.writeMap (SparseMatrix.java:96-148,
 * SparseArray.java:63-76) and the readMap that follows every fetch. Store-less, like
 * dml_shard_split: `desc` (and `cols` for matrices; arrays ignore it and use 1) names the
 * layout, the calls run on the current device and launch their kernels on `stream`.
 * `flags`: DML_FLAG_FLOAT_ARRAY_REF_STRIDE as the store was created with; the other
 * DML_FLAG_* bits are accepted and mean nothing here; any other bit is DML_E_INVALID_ARG.
 *
 * Record bytes (dml_record_bytes; either out-pointer may be NULL):
 *   push   matrices (AdaGrad included) [K key LE][cols x V LE]; arrays [K][V], a float
 *          array under DML_FLAG_FLOAT_ARRAY_REF_STRIDE [K][f32][4 zero bytes]
 *   fetch  what dml_store_fetch_device, _fetch_range_device and dml_group_pull write: the
 *          push layout for plain matrices and int / double arrays; AdaGrad
 *          [K][cols x (f32 value, f32 alpha)]; FloatArrayStore [K][f32][4 pad], under
 *          either flag
 *
 * dml_records_pack_device writes n push records at dev_out: record j holds key
 * dev_keys[j], or key_lo + j when dev_keys is NULL (a full-range gradient needs no key
 * list), and row j of dev_values, a row-major contiguous T[n][cols]. A 4-byte key is the
 * low 4 bytes of the int64 (the writer's (int) cast). *out_len = n x push record bytes.
 *
 * dml_records_unpack_device reads n fetch records at dev_records and writes up to three
 * planes, each skipped when its pointer is NULL (all three NULL: DML_E_INVALID_ARG):
 * dev_values_out T[n][cols]; dev_alpha_out float[n][cols], AdaGrad descs only (non-NULL
 * for any other desc: DML_E_INVALID_ARG); dev_keys_out int64[n], a 4-byte key
 * sign-extended as DataDesc.readKey does.
 *
 * Every move is a dword move: no float instruction touches a value, so NaN payloads,
 * -0.0 and denormals pass unchanged. Key arrays are 8-byte aligned; every other device
 * pointer (values, records, output, planes, f64 ones included) is 4-byte aligned and
 * nothing more, the rule of device pushes and fetch outputs. Only
 * [dev_out, dev_out + *out_len) is ever written, and of each plane exactly its
 * n x cols x V bytes (n x 8 for keys), so outputs may lie between other live data.
 * Inputs are read only inside their n records / rows / keys.
 *
 * Ordering: stream == NULL launches and waits; otherwise the kernels are enqueued on
 * `stream` and the call returns. Two consequences: (1) the inputs must be complete in
 * `stream` order (written by earlier work on `stream`, or by work the caller has
 * ordered before it; a dml_store_fetch_device given the same `stream` is); (2) a push
 * call reads its buffers from the store's own streams, not from `stream`, so the
 * caller synchronises `stream` before it hands a packed buffer to
 * dml_store_push_batch_device or a dml_group_push_* call.
 *
 * Errors, all before any launch and with nothing written. DML_E_INVALID_ARG: a null
 * desc or out_len, n < 0, matrix cols <= 0, a null required pointer with n > 0
 * (dev_values, dev_out; dev_records), a misaligned pointer, an unknown flag bit, an
 * output that overlaps an input of the same call or another output. DML_E_BAD_DESC: a
 * desc no store has. DML_E_UNSUPPORTED: a matrix desc with dense_column == 0 (SURVEY
 * defect 3), or a record of 2^31 dwords and more. DML_E_CAPACITY: cap < n x push record
 * bytes. *out_len is n x push record bytes whenever desc, cols, flags and n are valid
 * (so after DML_E_CAPACITY it says what was needed), else 0. n == 0 is DML_OK with
 * *out_len = 0 and nothing launched. */
int dml_record_bytes(const dml_desc* desc, int32_t cols, uint32_t flags, int64_t* push_rec, int64_t* fetch_rec);
int dml_records_pack_device(const dml_desc* desc, int32_t cols, uint32_t flags, const int64_t* dev_keys,
                            int64_t key_lo, int64_t n, const void* dev_values, void* dev_out, int64_t cap,
                            int64_t* out_len, void* stream);
int dml_records_unpack_device(const dml_desc* desc, int32_t cols, uint32_t flags, const void* dev_records,
                              int64_t n, int64_t* dev_keys_out, void* dev_values_out, float* dev_alpha_out,
                              void* stream);
/* Output bytes of one wave instruction's 64 lines and of one block's tile in the codec's
 * kernels (k_rec_pack, k_rec_unpack): the sizes their tests place stream and plane ends at. */
#define DML_CODEC_WAVE_BYTES 1024
#define DML_CODEC_BLOCK_BYTES 4096
/* Codec knob (diagnostic / tests / timing; process-wide, read at every launch; the bytes
 * are the same for every value). DML_CODEC_KNOB_WIDE_INDEX 1: a line's record or row by
 * 64-bit division whatever the length (the path streams of 2^32 dwords and more take;
 * shorter ones divide in 32 bits). DML_CODEC_KNOB_LOADS: 0 = source loads chosen by record
 * length, 1 = every dword gathered singly, 2 = 16-byte loads wherever a line lies inside
 * one row. DML_E_INVALID_ARG for an unknown knob or value. */
#define DML_CODEC_KNOB_WIDE_INDEX 1
#define DML_CODEC_KNOB_LOADS 2
int dml_diag_codec_knob(int32_t knob, int64_t value);

/* --- device gradient coalescer (the worker's KeyList + HashMap, in HBM) --- */

/* The reference worker fetches through a KeyList, a HashSet<Long> (KeyList.java:14-19,59-61),
 * and accumulates its update per key before SparseMatrix.push writes one record per entry
 * (SparseMatrix.java:46-60,96-148). A worker on the device holds occurrences instead: n keys
 * with repeats, and one gradient row per occurrence. dml_coalesce_device turns them into the
 * reference's shape: one row per distinct key. `desc` (and `cols` for matrices; arrays ignore
 * it and use 1) names the row, as for the codec; an AdaGrad desc is f32.
 *
 * Inputs: dev_keys int64[n]; dev_values a row-major contiguous T[n][cols], T from
 * desc->value_type.
 * dev_keys_out[0..m): the distinct keys of the list, ascending as signed 64-bit values;
 *   *out_rows = m. Unique keys in ascending order are the order the codec's pack and the
 *   store's identity push want.
 * dev_inverse_out[j] (int32[n], may be NULL): the u with dev_keys_out[u] == dev_keys[j]; a
 *   worker gathers the rows it pulled for the unique keys back to its occurrences with it.
 * dev_values_out[u][c] = (((+0.0 + v[j1][c]) + v[j2][c]) + ...) over the occurrences
 *   j1 < j2 < ... of key u in LIST ORDER. Each add rounds once as IEEE, no FMA and no
 *   reassociation; int32 adds wrap mod 2^32 and are not checked. Starting from +0.0 makes
 *   the result what a zero-initialised reference store holds after one handlePush of the
 *   occurrences as records in list order (FloatMatrixStore.java:200-222). Consequences: a
 *   lone -0.0 comes out +0.0, and a signalling NaN comes out quiet.
 * Keys-only mode, the KeyList half, run before the pull: dev_values == NULL requires
 *   dev_values_out == NULL; unique keys, the inverse and the count are written.
 *
 * Key arrays are 8-byte aligned; every other pointer is 4-byte aligned and nothing more, the
 * rule of device pushes. Only m x 8, m x cols x V and n x 4 bytes are ever written, so
 * outputs may lie between other live data. Inputs are read only inside their n keys / rows.
 *
 * Count and ordering: the host needs m to size the pack or the pull, so the call makes
 * exactly one host wait, for the count, on a pinned word of the context. With stream != NULL
 * the kernels that write the outputs are then enqueued on `stream` and the call returns;
 * with stream == NULL it waits for everything. Inputs must be complete in `stream` order.
 * One call is in flight per context: the next call (and dml_coalescer_destroy) first waits
 * for this one's event. The workspace (about 28 bytes per occurrence and the sort's own)
 * grows on demand and is reused. A context belongs to the device it was created for and is
 * not thread-safe.
 *
 * Errors. All but DML_E_CAPACITY are found before any HIP call and before `c` is
 * dereferenced, and leave *out_rows as it was. DML_E_INVALID_ARG: null c / desc / out_rows,
 * n < 0, matrix cols <= 0, a null required pointer with n > 0 (dev_keys, dev_keys_out;
 * dev_values_out when dev_values is given), a misaligned pointer, dev_values_out without
 * dev_values, an output (taken as min(n, cap_rows) rows; the inverse as n words) that
 * overlaps an input or another output. DML_E_BAD_DESC: a desc no store has.
 * DML_E_UNSUPPORTED: a matrix desc with dense_column == 0 (SURVEY defect 3), n >= 2^31, a
 * row of 2^31 dwords or more. DML_E_CAPACITY: m > cap_rows; *out_rows = m says what was
 * needed and NOTHING is written to any output (the writing kernels are launched only after
 * the host has seen the count). n == 0: DML_OK, *out_rows = 0, nothing launched. */
typedef struct dml_coalescer dml_coalescer; /* workspace, pinned count word, one event */
int dml_coalescer_create(int32_t device, dml_coalescer** out);
void dml_coalescer_destroy(dml_coalescer* c);
int dml_coalesce_device(dml_coalescer* c, const dml_desc* desc, int32_t cols, const int64_t* dev_keys, int64_t n,
                        const void* dev_values, int64_t* dev_keys_out, void* dev_values_out,
                        int32_t* dev_inverse_out, int64_t cap_rows, int64_t* out_rows, void* stream);
/* The coalescer's tiling, the sizes its tests place edges at: sorted keys per block of
 * k_co_heads; occurrence indices a group of k_co_sum fetches at a time (a group of fewer
 * lanes fetches one per lane); rows whose loads it issues before the first add. */
#define DML_COALESCE_BLOCK_KEYS 1024
#define DML_COALESCE_BATCH 16
#define DML_COALESCE_DEPTH 4
/* Diagnostic / timing: HIP-event times in ms of the last completed dml_coalesce_device on
 * `c` (waits for it): ms3[0] order (pairs and sort), ms3[1] k_co_heads (count, offsets and
 * the writing pass; the host wait between them is not counted), ms3[2] the row sum (0 in
 * keys-only mode). DML_E_INVALID_ARG before the first call that ran to its end. */
int dml_diag_coalesce_times(dml_coalescer* c, float* ms3);

/* --- native multi-GPU shard group (RCCL) -------------------------------- *
 * One process per GPU; rank r owns shard r of KeyRange.linearSplit(world)
 * (KeyRange.java:68-80). Full-range device-resident pushes are pre-reduced in
 * push order, reduce-scattered over xGMI (ncclReduceScatter, sum) and applied
 * by the owner — the path distml_amd/group.py runs over torch.distributed, for
 * hosts without Python (the JNI deployment). The caller distributes the
 * 128-byte unique id from rank 0 (e.g. over the PS control plane). Pushes are
 * asynchronous: buffers stay valid until the next dml_group_flush, and a
 * call's key / repeated-row errors surface at the next call or the flush.
 * fp32 results differ from the sequential order only by summation order
 * (DESIGN.md §6); int32 is exact.
 * Store order: the group applies its calls to its store in call order; a push made
 * straight to the dml_group_store handle bypasses that order, and a read of that
 * handle sees only the calls applied so far — call dml_group_flush before either,
 * or push through dml_group_push_local.
 * Collective order: every rank issues the same collectives in the same order
 * whatever fails locally; a rank whose call fails (a push that is not whole
 * records, a HIP error, a failed re-run) contributes zeros to that call's
 * collective, skips its own apply and returns the error. The group is then in an
 * undefined state for that rank (the reference's PS thread ends on an exception,
 * PSAgent.java:188-191): destroy it. */
typedef struct dml_group dml_group;
int dml_group_unique_id(uint8_t* out, int32_t cap);
int dml_group_create(const uint8_t* unique_id, int32_t world, int32_t rank, int32_t device, const dml_desc* desc,
                     int64_t total_rows, int32_t cols, int32_t pieces, dml_group** out);
/* The rank's shard store (fetch / checkpoint / read), owned by the group. */
int dml_group_store(dml_group* g, dml_store** store);
/* dml_prectx_stats of the group's speculative pre-reduce (zeros before the first
 * full-range call). */
int dml_group_prereduce_stats(dml_group* g, dml_store_counters* out, int32_t reset);
int dml_group_push_full_range(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* The exact path (AdaGrad, int32-checked, arrays, key-subset pushes): each of the
 * rank's n device-resident pushes is split by owner shard (dml_shard_split), the
 * slices go to their owners in one grouped ncclSend/ncclRecv exchange, and every
 * owner applies the slices it received in rank-major push order (rank 0's n
 * pushes, then rank 1's, ...) through the store's ordered push — the reference's
 * client-split + server-apply data flow, bit-exact with errors included. Every
 * rank calls with the same n (<= 64). The owner's pushes are asynchronous: their
 * errors surface at the next exchange call or at dml_group_flush. */
int dml_group_push_exchange(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* AdaGrad's sharded path for many pushes per rank: the rank's n
 * full-range pushes pre-reduced into Σu and Σu² (dml_prereduce_moments_piece),
 * one ncclReduceScatter of both, the owner's
 * dml_store_apply_adagrad_moments_device. xGMI bytes per rank: (world-1)/world
 * x 2 x the model, whatever n is (the exchange path moves n pushes). Within
 * 1e-6, not bit-exact; errors surface at the next call or the flush. Known
 * divergences: a maxDelta tie goes to the first element in row-major order (the
 * reference's: the first in push / record order, FloatMatrixStoreAdaGrad.java:273-277);
 * with NaN / Inf gradients alpha keeps its value; and alpha is
 * rewritten as f(delta) at every element whose delta ends above 1, not only on
 * rows a push of the call lists: after dml_store_set_alpha, a row with delta
 * above 1 that no push lists keeps the new initialAlpha in the reference
 * (:268-272) and gets f(delta) here; such a row's -0.0 data becomes +0.0. The
 * reduce-scattered message has no per-row touched mark to tell the rows apart.
 * dml_group_push_exchange and dml_group_push_chained are the paths without
 * these divergences. */
int dml_group_push_moments(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* Pushes the client already split to this shard (SparseMatrix.java:46-60): the
 * store's exact ordered device push (dml_store_push_batch_device), queued after
 * every earlier group call's apply; no collective. */
int dml_group_push_local(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* Order-exact chained reduce-scatter of the rank's n (0 <= n <= 64; ranks may
 * differ) full-range pushes, for fp32 / fp64 matrices, plain or AdaGrad (below).
 * Owner s's slice
 * starts as shard s and walks the ring s, s+1, ..., s-1: every rank adds its own
 * pushes' rows of the slice in push order, one IEEE rounding per add
 * (dml_prereduce_chain_piece), and forwards it with ncclSend / ncclRecv; the last
 * hop brings it home and the owner commits it (dml_store_assign_dense_device).
 * After the call, shard s holds, byte for byte, what one reference store over
 * shard s's key range holds after handlePush (FloatMatrixStore.java:200-222,
 * DoubleMatrixStore.java:153-190) of rank s's pushes in push order, then rank
 * s+1's, ..., then rank s-1's, each restricted to the records whose key lies in
 * the shard — an arrival order the reference's server may see (it applies pushes
 * as they arrive, PSAgent.java:166-186). A row a push does not list gets no add
 * from it (not even of +0.0). Per rank the call moves one model's bytes over
 * xGMI whatever n is (N-1 of its N slices are other shards'), in `pieces`
 * sub-chunks per slice, each sent while the next one is summed.
 * Order: the group's calls (push_local, push_full_range, push_exchange,
 * push_chained) apply to the store in call order, no flush needed between them.
 * Pushes as for the other device pushes: 4-byte aligned, read inside
 * [ptr, ptr + len) only, valid until dml_group_flush.
 * Failures: argument errors (null or misaligned pointer, n out of range) are
 * refused before the group's state moves and before the rank joins the ring.
 * A local failure never changes the sequence of sends and receives: the rank
 * forwards every slice unchanged in all N steps, its pushes appear in no shard,
 * and the other ranks' contributions still reach every shard, its own
 * included. A push that is not whole records, or a HIP error before the
 * pieces, is returned by this call; a key outside the matrix or a row listed
 * twice in one push (found by the key index on the device) is returned by the
 * rank's next group call or by dml_group_flush.
 * AdaGrad groups (FloatMatrixStoreAdaGrad): the slice carries data, delta, one
 * touched mark per row and the maxDelta record, each sub-chunk one message
 * (dml_prereduce_chain_piece_ada); about two planes' bytes per rank over xGMI.
 * After the call shard s holds the state of one FloatMatrixStoreAdaGrad over its
 * key range fed the same ring order (FloatMatrixStoreAdaGrad.java:239-284): data
 * and delta bit for bit; alpha bit for bit, computed once at the owner's commit
 * (dml_store_assign_adagrad_device) with the owner's parameters, on rows some
 * rank's accepted push listed in this call; maxDelta value, row and col, ties
 * included (the first in ring rank, push, record, column order holds it). A
 * failed rank marks no row and changes no maxDelta record. One documented
 * divergence, and no other: an element whose delta comes home NaN (a NaN
 * gradient reached it in this call) keeps the alpha the owner's store held
 * before the call, where the reference leaves the alpha of its last non-NaN
 * delta above 1; its data and delta are exact. dml_group_push_exchange is the
 * path without this divergence.
 * At world 1 the call is dml_store_push_batch_device. int32 descriptors:
 * DML_E_UNSUPPORTED (use dml_group_push_exchange), on every rank alike and
 * before any send. */
int dml_group_push_chained(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* The chained reduce-scatter for dense int32 matrices (IntMatrixStore): same
 * arguments, ring, buffers, call order and failed-rank rule as
 * dml_group_push_chained. After the call shard s equals one IntMatrixStore over
 * shard s's keys fed rank s's pushes, then rank s+1's, ..., then rank s-1's,
 * each in push order (IntMatrixStore.java:154-178): every add wraps mod 2^32 and
 * is checked; at the first counter left negative the shard holds every add up
 * to and including that one and nothing after it, and it is closed: it takes no
 * add from any rank in this call or any later one (PSAgent.java:188-191). The
 * other shards go on. Each slice carries a verdict record
 * (DML_CHAIN_I32_RECORD_BYTES) at the head of its first sub-chunk's message, so
 * S + N * 32 bytes per rank cross xGMI. No sub-chunk of a slice leaves a rank
 * before the rank's whole step over the slice has its verdict
 * (dml_prereduce_chain_close_i32), so piece time does not hide under the step's
 * own transfers as it does for floats.
 * Who reports: only the owner of a closed shard, through its next group call or
 * dml_group_flush: DML_E_NEGATIVE_COUNTER, key and col from
 * dml_store_error_state; a non-chained call (push_local, push_exchange,
 * push_full_range) right behind the closing call waits for the commit's record
 * and is refused as the reference refuses it; the next chained call does not
 * wait (the store's device-resident record already keeps the shard closed) and
 * reports once the host has seen the record. The owner's pushes still reach the
 * other shards. The other ranks return DML_OK.
 * At world 1 the call is dml_store_push_batch_device. Any group that is not a
 * dense int32 matrix: DML_E_UNSUPPORTED, on every rank alike and before any
 * send. */
int dml_group_push_chained_i32(dml_group* g, const void* const* dev_bufs, const int64_t* lens, int32_t n);
/* Collective pull: WorkerAgent.fetch (WorkerAgent.java:74-122) for workers whose key lists
 * and buffers are in HBM. Every rank calls it at the same position in its sequence of group
 * calls, each with its own int64 key list in device memory (8-byte aligned; nkeys may differ
 * per rank and may be 0), and receives the dense-column handleFetch records of its keys from
 * the shards that own them, byte for byte what dml_store_fetch_device writes on the owner
 * (every store kind: the K-byte key, AdaGrad's [value][alpha] pairs, FloatArrayStore's padded
 * slot).
 *
 * Split: keys are partitioned by owner under KeyRange.linearSplit(world) of [0, total_rows)
 * (KeyRange.java:68-80), stably: within one owner the list's order is kept, as
 * partitions[i].intersect(rowKeys) keeps it (KeyList.java:74-86). A key outside
 * [0, total_rows) is dropped (tested as a 64-bit value, no narrowing: the client's
 * intersect, and dml_shard_split); a key listed twice gets two records.
 *
 * Output, flags == 0 (owner-major): owner 0's records, then owner 1's, ..., each in list
 * order: the reference's byte[][] concatenated. out_counts[q] (world entries, may be NULL) =
 * records from owner q; *out_len = total bytes. DML_PULL_REQUEST_ORDER: record j is the
 * record of the j-th kept key of the list (no key dropped: record i belongs to keys[i]);
 * out_counts as before. dev_out is 4-byte aligned and nothing more, and only
 * [dev_out, dev_out + *out_len) is ever written.
 *
 * Visibility: a pull sees every group push call that any rank issued before it, and none
 * issued after it, with no flush in between: each rank first drains what dml_group_flush
 * drains (pending full-range, moments and chained handles, the int32 chain's verdict; the
 * previous dml_group_push_exchange's held slices are handed over after this call's first
 * stream wait, as dml_group_push_exchange does), then encodes on its store's apply stream.
 *
 * `stream` as in dml_store_fetch_device: NULL makes the call synchronous; otherwise
 * `stream` waits on one event behind the call's last kernel or transfer, and dev_out stays
 * valid until then. dev_keys must be complete when the call is made (the partition reads
 * them at once, and the host waits for its counts and for the count exchange; the owner
 * encode enters the store like every read, so the host may also wait there for earlier
 * pushes' index and verdict, as in dml_store_fetch_device). One pull is
 * in flight per group: the next pull first waits for this one's event.
 *
 * Local failures never strand a peer: a rank with a bad argument (DML_E_INVALID_ARG: a null
 * out_len, nkeys < 0, a null or misaligned dev_keys, a misaligned dev_out, an unknown flag)
 * or whose cap is below the kept records' bytes (DML_E_CAPACITY; *out_len and out_counts say
 * what was needed) asks for nothing, writes nothing, still serves its shard and takes part
 * in every exchange, and returns its error afterwards. A rank whose drain returns a deferred
 * store error, or whose shard is in its sticky error state, serves its shard's bytes as they
 * stand; the deferred error is returned at the end (a sticky state alone is DML_OK).
 * That guarantee covers argument, capacity and deferred store errors. A HIP, RCCL or
 * allocation failure in the middle of the call (DML_E_HIP) returns at once, as in
 * dml_group_push_exchange: its peers may then wait for it.
 * At world 1 there is no exchange: the records are encoded straight into dev_out.
 * A group of more than DML_PULL_MAX_WORLD ranks: DML_E_UNSUPPORTED, on every rank alike,
 * before any send, with nothing written (out_len and out_counts included). */
#define DML_PULL_REQUEST_ORDER 0x1
#define DML_PULL_MAX_WORLD 64
int dml_group_pull(dml_group* g, const int64_t* dev_keys, int64_t nkeys, void* dev_out, int64_t cap, int32_t flags,
                   int64_t* out_len, int64_t* out_counts, void* stream);
/* Output bytes of one wave instruction's 64 lines and of one block's tile in the request-order
 * permutation kernel (k_pull_unsplit): the sizes its tests place stream ends at. */
#define DML_PULL_WAVE_BYTES 1024
#define DML_PULL_BLOCK_BYTES 4096
int dml_group_flush(dml_group* g);
void dml_group_destroy(dml_group* g);
/* Fault injection for tests: the nth full-range call finished from now on (1 = the
 * next) fails its verdict as a local HIP error would (0 = off). */
int dml_group_debug_fail_verify(dml_group* g, int32_t nth);

/* --- synthetic workload generators (bench/test support) ----------------- *
 * Counter-based (SplitMix64) so the CPU oracle regenerates the same bytes.
 * Spec in DESIGN.md §Synthetic data. Run on `stream` (void* hipStream_t). */
int dml_synth_dense_bucket(void* dev_out, const dml_desc* desc, int64_t first_key,
                           int64_t shard_rows, int64_t nrec, int32_t cols, uint64_t seed,
                           uint64_t perm_a, uint64_t perm_c, void* stream);
int dml_synth_sparse_bucket(void* dev_out, const dml_desc* desc, int64_t first_key,
                            int64_t key_space, int64_t nrec, uint64_t seed,
                            uint64_t perm_a, uint64_t perm_c, void* stream);
int dml_synth_fill_store(dml_store* s, uint64_t seed);

/* Diagnostic: stream `bytes` (multiple of 16, 16-B aligned) from dev_src with
 * 16-B non-temporal loads, copying them to dev_dst (copy != 0) or only reading
 * them (copy == 0; dev_dst receives at most one word); timed by HIP events on
 * `stream`, *ms = kernel time. bench.py reports the reduce's fraction of these
 * measured HBM ceilings. */
int dml_diag_stream(int32_t copy, void* dev_dst, const void* dev_src, int64_t bytes, void* stream, float* ms);
/* Random-RMW floor (diagnostic): dev_array[dev_index[i]] += dev_values[i] for i < n,
 * one plain 4-B read-modify-write per update, in the given (sorted) order, timed on
 * `stream`, *ms = kernel time. Every index must lie inside dev_array; repeated
 * indices race, so the array's values are not meaningful afterwards (scratch only).
 * bench.py's config-3 leg times the leaf apply against it: the same updates sorted
 * globally, with no partition, are the best case of the random scatter-add. */
int dml_diag_rmw_floor(float* dev_array, const uint32_t* dev_index, const float* dev_values, int64_t n, void* stream,
                       float* ms);

/* Dense stream floor (diagnostic, config 4 and its AdaGrad variant): the store's f32
 * shard (cols a multiple of 4) plus n full-range pushes whose records are rows in order
 * (lens[b] = rows x record stride; record r is taken to be row r, keys not read), each
 * element summed in push order and written once: into the speculative second buffer
 * where the store has one (as k_flat_ident writes, *out_of_place = 1; the committed
 * shard is left alone), else in place; AdaGrad stores also delta += u·u in place (alpha
 * and maxDelta untouched). The plain stream of the reduce's bytes over the same
 * allocations, timed on `stream`, *ms = kernel time: bench.py's config-4 legs report
 * their kernels against it. */
int dml_diag_dense_floor(dml_store* s, const void* const* dev_bufs, const int64_t* lens, int32_t n, void* stream,
                         float* ms, int32_t* out_of_place);

/* Row-gather floor (diagnostic, config 5): for each of the ntouched rows dev_rows[i] of
 * an int32 shard (row-major, `cols` a multiple of 4, at most 1024), read the row once,
 * add the records dev_addr[dev_ptr[i] .. dev_ptr[i+1]) (device addresses of each
 * record's first value, in push order) and write the row once: the IntMatrixStore
 * reduce's bytes with no key index, slot table or negativity check. Timed on `stream`,
 * *ms = kernel time. bench.py's config-5 leg reports the reduce against it. */
int dml_diag_gather_floor(int32_t* dev_shard, int32_t cols, const int32_t* dev_rows, const int32_t* dev_ptr,
                          const uint64_t* dev_addr, int64_t ntouched, void* stream, float* ms);

/* Ring reduce-scatter footprint (diagnostic, bench.py --emulate-rs N): the local HBM
 * traffic one rank's ring reduce-scatter of a world x chunk_bytes partial makes —
 * world - 1 steps, each reading one chunk of the partial and the chunk that arrived
 * (dev_landing, 2 x chunk_bytes) and landing their sum in a buffer (the write a peer
 * makes into this rank's), then the last sum into dev_recv — on a grid of `channels`
 * blocks (RCCL's one block per channel), enqueued on `stream`. Values are not a
 * reduce-scatter's (no peer contributes): timing only. */
int dml_diag_ring_rs(int32_t value_type, const void* dev_partial, void* dev_recv, void* dev_landing,
                     int64_t chunk_bytes, int32_t world, int32_t rank, int32_t channels, void* stream);

/* The two kernels of dml_group_pull on the caller's buffers, one GPU, no group (diagnostic,
 * tests and timing). The partition: nkeys int64 keys (8-byte aligned) split by owner under
 * linearSplit(world) of [0, total_rows), world <= 64: dev_part_keys (nkeys entries) receives
 * the kept keys as [owner][list order]; dev_slot / dev_kept (nkeys entries each, may be NULL)
 * every list index's owner-major slot and kept index (the list index minus the dropped keys
 * before it), -1 for a dropped key; counts (host, world + 1 entries) the per-owner counts and
 * the dropped count. The permutation (k_pull_unsplit; skipped when dev_src or dev_dst is
 * NULL): dev_src holds one record of rec_bytes (whole dwords, >= 8) per kept key in
 * owner-major order, dev_dst receives them in list order; both 4-byte aligned, only
 * [dev_dst, dev_dst + kept x rec_bytes) is written. variant: 0 = the shipped load choice,
 * 1 = every dword gathered singly, 2 = 16-byte loads. Synchronous; *ms_partition /
 * *ms_unsplit (may be NULL) = kernel times by HIP events on `stream`. */
int dml_diag_pull_kernels(const int64_t* dev_keys, int64_t nkeys, int64_t total_rows, int32_t world,
                          int64_t* dev_part_keys, int64_t* dev_slot, int64_t* dev_kept, int64_t* counts,
                          const void* dev_src, void* dev_dst, int64_t rec_bytes, int32_t variant, void* stream,
                          float* ms_partition, float* ms_unsplit);

/* Store tuning knob (diagnostic / tests): DML_KNOB_IDENT_FULL_MIN_BYTES = the slot-table
 * size (bytes) from which an AdaGrad chunk of full-range pushes checks every record's key
 * up front (k_ident_full) instead of running the key index, so that all-identity chunks
 * run k_ada_ident (default 64 MiB: where the index's slot-table atomics leave the caches).
 * Lowering it lets tests drive that path at small sizes; results are the same either way.
 * Returns DML_E_INVALID_ARG for an unknown knob or a negative value. */
#define DML_KNOB_IDENT_FULL_MIN_BYTES 1
/* DML_KNOB_INDEX_CUS = k | pattern << 16: the store's index stream (the next chunk's key
 * index or sparse partition) on k CUs and its apply stream on the others, k = 0 (the
 * default) both on every CU; pattern 0 spreads the k CUs evenly over the CU numbering,
 * 1 takes the first k (config 3: the partition beside the leaf). */
#define DML_KNOB_INDEX_CUS 2
/* DML_KNOB_FETCH_KERNEL: the encode kernel of dml_store_fetch_device / _fetch_range_device.
 * 0 (the default) = the library's dispatch; 1 = always k_fetch (the host fetch's kernel, one
 * thread per key and column); 2 = always k_fetch_vec (whole 16-byte stores), where the
 * fetch returns DML_E_UNSUPPORTED if that kernel cannot take the store's shape (today it
 * takes every dense-column shape). With 2, bits 8-12 pick one of the launch shapes
 * DESIGN.md §4.10 compares (bits 8-9: 0 = shard loads chosen by record length, 1 = every
 * dword gathered singly, 2 = 16-byte loads; 1024: blocks renumbered XCD-contiguous;
 * 2048 / 4096: one / four vectors per thread); the bytes are the same for every value. */
#define DML_KNOB_FETCH_KERNEL 3
int dml_diag_store_knob(dml_store* s, int32_t knob, int64_t value);

/* The partition plan an array store makes for one chunk before any kernel runs (diagnostic /
 * tests; host arithmetic only, no device call, works without a GPU): value_type is the store's
 * DML_ELEMENT_TYPE_*, rows its shard's size, nrecs[0..n) the records of each of the chunk's
 * pushes (1 <= n <= 64), tail_cut != 0 when some push of the chunk ends inside a record. The
 * fields are SpPlan's: leaves of 2^SL rows, 2^D2 leaves per level-1 bin, cap1 /
 * cap2 records per bin / leaf of the single-pass layout, compact = 8-byte fp32 words, big = the
 * one-level partition with nbig big leaves of 2^BL rows and capS records per (big leaf, slice);
 * BL, nbig and capS are 0 unless big. bshift: the launched leaf kernel's line bucket is
 * (row - leaf's first row) >> bshift. Returns DML_E_INVALID_ARG for a bad argument. */
typedef struct dml_sparse_plan_info {
    int64_t nrec, nleaves, nbig, cap1, cap2, capS;
    int32_t SL, D2, nbins1, compact, big, BL, bshift, reserved;
} dml_sparse_plan_info;
int dml_diag_sparse_plan(int32_t value_type, int64_t rows, const int64_t* nrecs, int32_t n, int32_t tail_cut,
                         dml_sparse_plan_info* out);

/* --- misc --------------------------------------------------------------- */
const char* dml_last_error(void);   /* thread-local message for the last failure */
const char* dml_version(void);

#ifdef __cplusplus
}
#endif

#endif /* DISTML_PS_H */
