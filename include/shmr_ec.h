/*
 * shmr_ec.h -- C ABI of the MI355X-native Reed-Solomon erasure path for
 * shmr's StorageBlock (VirtualBlock) layer.
 *
 * Drop-in boundary: the reference binds reed_solomon_erasure::galois_8::
 * ReedSolomon (reference src/vfs/block.rs:10) and calls exactly three
 * entry points on the hot path:
 *
 *   ReedSolomon::new(data, parity)        src/vfs/block.rs:405, :531  -> shmr_ec_new
 *   r.encode(&mut Vec<Vec<u8>>)           src/vfs/block.rs:427        -> shmr_ec_encode
 *   r.reconstruct(&mut Vec<Option<..>>)   src/vfs/block.rs:560        -> shmr_ec_reconstruct
 *
 * plus the shard-size helper the callers use before every encode/decode
 * (calculate_shard_size, src/vfs/mod.rs:16-18) -> shmr_ec_shard_size.
 *
 * Everything runs on AMD Instinct MI355X (gfx950) through hand-written HIP
 * kernels.  There is no CPU compute fallback: without a usable GPU every
 * compute entry point returns SHMR_EC_NO_DEVICE / SHMR_EC_DEVICE_ERROR.
 *
 * Conventions: plain pointers and sizes, 0 on success, negative status on
 * failure, never aborts (an internal allocation failure returns
 * SHMR_EC_OUT_OF_MEMORY), never frees caller memory.  Thread-safe: contexts
 * may be shared across threads or created per call (the reference creates a
 * ReedSolomon per block from rayon workers, src/vfs/mod.rs:93-96).  Every
 * entry point runs under HIP's relaxed stream-capture mode (the calling
 * thread's mode is restored on return), so calls from other threads neither
 * fail nor break a graph capture in progress on some thread.
 */
#ifndef SHMR_EC_H
#define SHMR_EC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes.  -1..-13 are 1:1 with reed_solomon_erasure::Error (6.0.0),
 * which the reference wraps as ShmrError::EcError (src/config.rs:158,170-174). */
typedef enum shmr_ec_status {
    SHMR_EC_OK = 0,
    SHMR_EC_TOO_FEW_SHARDS = -1,
    SHMR_EC_TOO_MANY_SHARDS = -2,
    SHMR_EC_TOO_FEW_DATA_SHARDS = -3,
    SHMR_EC_TOO_MANY_DATA_SHARDS = -4,
    SHMR_EC_TOO_FEW_PARITY_SHARDS = -5,
    SHMR_EC_TOO_MANY_PARITY_SHARDS = -6,
    SHMR_EC_TOO_FEW_BUFFER_SHARDS = -7,
    SHMR_EC_TOO_MANY_BUFFER_SHARDS = -8,
    SHMR_EC_INCORRECT_SHARD_SIZE = -9,
    SHMR_EC_TOO_FEW_SHARDS_PRESENT = -10,
    SHMR_EC_EMPTY_SHARD = -11,
    SHMR_EC_INVALID_SHARD_FLAGS = -12,
    SHMR_EC_INVALID_INDEX = -13,
    /* library-level conditions (no crate equivalent) */
    SHMR_EC_INVALID_ARGUMENT = -100,
    SHMR_EC_NO_DEVICE = -101,
    SHMR_EC_DEVICE_ERROR = -102,
    SHMR_EC_OUT_OF_MEMORY = -103
} shmr_ec_status;

typedef struct shmr_ec shmr_ec_t;

/* Human-readable name of a status ("TooFewShardsPresent", ...). */
const char* shmr_ec_status_name(int status);

/* Library version string (names the flavour: "product" or "tools"). */
const char* shmr_ec_version(void);

/* Kernel build ID: hash of the kernel sources, device compile flags and
 * compiler version (12 hex digits).  Measurement records (PMC traffic) are
 * keyed by it, so they can be matched to the code that produced them. */
const char* shmr_ec_build_id(void);

/* 1 in the tools build (libshmr_ec_tools.so: measurement variants and kernel
 * knobs for tools/), 0 in the product library. */
int shmr_ec_is_tools_build(void);

/* ---- host logic (no GPU needed) ---------------------------------------- */

/* calculate_shard_size, src/vfs/mod.rs:16-18:
 * (length as f32 / data_shards as f32).ceil() as usize. 0 if data_shards==0. */
size_t shmr_ec_shard_size(uint64_t length, uint32_t data_shards);

/* ReedSolomon::new (src/vfs/block.rs:405,531).  Errors exactly as the crate:
 * data==0 -> TOO_FEW_DATA_SHARDS, parity==0 -> TOO_FEW_PARITY_SHARDS,
 * data+parity > 256 -> TOO_MANY_SHARDS.  Builds the (data+parity) x data
 * systematic Vandermonde matrix on the host; touches no GPU. */
int shmr_ec_new(uint32_t data_shards, uint32_t parity_shards, shmr_ec_t** out);
void shmr_ec_free(shmr_ec_t* rs);

uint32_t shmr_ec_data_shard_count(const shmr_ec_t* rs);
uint32_t shmr_ec_parity_shard_count(const shmr_ec_t* rs);
uint32_t shmr_ec_total_shard_count(const shmr_ec_t* rs);

/* Copies the (data+parity) x data coding matrix, row-major, into out
 * (out_len >= total*data). */
int shmr_ec_matrix(const shmr_ec_t* rs, uint8_t* out, size_t out_len);

/* Rows of the reconstruct plan the library would run for a presence
 * pattern: out_rows[m * data + t] (m < *n_out) applied to the shards listed in
 * in_idx[0..data) rebuilds shard out_idx[m].  Host only; for tests/tools. */
int shmr_ec_reconstruct_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards, int data_only,
                             uint16_t* in_idx, uint16_t* out_idx, uint8_t* out_rows,
                             size_t out_rows_len, uint32_t* n_out);

/* ---- host-buffer entry points (drop-in for the crate calls) ------------- */

/* ReedSolomon::encode (src/vfs/block.rs:427).  shards[0..data) are inputs,
 * shards[data..total) are overwritten with parity.  shard_lens[i] is the
 * length of shards[i]; the crate's checks run first and in its order
 * (count -> TOO_FEW/TOO_MANY_SHARDS, len 0 -> EMPTY_SHARD, unequal ->
 * INCORRECT_SHARD_SIZE).  Runs on the context's device: in place across
 * PCIe if the shards are mapped host memory (shmr_ec_host_alloc /
 * shmr_ec_host_register, zero-copy), else through a pooled mapped bounce
 * buffer (blocks up to "bounce_kib") or per-shard DMA staging. */
int shmr_ec_encode(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards);

/* ReedSolomon::reconstruct / reconstruct_data (src/vfs/block.rs:560).
 * present[i] != 0 marks shard i as Some(..); shard_lens[i] is only read for
 * present shards.  Absent shards must point at caller buffers of the common
 * shard length (the crate allocates them; the Rust shim allocates
 * vec![0; len] before calling).  data_only != 0: absent parity shards are left
 * untouched (and may be NULL).  All present -> no-op; fewer than data present
 * -> TOO_FEW_SHARDS_PRESENT. */
int shmr_ec_reconstruct(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                        const uint8_t* present, size_t nshards, int data_only);

/* ReedSolomon::verify.  The crate's checks, in its order, as shmr_ec_encode
 * (count, EMPTY_SHARD, INCORRECT_SHARD_SIZE), before any device work.
 * *consistent = 1 if shards[data..total) equal the parity of shards[0..data),
 * else 0.  No shard is written.  The block is gathered into device scratch
 * (grown without a free on the call path) and checked there by the kernel of
 * shmr_ec_verify_batch_dev; blocking. */
int shmr_ec_verify(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                   size_t nshards, int* consistent);

/* Asynchronous forms of shmr_ec_encode / shmr_ec_reconstruct (same arguments,
 * validation and errors, returned by the start call), so a Block Cache can
 * overlap its file I/O or copies with the GPU: when every shard the call
 * touches lies in mapped memory, the kernels are enqueued and the start call
 * returns with *op pending; on every other path the work is complete when it
 * returns.  While *op is pending the caller may read -- not write -- the input
 * shards (encode: shards [0, data); reconstruct: the present ones) and must not
 * touch the output shards.  shmr_ec_op_wait(op) waits for the work, frees op
 * and returns SHMR_EC_OK or a device error; on a start error *op is NULL. */
typedef struct shmr_ec_op shmr_ec_op_t;
int shmr_ec_encode_start(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards,
                         shmr_ec_op_t** op);
int shmr_ec_reconstruct_start(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                              const uint8_t* present, size_t nshards, int data_only, shmr_ec_op_t** op);
int shmr_ec_op_wait(shmr_ec_op_t* op);

/* ---- one block per call on device buffers: the submission queue ----------- *
 * The crate's encode / reconstruct of ONE block (ReedSolomon::encode at
 * src/vfs/block.rs:427, reconstruct at :560) whose shards are device buffers
 * on `device`: the same arguments, checks and errors as shmr_ec_encode /
 * shmr_ec_reconstruct, with d_shards[i] device pointers.  The inputs must be
 * complete when the call is made (written by synchronous copies, or by work
 * the caller has waited for): these calls take no stream.
 *
 * The reference makes one such call per block from rayon workers
 * (src/vfs/mod.rs:91-97).  One launch per block leaves the GPU launch-bound,
 * so per device ID the library keeps a submission queue: a call's block is
 * launched at once when fewer than "coalesce_depth" (default 1) batches are in
 * flight on the queue's stream, and otherwise merges with every call that
 * arrives meanwhile (from any thread, any codec; knob "coalesce_us": an idle
 * queue waits that long for company) into the next launch, which the queue's
 * watcher thread issues "coalesce_lead_us" (default 30; 0: at completion)
 * before the running batch's estimated end, so it is queued behind it -- one pointer-
 * table call per (codec, operation, length, data_only) group, whose shards,
 * if they sit on a slot lattice (a slab, a shmr_ec_pool), run the strided
 * kernels over their slots.  The call returns when its own block is written,
 * with its own status (a group's device error is its members' status).
 * Completion is a word in pinned host memory that a one-wave kernel behind
 * every batch advances: a waiting caller spins on it for "coalesce_spin_us"
 * (default 30) and then sleeps until the queue's watcher thread (which
 * follows the oldest batch, asleep on its event after "coalesce_watch_us",
 * default 200) wakes it; a call waited for while still held back launches
 * everything pending at once.  "coalesce_target" (default 64): that many pending
 * calls launch even with "coalesce_depth" batches in flight.  The *_start forms return with the
 * block queued (*op); shmr_ec_op_wait completes it.  While pending, inputs
 * may be read, outputs must not be touched. */
int shmr_ec_encode_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, size_t nshards,
                       int device);
int shmr_ec_reconstruct_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, const uint8_t* present,
                            size_t nshards, int data_only, int device);
int shmr_ec_encode_dev_start(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, size_t nshards,
                             int device, shmr_ec_op_t** op);
int shmr_ec_reconstruct_dev_start(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens,
                                  const uint8_t* present, size_t nshards, int data_only, int device,
                                  shmr_ec_op_t** op);

/* Submission-queue counters of a device ID since load: out[i] for i < n in
 * the order below. */
enum {
    SHMR_EC_Q_REQUESTS = 0,   /* blocks submitted (device calls, and mapped host calls under "coalesce") */
    SHMR_EC_Q_BATCHES = 1,    /* launch groups taken from the queue */
    SHMR_EC_Q_MAX_BATCH = 2,  /* the most blocks one launch group merged */
    SHMR_EC_Q_SLEEPS = 3,     /* waits that ended in a blocking event synchronize */
    SHMR_EC_Q_EARLY = 4,      /* batches launched behind a running one before its end (knob coalesce_lead_us) */
    SHMR_EC_Q_COUNTERS = 5
};
int shmr_ec_queue_stats(int device, uint64_t* out, size_t n);

/* ---- device-resident batched entry points ------------------------------ *
 * All pointers are device pointers on `device`; `stream` is a hipStream_t
 * (NULL = the null stream).  Block b's shard i lives at
 *     base + b * block_pitch + i * shard_pitch,
 * at any byte alignment (the reference's packed block buffer, shard i at
 * i * S, included).
 *
 * Stream-ordered: after the device's one-time initialisation (the first call
 * that touches the device, or shmr_ec_device_init) these calls make no
 * blocking HIP call -- they enqueue kernels (and, for an erasure pattern not
 * seen before on the device, one hipMemcpyAsync of its coefficient plan from
 * a permanent pinned slot) on `stream` and return.  They can be captured into
 * a HIP graph (e.g. torch.cuda.graph) once the device is initialised; a
 * capture that would need the initialisation returns INVALID_ARGUMENT with
 * nothing enqueued, and so does one whose stream state cannot be read (the
 * legacy null stream while another thread captures in global mode).
 * SHMR_EC_DEV_BLOCKING_CALLS counts the exceptions.
 *
 * Cross-stream coupling: the readiness of an upload (a plan image, an upload-
 * ring slot, a table-cache entry) that a call enqueued on a caller stream is
 * tracked by an event mirrored onto the device's one private stream, which
 * waits for the caller stream's events in the order they were recorded.  A
 * later call on ANOTHER stream that needs such an upload (or a busy ring
 * slot) may therefore wait for work queued earlier on unrelated caller
 * streams.  A stream held back by something outside the library (a host
 * function, a stream wait on a value, a collective) can delay, and with a
 * full ring block, another thread's call until it progresses.  Streams that
 * only reuse plans and tables already uploaded are not affected. */

/* One-time per-device initialisation (probe of the memory system's unaligned
 * access mode on a private stream, the plan arena and a 4 MiB capture reserve
 * in pinned and device memory).  Optional: the first device call does it
 * implicitly.  Blocking. */
int shmr_ec_device_init(int device);

/* Captured calls keep their tables in the device's capture reserve, which a
 * capture never grows: a captured *_ptrs_dev call needs nblocks * total * 8
 * bytes, a captured reconstruct of several erasure patterns in more than 32
 * block runs about 6 bytes per block plus 8 per pattern (each rounded up to
 * 256 bytes).  A captured call that does not fit returns OUT_OF_MEMORY with
 * nothing enqueued.  This makes sure one free range of `bytes` exists
 * (initialising the device if needed; blocking, not inside a capture).  A
 * captured call's block returns to the reserve when its graph and every
 * executable graph instantiated from it have been destroyed. */
int shmr_ec_capture_reserve(int device, size_t bytes);

/* Encode nblocks blocks: data shard i of block b at
 * d_data + b*data_block_pitch + i*data_shard_pitch; parity shard r at
 * d_parity + b*parity_block_pitch + r*parity_shard_pitch. */
int shmr_ec_encode_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch,
                             size_t data_block_pitch, uint8_t* d_parity, size_t parity_shard_pitch,
                             size_t parity_block_pitch, size_t nblocks, size_t shard_len,
                             int device, void* stream);

/* ReedSolomon::verify of nblocks blocks: a device-resident batch, addressed
 * exactly as shmr_ec_encode_batch_dev.
 * d_mismatch: nblocks uint32 words of DEVICE memory on `device` (4-byte
 * aligned), overwritten: 0 = block b is a codeword; else bit min(r, 31) is set
 * for every parity row r whose stored bytes differ from the recomputed ones
 * in [0, shard_len).  Nothing else is written: the kernels read the data and
 * the stored parity once ((data + parity) * shard_len bytes per block) and
 * store only to the word of a block that differs.  Stream-ordered, capturable
 * (the zeroing of d_mismatch is part of the enqueued work). */
int shmr_ec_verify_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch,
                             size_t data_block_pitch, const uint8_t* d_parity,
                             size_t parity_shard_pitch, size_t parity_block_pitch,
                             size_t nblocks, size_t shard_len, uint32_t* d_mismatch,
                             int device, void* stream);

/* ---- scrub: locate and repair one damaged shard per block ------------------ *
 * A block that fails shmr_ec_verify_batch_dev has every shard present, so no
 * `present` pattern says what to rebuild.  With parity >= 2 the code itself
 * says which single shard is wrong.  Per block, with the syndrome
 * s = C * data ^ stored parity (one byte per parity row and column):
 *   - parity shard r damaged: only row r differs (the verify word is 1 << r);
 *   - data shard j damaged: every row differs, and in every column
 *     s_r == (C[r][j] / C[0][j]) * s_0.
 * located[b] is SHMR_EC_LOCATE_CLEAN (the verify word is 0), the index in
 * [0, total) of the one shard whose damage explains the block, or
 * SHMR_EC_LOCATE_NONE (no single shard does: several are damaged).
 * What the answer promises:
 *   - parity >= 3: damage in two shards is never taken for damage in one.
 *   - parity == 2: the code has distance 3; damage in two shards can look
 *     like damage in a third, as with any distance-3 code.
 *   - data shards are told apart by the first group of min(parity, 4) parity
 *     rows only.  Damage in one data shard plus parity rows beyond that group
 *     is reported as the data shard; shmr_ec_scrub_batch_dev catches it with
 *     its closing verify.
 * Needs 2 <= parity <= 32 (INVALID_ARGUMENT otherwise: below 2 nothing can be
 * located, above 32 several rows share bit 31 of the verify word). */
#define SHMR_EC_LOCATE_CLEAN (-1)
#define SHMR_EC_LOCATE_NONE (-2)

/* Bytes of device scratch shmr_ec_locate_batch_dev needs for nblocks blocks
 * (positive, never shrinking as nblocks grows); 0 for a codec it refuses. */
size_t shmr_ec_locate_work_size(const shmr_ec_t* rs, size_t nblocks);

/* Verify and locate nblocks blocks, addressed exactly as
 * shmr_ec_verify_batch_dev.  d_mismatch (nblocks uint32, device) receives that
 * call's words unchanged; d_located (nblocks int32, device) the answers above;
 * d_work is work_bytes >= shmr_ec_locate_work_size(rs, nblocks) bytes of
 * device scratch (4-byte aligned; too small: INVALID_ARGUMENT, nothing
 * enqueued).  Read-only over the shards: the verify kernels, then a kernel
 * that reads one word per tile of a block that is clean or differs in parity
 * rows only, and the data and first-group parity of the others.  Stream-
 * ordered, no allocation and no host readback.  NOT capturable: a `stream`
 * that is being captured into a graph is refused with INVALID_ARGUMENT and
 * nothing is enqueued (a replayed locate has returned answers that its
 * eager call does not; until that is understood the call stays out of
 * graphs, since a scrub writes what locate names). */
int shmr_ec_locate_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch,
                             size_t data_block_pitch, const uint8_t* d_parity,
                             size_t parity_shard_pitch, size_t parity_block_pitch,
                             size_t nblocks, size_t shard_len, uint32_t* d_mismatch,
                             int32_t* d_located, void* d_work, size_t work_bytes,
                             int device, void* stream);

/* The whole scrub, blocking (NOT stream-ordered, NOT capturable: it waits on
 * `stream` twice and takes pooled device scratch): locate; copy the answers
 * to the host; rebuild the located shard of each such block in place through
 * shmr_ec_reconstruct_ptrs_dev's path (present = every shard but that one);
 * verify again, and demote a rebuilt block that still differs to
 * SHMR_EC_LOCATE_NONE (its located shard has been rewritten).  Blocks that
 * locate reports as SHMR_EC_LOCATE_NONE are not written at all.
 * located_host: nblocks int32 of HOST memory, or NULL.  counts (HOST, 3
 * entries): blocks clean, repaired, not repairable; written (zeroed first)
 * only once the arguments and the device have been accepted, so a refused
 * call leaves them alone. */
int shmr_ec_scrub_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch,
                            size_t data_block_pitch, uint8_t* d_parity, size_t parity_shard_pitch,
                            size_t parity_block_pitch, size_t nblocks, size_t shard_len,
                            int32_t* located_host, uint64_t* counts, int device, void* stream);

/* ---- scrub, parity >= 4: locate and repair two damaged shards per block ------ *
 * The calls above stop at one damaged shard per block.  A code with
 * parity >= 4 has distance >= 5 and determines two: with G the first group of
 * four parity rows and H' = [C[0:4] | I_4], damage in shards e and f leaves
 * s_G in span(H'_e, H'_f) in every column, and no other pair is consistent
 * with every column once each of the two is hit somewhere.  Per block two
 * answers, located[2b] and located[2b + 1]:
 *   - (shmr_ec_locate_batch_dev's answer, SHMR_EC_LOCATE_CLEAN) wherever that
 *     answer is not SHMR_EC_LOCATE_NONE: clean blocks and single shards are
 *     exactly locate's;
 *   - (lower index, higher index) of the one pair of shards whose damage
 *     explains the block;
 *   - (SHMR_EC_LOCATE_NONE, SHMR_EC_LOCATE_NONE): no single shard and no pair.
 * What the answer promises:
 *   - the located pair is exact for damage in two of the data + 4 shards the
 *     group sees (the data shards and parity shards 0 .. 3);
 *   - parity == 4 (distance 5): damage in three shards can pass for damage in
 *     two, as with any distance-5 code;
 *   - parity >= 5: that case is caught by shmr_ec_scrub_pair_batch_dev's
 *     closing verify;
 *   - parity rows at and beyond 4 are used only through the verify word, as in
 *     locate: a block with a row there that does not differ has no pair with a
 *     data shard in it, and a data shard plus a parity shard beyond the group
 *     is still reported as the data shard alone (and demoted by the scrub's
 *     closing verify).
 * Needs 4 <= parity <= 32 and data <= 29 (the pair tables of a larger code do
 * not fit the 64 KiB of LDS they are staged in); INVALID_ARGUMENT otherwise. */

/* Bytes of device scratch shmr_ec_locate_pair_batch_dev needs for nblocks
 * blocks (positive, never shrinking as nblocks grows, at least
 * shmr_ec_locate_work_size: locate's scratch, the pair bitmaps, a worklist and
 * its counter); 0 for a codec it refuses. */
size_t shmr_ec_locate_pair_work_size(const shmr_ec_t* rs, size_t nblocks);

/* Verify, locate, and locate pairs in nblocks blocks: arguments as
 * shmr_ec_locate_batch_dev, except that d_located is nblocks * 2 int32 (device)
 * and d_work is work_bytes >= shmr_ec_locate_pair_work_size(rs, nblocks).
 * d_mismatch receives verify's words unchanged.  Read-only over the shards:
 * behind locate's kernels, a kernel that lists the blocks no single shard
 * explains and one that reads the data and first-group parity of the listed
 * blocks (one word per workgroup when none is listed).  Stream-ordered, no
 * allocation and no host readback.  NOT capturable, as
 * shmr_ec_locate_batch_dev: a capturing `stream`, a small d_work and an
 * unsupported codec are refused with INVALID_ARGUMENT and nothing is
 * enqueued. */
int shmr_ec_locate_pair_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch,
                                  size_t data_block_pitch, const uint8_t* d_parity,
                                  size_t parity_shard_pitch, size_t parity_block_pitch,
                                  size_t nblocks, size_t shard_len, uint32_t* d_mismatch,
                                  int32_t* d_located, void* d_work, size_t work_bytes,
                                  int device, void* stream);

/* The whole scrub for up to two damaged shards per block, blocking (NOT
 * stream-ordered, NOT capturable), arguments as shmr_ec_scrub_batch_dev:
 * locate pairs; copy the answers to the host; rebuild the one or two located
 * shards of each such block in place through shmr_ec_reconstruct_ptrs_dev's
 * path (present = every shard but those); verify again, and demote a rebuilt
 * block that still differs to (SHMR_EC_LOCATE_NONE, SHMR_EC_LOCATE_NONE) (its
 * located shards have been rewritten).  Blocks reported
 * SHMR_EC_LOCATE_NONE are not written at all.
 * located_host: nblocks * 2 int32 of HOST memory, or NULL.  counts (HOST, 4
 * entries): blocks clean, repaired in one shard, repaired in two, not
 * repairable; written (zeroed first) only once the arguments and the device
 * have been accepted, so a refused call leaves them alone. */
int shmr_ec_scrub_pair_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch,
                                 size_t data_block_pitch, uint8_t* d_parity,
                                 size_t parity_shard_pitch, size_t parity_block_pitch,
                                 size_t nblocks, size_t shard_len, int32_t* located_host,
                                 uint64_t* counts, int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_locate_checked_plan): the
 * coefficients the pair kernel multiplies by, in pair-index order.  The
 * candidates of a block are the data-data pairs (a, b), a < b, in
 * lexicographic order, then the data-parity pairs (a, data + r), r < 4, at
 * a * 4 + r; *npairs = data (data - 1) / 2 + 4 data of them.  coeffs: four
 * bytes per data-data pair (s_2 == c0 s_0 ^ c1 s_1, s_3 == c2 s_0 ^ c3 s_1),
 * then two per data-parity pair (the ratios of the two rows other than r and
 * the base row against the base row, ascending row; the base row is row 0,
 * or row 1 for r == 0): 2 data (data - 1) + 8 data bytes.  coeffs_len below
 * that, or a codec the pair calls refuse: INVALID_ARGUMENT. */
int shmr_ec_locate_pair_plan(shmr_ec_t* rs, uint8_t* coeffs, size_t coeffs_len, uint32_t* npairs);

/* ---- parity delta update: writes into device-resident blocks ---------------- *
 * Changes part of a resident block and keeps its parity valid without
 * re-encoding it.  The code is linear: for every update,
 *   - bytes [offset, offset + len) of data shard `shard` of block `block`
 *     become d_src[src_offset .. src_offset + len);
 *   - every parity row r gets parity_r[col] ^= C[r][shard] * (old[col] ^ new[col])
 *     on those columns.
 * No other byte is written: not the other shards, the pitch padding past
 * shard_len, or the other blocks.  The syndrome of every block is unchanged:
 * a codeword stays a codeword, a damaged block keeps exactly its damage.
 * Traffic is (3 + 2 * parity) * len per update instead of a whole encode. */
typedef struct shmr_ec_update {
    uint32_t block;      /* block index, addressed as in shmr_ec_encode_batch_dev */
    uint32_t shard;      /* data shard, < data */
    uint64_t offset;     /* first byte within the shard */
    uint64_t len;        /* bytes, > 0, offset + len <= shard_len */
    uint64_t src_offset; /* where the new bytes start in d_src */
} shmr_ec_update;

/* Applies nupdates updates (HOST array) to nblocks blocks addressed exactly as
 * shmr_ec_encode_batch_dev; d_src: src_bytes bytes of DEVICE memory on
 * `device` holding the new bytes.  d_src MUST NOT overlap the shards (the
 * caller's contract: it is not checked, and the result of an overlap is
 * undefined).  Any alignment of the bases, pitches, offset and src_offset and
 * any parity >= 1 is accepted.
 * Checked in this order, all before any device work: NULL rs
 * (INVALID_ARGUMENT); nupdates == 0 or nblocks == 0 (OK, nothing enqueued);
 * shard_len == 0 (EMPTY_SHARD); a NULL pointer (INVALID_ARGUMENT); per update
 * block >= nblocks, shard >= data, len == 0, offset + len > shard_len or
 * src_offset + len > src_bytes (INVALID_ARGUMENT); two updates whose byte
 * ranges intersect in the same (block, shard) (INVALID_ARGUMENT: the order of
 * two writes to one byte is not defined within a call); the device.
 * Updates of different shards of a block over the same columns are fine: the
 * call orders them itself (rounds, shmr_ec_update_rounds).
 * Stream-ordered; after the first call on a device no blocking call of the
 * library's own.  NOT capturable: a `stream` that is being captured into a
 * graph is refused with INVALID_ARGUMENT and nothing is enqueued. */
int shmr_ec_update_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch,
                             size_t data_block_pitch, uint8_t* d_parity, size_t parity_shard_pitch,
                             size_t parity_block_pitch, size_t nblocks, size_t shard_len,
                             const shmr_ec_update* updates, size_t nupdates, const uint8_t* d_src,
                             size_t src_bytes, int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_reconstruct_plan): the checks of
 * shmr_ec_update_batch_dev on the list, then the round each update runs in
 * (round_of: nupdates entries, or NULL) and the number of rounds.  Two updates
 * of one block share a round only if their column ranges are disjoint (the
 * kernel stores exactly the parity bytes of an update's columns), so pairwise
 * disjoint ranges take 1 round and m shards of a block written over the same
 * columns take m. */
int shmr_ec_update_rounds(const shmr_ec_t* rs, const shmr_ec_update* updates, size_t nupdates,
                          size_t nblocks, size_t shard_len, size_t src_bytes, uint32_t* round_of,
                          uint32_t* nrounds);

/* Reconstruct nblocks blocks in place.  All total shards of block b live at
 * d_shards + b*block_pitch + i*shard_pitch.  present is HOST memory,
 * nblocks x total flags (row-major).  Blocks may have different presence
 * patterns; validation of every block precedes any launch. */
int shmr_ec_reconstruct_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch,
                                  size_t block_pitch, const uint8_t* present, size_t nblocks,
                                  size_t shard_len, int data_only, int device, void* stream);

/* ---- ranged reads from device-resident blocks, degraded or whole -------------- *
 * The read half of shmr_ec_update_batch_dev (VirtualBlock::read): byte ranges of
 * data shards copied out of resident blocks into one destination buffer.  The
 * code is column-wise -- column c of an absent shard depends only on column c
 * of the inputs -- so a range of a lost shard is rebuilt from the same range of
 * `data` survivors, without rebuilding the shard.  For every request,
 * d_dst[dst_offset .. dst_offset + len) receives bytes [offset, offset + len) of
 * data shard `shard` of block `block`: the bytes that
 * shmr_ec_reconstruct_batch_dev(..., data_only = 1) would leave in that shard
 * for the block's `present` row.
 *   - shard present: its stored bytes, a plain copy (traffic 2 * len);
 *   - shard absent: per column the sum over t of D[shard][t] * input_t[col],
 *     the inputs the first `data` present shards in index order (the crate's
 *     rule; parity shards can be inputs, never requests), D the row that
 *     shmr_ec_reconstruct_plan gives for the pattern (traffic (data + 1) * len).
 * Read-only over the shards: no shard byte is written, absent slots are never
 * read, and nothing of d_dst outside the requested ranges is written.
 * NOT checked: the survivors.  A damaged survivor is rebuilt into the answer
 * exactly as a plain reconstruct rebuilds it; shmr_ec_reconstruct_checked_batch_dev
 * and shmr_ec_locate_checked_batch_dev are the calls that look. */
typedef struct shmr_ec_read {
    uint32_t block;      /* block index, addressed as in shmr_ec_reconstruct_batch_dev */
    uint32_t shard;      /* data shard, < data */
    uint64_t offset;     /* first byte within the shard */
    uint64_t len;        /* bytes, > 0, offset + len <= shard_len */
    uint64_t dst_offset; /* where the bytes go in d_dst */
} shmr_ec_read;

/* Serves nreads requests (HOST array) from nblocks blocks addressed exactly as
 * shmr_ec_reconstruct_batch_dev, `present` as there (HOST flags, nblocks x
 * total, one pattern per block; blocks of different patterns share a launch).
 * d_dst: dst_bytes bytes of DEVICE memory on `device`.  d_dst MUST NOT overlap
 * the shards (the caller's contract: it is not checked, and the result of an
 * overlap is undefined).  Any alignment of the base, pitches, offset and
 * dst_offset is accepted.
 * Checked in this order, all before any device work: NULL rs
 * (INVALID_ARGUMENT); nreads == 0 or nblocks == 0 (OK, nothing enqueued);
 * shard_len == 0 (EMPTY_SHARD); a NULL pointer (INVALID_ARGUMENT); per request
 * block >= nblocks, shard >= data, len == 0, offset + len > shard_len or
 * dst_offset + len > dst_bytes (INVALID_ARGUMENT); two requests whose
 * destination ranges intersect (INVALID_ARGUMENT; two requests may read the
 * same source bytes); a block with fewer than `data` present shards
 * (TOO_FEW_SHARDS_PRESENT: every block is checked, as the reconstruct does);
 * the device.
 * Stream-ordered, no host readback; after the first call on a device no
 * blocking call and no allocation of the library's own.  NOT capturable: a
 * `stream` that is being captured into a graph is refused with
 * INVALID_ARGUMENT and nothing is enqueued.  One launch per table chunk
 * (shmr_ec_read_plan), counted under SHMR_EC_DEV_LAUNCHES.
 * Whole-shard reads belong to shmr_ec_reconstruct_batch_dev_out: measured on
 * RS(8,3) x 4 MiB x 512 blocks, a whole lost shard per block takes 1.19x the
 * time of that call (small ranges: 5.2x faster at 4 KiB and 3.7x at 64 KiB
 * than rebuilding the shards and copying the ranges). */
int shmr_ec_read_batch_dev(shmr_ec_t* rs, const uint8_t* d_shards, size_t shard_pitch,
                           size_t block_pitch, const uint8_t* present, size_t nblocks,
                           size_t shard_len, const shmr_ec_read* reads, size_t nreads,
                           uint8_t* d_dst, size_t dst_bytes, int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_update_rounds): the checks of
 * shmr_ec_read_batch_dev on the list and the flags, in its order, then per
 * request whether it is rebuilt (rebuilt: nreads entries, 0 copy / 1 rebuild,
 * or NULL), the number of kernel pieces (a request is a byte-granular head, whole
 * 16-byte chunks and a byte-granular tail) and the number of table chunks the
 * list uploads in (one launch each). */
int shmr_ec_read_plan(shmr_ec_t* rs, const uint8_t* present, size_t nblocks, size_t shard_len,
                      const shmr_ec_read* reads, size_t nreads, size_t dst_bytes,
                      uint8_t* rebuilt, uint32_t* npieces, uint32_t* nchunks);

/* ---- parity delta update of degraded device-resident blocks ------------------- *
 * The write half of shmr_ec_read_batch_dev: shmr_ec_update_batch_dev for blocks
 * with absent shards, without rebuilding them first.  The code is linear and
 * column-wise, so for every update of columns [a, b) = [offset, offset + len)
 * of data shard j = `shard` of block B = `block`:
 *   - shard j present: data_j[col] becomes d_src[src_offset + col - a], and
 *     every PRESENT parity row r of B gets parity_r[col] ^= C[r][j] * (old[col]
 *     ^ new[col]); absent parity slots are skipped (traffic (3 + 2 p') * len,
 *     p' the present parity rows);
 *   - shard j absent: old[col] is the sum over t of D[j][t] * input_t[col], the
 *     bytes shmr_ec_reconstruct_batch_dev(..., data_only = 1) would leave in the
 *     shard -- the inputs the first `data` present shards in index order (the
 *     crate's rule; parity shards can be inputs), D the row that
 *     shmr_ec_reconstruct_plan gives for the pattern.  delta = old ^ new goes
 *     into every present parity row as above; slot j stays absent and is not
 *     touched (traffic (data + 1 + 2 p') * len).  Afterwards the survivors are
 *     the punctured codeword of the new data: any later reconstruct or read
 *     returns the new bytes.
 * Byte-exact footprint: only bytes [a, b) of shard j (if present) and of the
 * present parity shards of B are stored; absent slots are never read and never
 * written; the pitch padding past shard_len, the other shards and the other
 * blocks keep their bytes.  A block with every shard present gets exactly the
 * bytes shmr_ec_update_batch_dev writes.
 * Damage is preserved: what is XORed into the present shards is the punctured
 * codeword of delta, so the surplus-row word of
 * shmr_ec_reconstruct_checked_batch_dev is the same before and after.  NOT
 * checked: the survivors.  A damaged survivor among the inputs goes into `old`
 * as a plain reconstruct would rebuild it; shmr_ec_reconstruct_checked_batch_dev
 * and shmr_ec_locate_checked_batch_dev are the calls that look.
 * Several updates of one block over intersecting columns, of present and absent
 * shards in any mix, are ordered by the call itself with the round rule of
 * shmr_ec_update_rounds (same block, disjoint columns: same round).  The result
 * does not depend on the order of the rounds: each round leaves the survivors
 * a punctured codeword plus the original damage.
 *
 * Applies nupdates updates (HOST array, the struct of shmr_ec_update_batch_dev)
 * to nblocks blocks addressed exactly as shmr_ec_read_batch_dev: all total
 * shards at one pitch, `present` HOST flags, nblocks x total, one pattern per
 * block (blocks of different patterns share a launch).  d_src: src_bytes bytes
 * of DEVICE memory on `device` holding the new bytes.  d_src MUST NOT overlap
 * the shards (the caller's contract: it is not checked, and the result of an
 * overlap is undefined).  Any alignment of the base, pitches, offset and
 * src_offset and any code shmr_ec_update_batch_dev takes (parity >= 1) is
 * accepted.
 * Checked in this order, all before any device work: NULL rs
 * (INVALID_ARGUMENT); nupdates == 0 or nblocks == 0 (OK, nothing enqueued);
 * shard_len == 0 (EMPTY_SHARD); a NULL pointer, `present` included
 * (INVALID_ARGUMENT); the per-update range checks and the intersecting-ranges
 * check of shmr_ec_update_batch_dev (INVALID_ARGUMENT); a block, updated or
 * not, with fewer than `data` present shards (TOO_FEW_SHARDS_PRESENT); the
 * device.
 * Stream-ordered, no host readback; after the first call on a device no
 * blocking call of the library's own.  NOT capturable: a `stream` that is being
 * captured into a graph is refused with INVALID_ARGUMENT and nothing is
 * enqueued.  One launch per round per table chunk
 * (shmr_ec_update_degraded_plan), counted under SHMR_EC_DEV_LAUNCHES.
 * Measured on RS(8,3) x 4 MiB x 512 blocks with one data shard lost per block,
 * against shmr_ec_reconstruct_batch_dev + shmr_ec_update_batch_dev: a write into
 * the lost shard is 4.6x faster at 4 KiB, 4.1x at 64 KiB and 1.12x at the whole
 * shard; rebuilding first is never faster, up to all `data` shards of every
 * block (1.03x).  A cache that rewrites most of a block
 * should rebuild and re-encode it instead, as for shmr_ec_update_batch_dev. */
int shmr_ec_update_degraded_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch,
                                      size_t block_pitch, const uint8_t* present, size_t nblocks,
                                      size_t shard_len, const shmr_ec_update* updates,
                                      size_t nupdates, const uint8_t* d_src, size_t src_bytes,
                                      int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_read_plan): the checks of
 * shmr_ec_update_degraded_batch_dev on the list and the flags, in its order,
 * then the rounds as shmr_ec_update_rounds reports them (round_of: nupdates
 * entries), per update whether its shard is absent (rebuilt: nupdates entries,
 * 0 present / 1 absent), the number of kernel pieces and the number of table
 * chunks the list uploads in.  Any out pointer may be NULL. */
int shmr_ec_update_degraded_plan(shmr_ec_t* rs, const uint8_t* present, size_t nblocks,
                                 size_t shard_len, const shmr_ec_update* updates, size_t nupdates,
                                 size_t src_bytes, uint32_t* round_of, uint32_t* nrounds,
                                 uint8_t* rebuilt, uint32_t* npieces, uint32_t* nchunks);

/* ---- checked reconstruct: verify the spare shards while rebuilding ----------- *
 * shmr_ec_reconstruct_batch_dev reads the first `data` present shards of a
 * block and never looks at the other present ones; shmr_ec_verify_batch_dev
 * needs every shard present.  This call does both in one pass over a block
 * with absent shards, so damage in a surviving shard is reported instead of
 * being rebuilt into the absent ones unnoticed.  Per block, with np >= data
 * present shards:
 *   - inputs: the first `data` present shards in index order (the crate's rule);
 *   - rebuilt: exactly the shards, rows and bytes of
 *     shmr_ec_reconstruct_batch_dev for this pattern and data_only;
 *   - surplus: the np - data present shards behind the inputs (always parity
 *     shards; with every shard present, the whole parity).  Each surplus shard
 *     data + r is recomputed from the inputs and compared on [0, shard_len).
 * d_mismatch[b], b the block's index in the batch: 0 if every surplus shard
 * agrees (or there is none: np == data), else bit min(r, 31) for each surplus
 * parity row r that differs -- the encoding of shmr_ec_verify_batch_dev, whose
 * word a block with every shard present gets exactly (nothing of it is
 * written).  The code is MDS: one damaged input byte makes EVERY surplus row
 * differ (the word is shmr_ec_checked_rows of the pattern), damage in surplus
 * shard data + r only row r.  Rebuilt bytes are written whether or not the
 * word ends up non-zero: the word says they are suspect.
 * Addressing and `present` exactly as shmr_ec_reconstruct_batch_dev (HOST
 * flags, nblocks x total, patterns may differ per block, every block validated
 * before any launch); absent slots are never read.  d_mismatch: nblocks uint32
 * words of DEVICE memory, 4-byte aligned, overwritten (the zeroing is part of
 * the enqueued work).
 * Checked in this order, all before any device work: NULL rs
 * (INVALID_ARGUMENT); nblocks == 0 (OK, nothing enqueued); shard_len == 0
 * (EMPTY_SHARD); a NULL pointer or unknown flag bits (INVALID_ARGUMENT); a
 * block with fewer than `data` present (TOO_FEW_SHARDS_PRESENT); the device.
 * Stream-ordered, no host readback.  NOT capturable: a `stream` that is being
 * captured into a graph is refused with INVALID_ARGUMENT and nothing is
 * enqueued.  Counted under SHMR_EC_DEV_BLOCKS_VERIFIED (every block),
 * SHMR_EC_DEV_BLOCKS_RECONSTRUCTED (blocks with an absent shard) and
 * SHMR_EC_DEV_LAUNCHES (per pattern, one per group of <= 4 plan rows). */
#define SHMR_EC_CHECK_DATA_ONLY 1  /* as data_only of shmr_ec_reconstruct_batch_dev */
#define SHMR_EC_CHECK_NO_REBUILD 2 /* compare only: no shard is written ("verify with erasures") */
int shmr_ec_reconstruct_checked_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch,
                                          size_t block_pitch, const uint8_t* present,
                                          size_t nblocks, size_t shard_len, int flags,
                                          uint32_t* d_mismatch, int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_reconstruct_plan): the bit mask
 * (bit min(r, 31)) of the parity rows the check compares for one presence
 * pattern.  Counts as shmr_ec_reconstruct_plan (TOO_FEW / TOO_MANY_SHARDS,
 * TOO_FEW_SHARDS_PRESENT). */
int shmr_ec_checked_rows(const shmr_ec_t* rs, const uint8_t* present, size_t nshards, uint32_t* rows);

/* Host only; for tests and tools: the plan the checked reconstruct runs for a
 * presence pattern and `flags`, in the shape of shmr_ec_reconstruct_plan.
 * Rows [0, *n_store) are stored to shard out_idx[m] (the rows of
 * shmr_ec_reconstruct_plan, verbatim); rows [*n_store, *n_store + *n_check)
 * are compared with the stored bytes of surplus shard out_idx[m].
 * out_idx holds total entries, out_rows at least (*n_store + *n_check) * data. */
int shmr_ec_checked_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards, int flags,
                         uint16_t* in_idx, uint16_t* out_idx, uint8_t* out_rows,
                         size_t out_rows_len, uint32_t* n_store, uint32_t* n_check);

/* ---- degraded blocks: locate a damaged survivor, and rebuild around it ------- *
 * The checked reconstruct says that a survivor of a degraded block is damaged;
 * these calls say which one, where the code can, and rebuild the block from
 * the others.  Per block with np present shards, s = np - data surplus shards
 * and D = M[surplus] * inv(M[inputs]) (one row per surplus shard, the rows the
 * check compares): the inputs and the surplus shards are an MDS code of their
 * own, so with the syndrome s_r of surplus row r
 *   - surplus shard data + r damaged: only its row differs (the word has
 *     exactly its bit);
 *   - input t damaged: every compared row differs (the word is
 *     shmr_ec_checked_rows of the pattern), and in every column
 *     s_r == (D[r][t] / D[0][t]) * s_0.
 * located[b] is SHMR_EC_LOCATE_CLEAN (the word is 0; also a block with s == 0,
 * where nothing was compared -- as the checked reconstruct reports it), the
 * index in [0, total) of the one present shard whose damage explains the block,
 * or SHMR_EC_LOCATE_NONE.  A block with every shard present gets exactly
 * shmr_ec_locate_batch_dev's answer.
 * What the answer promises:
 *   - s >= 3: damage in two survivors is never taken for damage in one.
 *   - s == 2: damage in two survivors in the same column can pass for damage
 *     in a third (distance 3).  Damage in different columns cannot.
 *   - s <= 1: nothing is located; a non-zero word gives SHMR_EC_LOCATE_NONE (one
 *     row cannot tell its own shard from an input).
 *   - inputs are told apart by the first min(s, 4) surplus rows only.  Damage
 *     in one input plus surplus rows beyond that group is reported as the
 *     input; shmr_ec_reconstruct_repair_batch_dev catches it with its closing
 *     verify.
 *
 * shmr_ec_locate_checked_batch_dev: shmr_ec_reconstruct_checked_batch_dev with
 * the same addressing, `present`, `flags` and counters -- d_mismatch receives
 * that call's words unchanged, the shards what that call writes -- plus
 * d_located (nblocks int32, device) and d_work, work_bytes >=
 * shmr_ec_locate_work_size(rs, nblocks) bytes of device scratch (4-byte
 * aligned).  Needs 2 <= parity <= 32 (INVALID_ARGUMENT otherwise, before
 * anything else is looked at).  Checked in that call's order, the scratch with
 * the pointers.  Behind the check's kernels: per presence pattern with s >= 2
 * a read-only kernel (one word per tile of a block whose word is not the
 * pattern's row mask; the inputs and the first min(s, 4) surplus shards of the
 * others) and per pattern an O(nblocks) kernel that writes the answers.  One
 * more SHMR_EC_DEV_LAUNCHES per pattern with s >= 2.  Stream-ordered, no
 * allocation and no host readback.  NOT capturable (INVALID_ARGUMENT, nothing
 * enqueued). */
int shmr_ec_locate_checked_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch,
                                     size_t block_pitch, const uint8_t* present, size_t nblocks,
                                     size_t shard_len, int flags, uint32_t* d_mismatch,
                                     int32_t* d_located, void* d_work, size_t work_bytes,
                                     int device, void* stream);

/* The whole repair, blocking (NOT stream-ordered, NOT capturable: it waits on
 * `stream` twice and takes pooled device scratch), built as
 * shmr_ec_scrub_batch_dev: the locate above with flags 0 (every absent shard
 * rebuilt at the checked reconstruct's one pass); the answers copied to the
 * host; for each block with a located shard, its absent shards and the located
 * one rebuilt through shmr_ec_reconstruct_batch_dev's path (present = the
 * given flags minus the located shard: at least `data` remain, since s >= 2);
 * a verify of the whole batch, every slot having been written; a repaired
 * block that still differs demoted to SHMR_EC_LOCATE_NONE (its located shard
 * has been rewritten).  A block that locate reports as SHMR_EC_LOCATE_NONE
 * keeps its present shards byte for byte; its absent slots hold the suspect
 * rebuild, the checked reconstruct's contract.
 * located_host: nblocks int32 of HOST memory, or NULL.  counts (HOST, 3
 * entries): blocks clean, repaired, not repairable; written (zeroed first)
 * only once the arguments and the device have been accepted, so a refused
 * call leaves them alone.  Checked in this order: NULL rs or counts, or a
 * codec outside 2 <= parity <= 32 (INVALID_ARGUMENT); nblocks == 0 (OK);
 * shard_len == 0 (EMPTY_SHARD); a NULL d_shards or present (INVALID_ARGUMENT);
 * a block with fewer than `data` present (TOO_FEW_SHARDS_PRESENT); the device. */
int shmr_ec_reconstruct_repair_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch,
                                         size_t block_pitch, const uint8_t* present,
                                         size_t nblocks, size_t shard_len, int32_t* located_host,
                                         uint64_t* counts, int device, void* stream);

/* Host only; for tests and tools (as shmr_ec_checked_plan): what the degraded
 * locate runs for a presence pattern.  in_idx (data entries): the inputs;
 * out_idx (total entries, the first s used): the s surplus shards, ascending;
 * ratio_rows: *n_rows rows of `data` entries, row r-1 entry t =
 * D[r][t] / D[0][t], *n_rows = min(s, 4) - 1, or 0 for s < 2 (nothing can be
 * located); *row_mask: shmr_ec_checked_rows of the pattern.  ratio_rows_len <
 * *n_rows * data, or a pattern with a zero D[0][t] (none of this matrix has
 * one): INVALID_ARGUMENT.  Counts and presence as shmr_ec_reconstruct_plan. */
int shmr_ec_locate_checked_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards,
                                uint16_t* in_idx, uint16_t* out_idx, uint8_t* ratio_rows,
                                size_t ratio_rows_len, uint32_t* n_rows, uint32_t* row_mask);

/* Reconstruct with the crate's memory semantics: every absent shard is
 * rebuilt into a buffer of its own (reed_solomon_erasure allocates
 * vec![0; len] for each None, called at src/vfs/block.rs:556-565; load_block
 * then concatenates them, :567-576), not into the block's slot.  Present
 * shards of block b are read in place at d_shards + b*block_pitch +
 * i*shard_pitch (absent slots are neither read nor written); block b's
 * rebuilt shards, in ascending shard index, are written to
 *     d_out + b*out_block_pitch + j*out_shard_pitch,  j = 0 .. rebuilt-1
 * (data_only != 0: the absent data shards only).  d_out must hold the largest
 * rebuilt count of the batch per block and must not overlap a present shard.
 * Blocks with every shard present write nothing.  Validation and errors as
 * shmr_ec_reconstruct_batch_dev. */
int shmr_ec_reconstruct_batch_dev_out(shmr_ec_t* rs, const uint8_t* d_shards, size_t shard_pitch,
                                      size_t block_pitch, const uint8_t* present, size_t nblocks,
                                      size_t shard_len, int data_only, uint8_t* d_out,
                                      size_t out_shard_pitch, size_t out_block_pitch, int device,
                                      void* stream);

/* Device-resident shards that live anywhere -- the crate's own argument shape
 * (ReedSolomon::encode(&mut [Vec<u8>]) at block.rs:427 over shards that
 * block.rs:408-419 copies into a Vec each; reconstruct(&mut [Option<Vec<u8>>])
 * at block.rs:560, every None rebuilt into a fresh buffer, :556-565), batched.
 * d_shards is a HOST array of nblocks x total DEVICE pointers:
 * d_shards[b*total + i] is shard i of block b, shard_len bytes, any alignment
 * (16-byte aligned shards take the vector kernels; otherwise the device's
 * verified unaligned access mode, else byte-granular).  The table is copied
 * before the call returns (the caller may reuse it) and uploaded on `stream`;
 * stream-ordered and graph-capturable as the calls above.
 * encode: shards [0, data) in, [data, total) overwritten with parity; every
 * pointer non-NULL.
 * reconstruct: present = nblocks x total host flags; absent shards point at
 * caller buffers that receive the rebuilt bytes (absent parity may be NULL
 * with data_only != 0); validation and errors as shmr_ec_reconstruct_batch_dev. */
int shmr_ec_encode_ptrs_dev(shmr_ec_t* rs, uint8_t* const* d_shards, size_t nblocks, size_t shard_len,
                            int device, void* stream);
int shmr_ec_reconstruct_ptrs_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const uint8_t* present,
                                 size_t nblocks, size_t shard_len, int data_only, int device, void* stream);

/* ---- host-buffer batches over one or more GPUs ---------------------------- *
 * Blocks held in HOST memory (the Block Cache / shard file buffers), whole
 * blocks round-robin across `devices` (block b -> devices[b % ndev]); per
 * device the H2D copy, the kernel and the D2H copy of successive chunks
 * overlap on separate streams.  host_shards[b * total + i] points at shard i
 * of block b, each shard_len bytes.  Mapped buffers (shmr_ec_host_alloc /
 * shmr_ec_host_register) are coded in place across PCIe (zero-copy); other
 * pinned buffers are DMA'd; pageable ones are gathered into a mapped pinned
 * mirror by a crew of copy threads and coded there ("mirror_zc").
 * Synchronous; every block is validated before device work. */
int shmr_ec_encode_blocks_host(shmr_ec_t* rs, uint8_t* const* host_shards, size_t nblocks,
                               size_t shard_len, const int* devices, int ndev);

/* Reconstruct host-resident blocks: present = nblocks x total flags; absent
 * shards are written (absent parity only when data_only == 0) and need a
 * buffer; semantics per block as shmr_ec_reconstruct. */
int shmr_ec_reconstruct_blocks_host(shmr_ec_t* rs, uint8_t* const* host_shards, const uint8_t* present,
                                    size_t nblocks, size_t shard_len, int data_only,
                                    const int* devices, int ndev);

/* Mapped (page-locked, device-visible from every GPU) host memory for Block
 * Cache buffers.  When every shard a host-buffer call touches (shmr_ec_encode,
 * shmr_ec_reconstruct, the *_blocks_host batches) lies in memory from
 * shmr_ec_host_alloc or a range given to shmr_ec_host_register, the kernels
 * read and write those buffers in place across PCIe (zero-copy: no staging
 * copies, no device buffers); otherwise the call stages through device memory. */
int shmr_ec_host_alloc(size_t bytes, void** out);
void shmr_ec_host_free(void* p);

/* Page-locks and maps an existing host range (e.g. a Rust Vec<u8> Block Cache
 * buffer) for zero-copy use; shmr_ec_host_unregister(p) with the same p undoes
 * it.  The range must stay allocated while registered. */
int shmr_ec_host_register(void* p, size_t bytes);
int shmr_ec_host_unregister(void* p);

/* Device memory for block batches (the *_batch_dev entry points), so a caller
 * (e.g. the Rust shim) needs no HIP bindings of its own.  contiguous == 0 is a
 * plain hipMalloc; contiguous != 0 asks for physically contiguous VRAM
 * (hipDeviceMallocContiguous, mapped with large page fragments) and fails
 * with OUT_OF_MEMORY if the driver cannot supply it (no silent fallback).
 * Measured on MI355X: contiguous VRAM lifts the XOR-only replica of the
 * RS(8,3) access pattern over 2,048 blocks (11 GiB) from 76 % to 78.5 % of
 * HBM peak, but the GF kernel itself runs the same on both (78.8 % at 2,048
 * blocks, 79.7 % at 512).  Free with shmr_ec_device_free on the same device.
 * The frees here (shmr_ec_device_free, shmr_ec_device_free_shards,
 * shmr_ec_pool_destroy, shmr_ec_host_free) are hipFree / hipHostFree: each
 * waits for the work of every stream of the device, a caller stream held by a
 * wait included.  The compute calls grow their own scratch without a free
 * (r06 s40); only the pinned bounce pool of pageable host calls frees, and only
 * a buffer returned while 32 others lie idle. */
int shmr_ec_device_alloc(int device, size_t bytes, int contiguous, void** out);
int shmr_ec_device_free(int device, void* p);

/* Shard buffers for the *_ptrs_dev calls with the slot placement of the
 * device-resident batches: nblocks x shards_per_block buffers of shard_len
 * bytes carved from one device slab (256-byte aligned base), each at the slot
 * pitch P = shard_len rounded up to 4 KiB, plus one 4 KiB page when that is a
 * multiple of 64 KiB:
 *     out_ptrs[b * shards_per_block + i] = slab + (b * shards_per_block + i) * P.
 * The crate keeps every shard in a Vec<u8> of its own (reference
 * src/vfs/block.rs:408-419, :556-565); a device Block Cache that takes its
 * shard buffers from here -- all total shards of its blocks in one call, and
 * the buffers for rebuilt shards (one per absent shard) in another -- hands
 * the *_ptrs_dev calls tables that form a slot grid, which run through the
 * strided kernels (knob "ptrs_grid").  The bytes are not initialised.  Free
 * with shmr_ec_device_free_shards(device, out_ptrs[0]); any other pointer
 * returns INVALID_ARGUMENT (shmr_ec_device_free(device, out_ptrs[0]) frees
 * it too). */
int shmr_ec_device_alloc_shards(int device, size_t nblocks, size_t shards_per_block, size_t shard_len,
                                uint8_t** out_ptrs);
int shmr_ec_device_free_shards(int device, uint8_t* first);

/* A device Block Cache of per-block slots (r06).  The reference's Block Cache
 * takes and drops one block's buffers at a time (src/vfs/block.rs:148-152,
 * :586-608); a shmr_ec_device_alloc_shards slab is freed only whole.  A pool
 * carves block slots -- shards_per_block shard buffers of shard_len bytes at
 * the slot pitch P of the device-resident batches (shard_len rounded up to 4
 * KiB, one page more for a multiple of 64 KiB) -- from device slabs of
 * slots_per_slab slots (allocated on demand, blocking), and hands them out one
 * block at a time, the lowest free slot first:
 *     out_ptrs[i] = slab + slot * shards_per_block * P + i * P.
 * Pointer tables over pool blocks, in any order and with holes, lie on the
 * slab's slot lattice: the *_ptrs_dev calls and the submission queue run them
 * through the strided kernels over their slots.  shmr_ec_pool_free takes
 * out_ptrs[0] of an alloc (anything else, or a second free: INVALID_ARGUMENT);
 * shmr_ec_pool_destroy frees every slab (no kernel may still use them).  The
 * bytes are not initialised. */
typedef struct shmr_ec_pool shmr_ec_pool_t;
int shmr_ec_pool_new(int device, size_t shards_per_block, size_t shard_len, size_t slots_per_slab,
                     shmr_ec_pool_t** out);
int shmr_ec_pool_alloc(shmr_ec_pool_t* pool, uint8_t** out_ptrs);
int shmr_ec_pool_free(shmr_ec_pool_t* pool, uint8_t* first);
int shmr_ec_pool_destroy(shmr_ec_pool_t* pool);
int shmr_ec_pool_stats(shmr_ec_pool_t* pool, uint64_t* slabs, uint64_t* slots, uint64_t* in_use);

/* ---- configuration -------------------------------------------------------- */

/* Device used by the host-buffer entry points (default 0; negative ->
 * SHMR_EC_INVALID_ARGUMENT).  Device IDs are checked at every compute call:
 * an ID >= the number of GPUs returns SHMR_EC_INVALID_ARGUMENT
 * (SHMR_EC_NO_DEVICE without a GPU); the *_blocks_host calls check every
 * entry of their device list the same way, and a NULL list or ndev <= 0 is
 * INVALID_ARGUMENT -- all before any buffer is touched.  A device listed
 * twice gets two shares of the blocks. */
int shmr_ec_set_device(shmr_ec_t* rs, int device);

/* Tuning knobs (process-wide).
 *
 * Host-path knobs (both flavours; they choose how bytes move, never what
 * the kernels compute): "coalesce" (0/1, default 0 -- measured no faster on
 * PCIe-bound mapped blocks): shmr_ec_encode /
 * shmr_ec_reconstruct (and *_start) whose shards all lie in mapped memory go
 * through the device's submission queue (above), merged with concurrent
 * calls, instead of one zero-copy launch per call; "coalesce_depth",
 * "coalesce_target", "coalesce_us", "coalesce_max" (blocks per launch, default
 * 1024), "coalesce_spin_us", "coalesce_watch_us", "coalesce_lead_us" and "coalesce_idle_us" (default 1000:
 * the watcher spins this long for calls after the queue goes idle, then sleeps): the queue (above).  "bounce_kib": pageable single-block calls whose
 * (k+p) x shard bytes fit in this many KiB go through one mapped bounce
 * buffer and a single zero-copy launch instead of per-shard DMA copies
 * (default 8192; 0 disables).  "mirror_zc" (0/1, default 1): pageable host
 * batches are gathered into a pinned mirror that the kernel codes in place
 * across PCIe (zero-copy) instead of DMA-ing it to device staging.
 * "ptrs_grid" (0/1, default 1): a *_ptrs_dev table whose shards form a slot
 * grid -- entry (b, i) at base + b * block_pitch + i * shard_pitch for the
 * inputs, and for the outputs (encode: parity rows; reconstruct: the absent
 * shards in place, or rebuilt shard j of block b at out + b * out_block_pitch +
 * j * out_shard_pitch) -- runs through the strided kernels of the *_batch_dev
 * calls with no table (same bytes; SHMR_EC_DEV_PTR_TABLE_GRIDS counts them);
 * 0 always takes the table kernels.  A table whose blocks sit on a slot
 * lattice (a slab or a pool, in any order, with holes) runs the strided
 * kernels over its slots when they form one arithmetic run or up to 32 runs
 * (segment launches); beyond that the table kernels run, measured faster than
 * an uploaded slot list ("lattice_list" (0/1, default 0): 1 takes the list).
 * Rebuilds with several erasure patterns in more runs than that take the
 * table kernels too.
 * "ptrs_direct" (default 16): zero-copy launches of at most this many 4 KiB
 * tiles read their shard-pointer table from pinned host memory in place
 * instead of uploading it first (0: always upload).  "sync_spin_us"
 * (default 0): the single-call and zero-copy paths poll their stream this
 * long before a blocking synchronize.
 *
 * Kernel knobs select a measurement variant of the kernel.  In the product
 * library (libshmr_ec.so) every launch uses the measured per-shape policy and
 * a kernel knob can only be set to its default (anything else returns
 * SHMR_EC_INVALID_ARGUMENT); the tools build (libshmr_ec_tools.so) takes:
 * "chunks" (16-B chunks per lane per tile: 1, 2, 4), "nt_load", "nt_store"
 * (nontemporal 0/1), "occ8" (0/1), "grid" (-1 one
 * workgroup per tile, 0 balanced persistent grid, >0 capped persistent
 * grid), "threads" (lanes per workgroup: 128, 256, 512), "depth" (register
 * ring depth = shards of loads in flight + 1: 1, 2, 3, 5, 9), "wgs_per_cu"
 * (0 = no cap, else the most workgroups resident per CU, enforced by LDS
 * padding; auto: 7 for single-row reconstructs, else no cap), "occ" (0, 5, 6, 7: register budget for that many waves per SIMD),
 * "early" (0/1: issue the first data loads before the plan's LDS staging
 * completes; auto: encodes with fewer than 8 data shards or 4 output rows),
 * "spre" (0/1: coefficient tables and shard offsets by scalar
 * loads one shard ahead, no LDS), "fuse_tail" (0/1: a shard length that is
 * not a multiple of the tile runs the partial last tile of every block at the
 * head of the full-tile launch instead of in a second launch), "glds" (0/1:
 * input ring in LDS filled by global_load_lds_dwordx4, depth = ring slots),
 * "serial" (0/1: GF math ordered one dword at a time, fewer VGPRs; auto:
 * encodes of 4 output rows), "sc1_store" (0/1: stores with the sc1 cache
 * policy instead of nontemporal; auto: reconstructs into a compact output),
 * "diag"
 * (0/1: XOR-only diagnostic kernel, WRONG results, for ceiling measurements).
 * Prefix "encode." or "decode." to set one operation class only.
 * "chunks", "nt_load", "nt_store", "depth", "wgs_per_cu", "occ", "early",
 * "spre", "fuse_tail", "glds", "serial" and "sc1_store" default to -2 (auto): the per-shape policy; any other value pins
 * the knob, and setting -2 returns it to the policy. */
int shmr_ec_set_tuning(const char* key, int value);
int shmr_ec_get_tuning(const char* key);

/* Writes the kernel variant that a launch of `rows` output rows over
 * `data_shards` inputs would use (encode: decode=0, reconstruct in place:
 * decode=1, reconstruct into a compact output: decode=2; over 16-byte aligned
 * device shard-pointer tables, *_ptrs_dev: encode 3, reconstruct 4). */
int shmr_ec_describe_variant(int decode, uint32_t data_shards, uint32_t rows, char* buf, size_t len);

/* Kernel inventory: every gf_apply kernel instantiation compiled into this
 * library -- the full-tile kernels the launch policy can select (mode 0, one
 * per reachable (rows, chunks, flags); the product list is derived from the
 * policy at compile time) and the partial-tile (mode 1), byte-granular (mode 2)
 * and realigning (mode 3) kernels per row count -- with the launches each has
 * served in this process.  Writes min(cap, count) entries and returns the
 * count (out may be NULL to query it).  flags are the kernel's template flags
 * (the F of gf_apply_kernel<R, U, MODE, F> in the code object's symbol). */
typedef struct shmr_ec_kernel_info {
    uint32_t rows, chunks, mode, flags;
    uint64_t launches;
} shmr_ec_kernel_info;
size_t shmr_ec_kernel_inventory(shmr_ec_kernel_info* out, size_t cap);

/* Decode-matrix LRU statistics of the (data, parity) codec (crate cache
 * semantics, capacity 254). */
int shmr_ec_cache_stats(const shmr_ec_t* rs, uint64_t* hits, uint64_t* misses);

/* Number of visible GPUs (0 when none; never fails). */
int shmr_ec_device_count(void);

/* Blocks the host-buffer entry points served zero-copy (mapped memory) and
 * through device staging since the library was loaded.  Either may be NULL. */
int shmr_ec_path_stats(uint64_t* zero_copy_blocks, uint64_t* staged_blocks);

/* Per-device counters since the library was loaded, for the device ID the
 * caller passed (blocks b -> devices[b % ndev] of the *_blocks_host calls, the
 * context's device, or a *_batch_dev call's device): out[i] for i < n in the
 * order below.  Every per-device object (plan images, upload rings, staging
 * streams) is created per device ID, so N GPUs show N sets.  In the tools
 * build, tuning key "alias_devices" = a adds IDs n .. n+a-1 that run on
 * physical GPU (id mod n) with their own per-device state (a one-GPU
 * rehearsal of multi-device bookkeeping); the product library has none. */
enum {
    SHMR_EC_DEV_BLOCKS_ENCODED = 0,
    SHMR_EC_DEV_BLOCKS_RECONSTRUCTED = 1, /* blocks with at least one absent shard */
    SHMR_EC_DEV_LAUNCHES = 2,             /* full-tile launch groups (<= 4 rows each) */
    SHMR_EC_DEV_PLAN_IMAGES = 3,          /* coefficient plans uploaded to this device */
    SHMR_EC_DEV_UPLOAD_RINGS = 4,         /* pinned upload rings created for this device */
    SHMR_EC_DEV_STAGING_STREAMS = 5,      /* staging / pipeline streams created for this device */
    SHMR_EC_DEV_BLOCKING_CALLS = 6,       /* blocking HIP calls the library made on its own: device
                                             init, plan-arena growth, upload-ring creation and waits
                                             for a ring slot (not the host-buffer calls' final sync) */
    SHMR_EC_DEV_PTR_TABLE_HITS = 7,       /* *_ptrs_dev tables reused from the device's table cache
                                             (no upload) */
    SHMR_EC_DEV_CAPTURE_TABLES = 8,       /* capture-reserve blocks taken by captured calls */
    SHMR_EC_DEV_CAPTURE_RELEASED = 9,     /* ... and returned when their graph was destroyed */
    SHMR_EC_DEV_PTR_TABLE_GRIDS = 10,     /* *_ptrs_dev calls whose table named a slot grid and ran
                                             through the strided kernels (no table) */
    SHMR_EC_DEV_BLOCKS_VERIFIED = 11,     /* blocks checked by shmr_ec_verify / shmr_ec_verify_batch_dev */
    SHMR_EC_DEV_COUNTERS = 12
};
int shmr_ec_device_stats(int device, uint64_t* out, size_t n);

#ifdef __cplusplus
}
#endif

#endif /* SHMR_EC_H */
