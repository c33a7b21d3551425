/*
 * g1s_diff.h -- C-ABI of the MI355X-native `diff` film-grain estimator.
 *
 * Drop-in boundary: the three-method object API of av1_grain::DiffGenerator as
 * grav1synth uses it (paths relative to the reference tree):
 *     DiffGenerator::new(fps, source_bd, denoised_bd)   src/main.rs:420-427
 *     differ.diff_frame(&source_frame, &denoised_frame) src/main.rs:442,462,482,502
 *     differ.finish() -> Vec<GrainTableSegment>         src/main.rs:524
 * and the `.tbl` writer fed from it (src/main.rs:525-529, 631-696).  A Rust
 * `grav1synth` binds these symbols with an `extern "C"` block.
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * All pixel work runs as HIP kernels for gfx950; the library fails loudly
 * (G1S_ERR_NO_DEVICE) when no HIP device is usable -- there is no CPU fallback.
 */
#ifndef G1S_DIFF_H
#define G1S_DIFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G1S_ABI_VERSION 1

/* av1_grain::{NUM_Y_POINTS, NUM_UV_POINTS, NUM_Y_COEFFS, NUM_UV_COEFFS}
 * (imported at src/parser/grain.rs:2; capacities at :27-31 and :46-50). */
#define G1S_NUM_Y_POINTS 14
#define G1S_NUM_UV_POINTS 10
#define G1S_NUM_Y_COEFFS 24
#define G1S_NUM_UV_COEFFS 25

enum {
  G1S_OK = 0,
  G1S_ERR_INVALID = -1,       /* bad argument / unsupported format */
  G1S_ERR_DIM_MISMATCH = -2,  /* source and denoised frame geometry differ */
  G1S_ERR_NOT_ENOUGH_FLAT = -3, /* "Not enough flat blocks to update noise estimate" */
  G1S_ERR_SOLVE = -4,         /* luma AR / strength equation system is singular */
  G1S_ERR_NO_DEVICE = -5,     /* no usable HIP device or kernel image */
  G1S_ERR_HIP = -6,           /* a HIP runtime call failed (see last_error) */
  G1S_ERR_STATE = -7,         /* call not legal in this state (e.g. after finish) */
  G1S_ERR_CAPACITY = -8,      /* output buffer too small */
  G1S_ERR_UNSUPPORTED = -9    /* valid request this path does not serve (a resize of deep samples without their bit depth) */
};

/* One decoded frame == v_frame::Frame<T> as produced by
 * BitstreamReader::decode_frame (src/reader.rs:172-212): planar Y,U,V; u8 for
 * 8-bit, native-endian u16 for 9..16-bit (src/reader.rs:51-67); chroma planes
 * decimated by (xdec, ydec) (src/reader.rs:69-85). */
typedef struct {
  uint32_t width, height;   /* luma plane size in samples */
  uint8_t bytes_per_sample; /* 1 or 2 */
  uint8_t xdec, ydec;       /* chroma subsampling log2: 4:2:0=(1,1) 4:2:2=(1,0) 4:4:4=(0,0) */
  uint8_t nplanes;          /* 1 (monochrome) or 3 */
  const void *data[3];
  size_t stride_bytes[3];
  int32_t on_device;        /* 0: host memory, copied before the call returns (the
                               `&Frame` borrow of src/main.rs:442).
                               1: device (HIP) memory of this process; must stay valid and
                               unmodified until g1s_diff_frames_released() covers the frame
                               (g1s_diff_sync()/finish at the latest).
                               2: PINNED host memory (hipHostMalloc / hipHostRegister): the copy
                               is queued and the call returns at once; must stay valid and
                               unmodified until g1s_diff_frames_copied() covers the frame */
} g1s_frame_t;

/* POD mirror of av1_grain::GrainTableSegment, field for field as consumed by
 * `impl From<av1_grain::GrainTableSegment>` at src/parser/grain.rs:108-133 and
 * src/main.rs:705-713. */
typedef struct {
  uint64_t start_time, end_time;
  uint16_t random_seed;
  uint8_t num_y_points, num_cb_points, num_cr_points;
  uint8_t scaling_points_y[G1S_NUM_Y_POINTS][2];
  uint8_t scaling_points_cb[G1S_NUM_UV_POINTS][2];
  uint8_t scaling_points_cr[G1S_NUM_UV_POINTS][2];
  uint8_t scaling_shift;
  uint8_t ar_coeff_lag;
  uint8_t num_y_coeffs, num_uv_coeffs; /* 2*lag*(lag+1) and that + 1 (src/parser/grain.rs:40-44) */
  int8_t ar_coeffs_y[G1S_NUM_Y_COEFFS];
  int8_t ar_coeffs_cb[G1S_NUM_UV_COEFFS];
  int8_t ar_coeffs_cr[G1S_NUM_UV_COEFFS];
  uint8_t ar_coeff_shift;
  uint8_t cb_mult, cb_luma_mult;
  uint16_t cb_offset;
  uint8_t cr_mult, cr_luma_mult;
  uint16_t cr_offset;
  uint8_t chroma_scaling_from_luma;
  uint8_t grain_scale_shift;
  uint8_t overlap_flag;
} g1s_segment_t;

/* Options; NULL == reference behaviour (lag 3, chroma estimated when present). */
typedef struct {
  uint32_t struct_size;   /* sizeof(g1s_opts_t), for forward compatibility */
  int32_t device;         /* HIP device ordinal; -1 = current device */
  uint32_t ar_coeff_lag;  /* 1..3; 0 = default (3, the reference's NOISE_MODEL_LAG) */
  uint32_t luma_only;     /* 1 = skip chroma planes (extension; reference: 0) */
  uint32_t batch_frames;  /* frames per kernel batch (<= 256); 0 = default: about 530 Mpixels' worth
                             (64 at 4K, 128 at 1080p) */
  uint32_t records_only;  /* frame-shard mode: do not fold here (the ordered fold runs
                             after the exchange, see g1s_fold_*).
                             0 = fold locally (single GPU);
                             1 = emit the per-frame records;
                             2 = run the per-frame half of the fold here as well and emit
                                 the per-frame "latest" states (~27 KB instead of ~250 KB a
                                 4K frame): only the ordered merge is left for rank 0. */
} g1s_opts_t;

typedef struct g1s_diff g1s_diff_t;

/* DiffGenerator::new (src/main.rs:420-427).  Returns NULL on failure; the
 * reason is then available from g1s_last_global_error(). */
g1s_diff_t *g1s_diff_new(int64_t fps_num, int64_t fps_den, uint32_t source_bit_depth,
                         uint32_t denoised_bit_depth, const g1s_opts_t *opts);
const char *g1s_last_global_error(void);

/* DiffGenerator::diff_frame (src/main.rs:442).  Frames are consumed in call
 * order.  Work is queued and may still be running when the call returns;
 * errors of queued frames (not enough flat blocks, singular system) surface on
 * a later diff_frame / sync / finish call, exactly once.
 * Device planes (on_device == 1) are read in place, through the pointer and the row stride given: any base the sample
 * size allows and any stride from the row upwards; 16-byte-aligned bases and strides in all six planes of a batch take
 * the fastest kernels, the others give the same table.  Refused for either frame and any plane, with G1S_ERR_INVALID
 * and the frame and plane in g1s_diff_last_error, before anything is copied or queued: a null plane pointer, a stride
 * smaller than the plane's row in bytes, an odd stride under 2-byte samples, a stride above 0xffffffff.  The refusal is
 * sticky (the job has lost a frame): every later call returns it.
 * Limits of what the kernels address, refused the same way (same code, same stickiness, the limit named in the text):
 *   size    a frame is at most 131 072 x 131 072 luma samples (4 096 blocks of 32 a side: the unit lists of the
 *           accumulation kernels pack a block's column and row into 12-bit fields).  131 073 either way is refused.
 *   stride  a row stride is at most 119 304 647 bytes (0xffffffff / 36: the kernels form row x stride in 32 bits for the 36
 *           rows of a block's tile with its halo), however few rows the plane has.
 *   extent  the bytes from a plane's first sample to its last, stride_bytes x (rows - 1) + the row's bytes, computed
 *           in 64 bits for every plane that is read, are at most 2^32 - 1.  Planes of up to 2^31 - 1 bytes run either
 *           chain of kernels; a batch that holds a device plane of 2^31 bytes or more runs the stream chain (same
 *           table, slower); 2^32 or more is refused.  Host frames are judged by the stride they are handed over with. */
int g1s_diff_frame(g1s_diff_t *, const g1s_frame_t *source, const g1s_frame_t *denoised);
/* n frame pairs in one call (same semantics as n diff_frame calls). */
int g1s_diff_frames(g1s_diff_t *, const g1s_frame_t *source, const g1s_frame_t *denoised, size_t n);
/* Drain all queued work (kernels + ordered fold). */
int g1s_diff_sync(g1s_diff_t *);
/* How many frame pairs, counted in the order they were handed over, the generator is done reading: the planes of
 * on_device frames (and of host frames, which are copied at the call anyway) before that count may be freed or
 * overwritten.  Monotonic; reaches the number of frames handed over after g1s_diff_sync / g1s_diff_finish.  A caller
 * that streams device-resident frames polls this instead of keeping every frame alive until the end. */
uint64_t g1s_diff_frames_released(g1s_diff_t *);
/* Same count for the HOST planes of frames handed over with on_device == 2 (pinned, copied asynchronously): frame
 * pairs before the returned count have been copied to the device.  wait_for > 0: block until at least that many have
 * (clamped to the frames handed over).  Frames with on_device 0 or 1 count as copied when their call returns. */
uint64_t g1s_diff_frames_copied(g1s_diff_t *, uint64_t wait_for);
/* DiffGenerator::finish (src/main.rs:524).  Ends the stream: afterwards no more frames are accepted.  *n_out = the
 * number of segments; if cap is too small the call returns G1S_ERR_CAPACITY with *n_out set and NOTHING is lost --
 * call again with a buffer of *n_out segments (the reference's Vec has no cap). */
int g1s_diff_finish(g1s_diff_t *, g1s_segment_t *out, size_t cap, size_t *n_out);
void g1s_diff_free(g1s_diff_t *);
/* anyhow::Error text of the last failure ("" if none). */
const char *g1s_diff_last_error(const g1s_diff_t *);

/* ---- frame-shard mode (multi-GPU): records out, ordered fold after exchange ---- */
/* Size in bytes of one per-frame record for this geometry (all exact integers:
 * AR normal-equation sums, per-block noise statistics, flat mask). */
size_t g1s_record_size(uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec,
                       uint32_t nplanes, uint32_t lag);
/* Zero a record buffer of g1s_record_size() bytes and write its header. */
int g1s_record_init(void *rec, size_t cap_bytes, uint32_t width, uint32_t height, uint32_t xdec,
                    uint32_t ydec, uint32_t nplanes, uint32_t lag);
/* Copies the records of all frames queued so far (frame order) into buf and
 * clears the internal list.  records_only generators only. */
int g1s_diff_take_records(g1s_diff_t *, void *buf, size_t cap_bytes, size_t *n_frames);
/* records_only == 2: latest states (g1s_latest_size() bytes each, frame order), whole batches:
 * sync = 0: exactly the batches queued before the two most recent ones that were not handed out yet
 * (waits for them if need be; deterministic, so that ranks deliver the same batches in the same
 * round); sync = 1: everything queued so far. */
int g1s_diff_take_latest(g1s_diff_t *, int sync, void *buf, size_t cap_bytes, size_t *n_frames);

/* ---- frame-shard rounds (one process per GPU): the exchange protocol behind the ABI, the transport with the host ----
 * The video is dealt to the N ranks batch by batch (batch j of batch_frames frame pairs -> rank j % N).  The job runs in
 * ROUNDS; in a round every rank (1) feeds its next batch, if the video still has one for it, (2) calls g1s_shard_pack,
 * (3) takes part in ONE gather of the fixed-size messages to rank 0 -- ncclAllGather / ncclSend+Recv on RCCL, MPI_Gather,
 * torch.distributed.gather: whatever the host application owns; this library links no communication library --
 * and rank 0 hands the N gathered messages, rank order, to g1s_shard_merge.  After the last feeding round every rank runs
 * g1s_shard_flush_rounds() more rounds with flush = 1 (the batches still in the generator's pipeline).  Rank 0's fold then finishes the table:
 * identical, byte for byte, to one generator fed the whole video (the states are exact; only their merge is ordered).
 * Message = 24-byte header + batch_frames latest states (g1s_latest_size() each, ~27 KB): N x 0.9 MB a round at 4K.
 * The header says WHICH of the sending rank's batches the message carries; the root merges by that index (global batch =
 * local batch * N + rank), so ranks that have fed different numbers of batches -- the idle rank of a short last round is
 * one feed behind -- may send different local batches in the same round: a batch that arrives before its predecessors
 * waits inside the fold, and g1s_fold_finish refuses (G1S_ERR_STATE) while one is still missing. */
size_t g1s_shard_msg_size(uint32_t ar_coeff_lag, uint32_t batch_frames);
/* This rank's message of the round: the latest states of ONE batch -- the oldest one not sent yet among those the generator
 * has finished (flush = 0: never waits; the message is empty when every unsent batch is still in the pipeline, which holds
 * at most g1s_shard_flush_rounds()) or among all (flush = 1: drains the generator first) -- or an empty message.  records_only = 2 generators. */
int g1s_shard_pack(g1s_diff_t *, int flush, void *msg, size_t cap_bytes);
/* How many batches a generator can still hold unsent when its last frame has been fed (its slots): the flush rounds every rank
 * runs behind its last feeding round. */
unsigned g1s_shard_flush_rounds(void);
/* A message from latest states made elsewhere (g1s_latest_from_record): n <= batch_frames.  Without a batch index: the
 * root merges such messages as they come (rounds in order, ranks in order) -- the caller keeps its ranks in lock step. */
int g1s_shard_msg_from_latest(const void *blobs, size_t n, uint32_t ar_coeff_lag, uint32_t batch_frames, void *msg, size_t cap_bytes);
/* The same with the index of the batch among the sending rank's batches (0, 1, ...; G1S_SHARD_NO_INDEX: none). */
#define G1S_SHARD_NO_INDEX UINT64_MAX
int g1s_shard_msg_from_latest_at(const void *blobs, size_t n, uint32_t ar_coeff_lag, uint32_t batch_frames, uint64_t local_batch,
                                 void *msg, size_t cap_bytes);
size_t g1s_latest_size(uint32_t ar_coeff_lag);
/* The per-frame half of the fold on the host: record -> latest state.  Thread-safe.  A frame
 * that fails (not enough flat blocks, singular system) yields a blob that carries the error;
 * it surfaces when the blob is pushed. */
int g1s_latest_from_record(const void *record, size_t size_bytes, uint32_t ar_coeff_lag, void *blob,
                           size_t cap_bytes);
/* The same for n records a stride apart, on the process' per-frame pool (G1S_FOLD_THREADS threads, the caller included). */
int g1s_latest_from_records(const void *records, size_t stride_bytes, size_t n, uint32_t ar_coeff_lag, void *blobs,
                            size_t blob_stride_bytes);
/* The cores this process may use: hardware threads cut to the cgroup CPU quota (the default size of the per-frame pool;
 * a launcher of several local ranks divides it among them: bench.py). */
unsigned g1s_usable_cpus(void);

typedef struct g1s_fold g1s_fold_t;
/* The sequential part of DiffGenerator (noise-model update, segmentation,
 * quantisation) over records, in frame order.  Pure host code. */
g1s_fold_t *g1s_fold_new(int64_t fps_num, int64_t fps_den, uint32_t lag);
int g1s_fold_push(g1s_fold_t *, const void *record, size_t size_bytes);
/* n records, stride_bytes apart, in frame order: the per-frame half runs on a
 * host thread pool, the ordered half serially.  Same result as n pushes. */
int g1s_fold_push_many(g1s_fold_t *, const void *records, size_t stride_bytes, size_t n);
/* n latest states, stride_bytes apart, in frame order: the ordered half only. */
int g1s_fold_push_latest(g1s_fold_t *, const void *blobs, size_t stride_bytes, size_t n);
/* Rank 0: the `world` gathered messages of one round, stride_bytes apart, rank order -> the ordered merge (by the batch
 * index the messages carry; messages without one: rounds must be merged in order). */
int g1s_shard_merge(g1s_fold_t *, const void *msgs, size_t stride_bytes, uint32_t world);
/* Same contract as g1s_diff_finish: G1S_ERR_CAPACITY leaves the segments in place for a second call. */
int g1s_fold_finish(g1s_fold_t *, g1s_segment_t *out, size_t cap, size_t *n_out);
void g1s_fold_free(g1s_fold_t *);
const char *g1s_fold_last_error(const g1s_fold_t *);
/* Frames folded so far (pushed or merged in order): a driver of the round protocol checks it against the frames it fed
 * before g1s_fold_finish -- a batch still inside a generator's pipeline is a frame missing here. */
uint64_t g1s_fold_frames(const g1s_fold_t *);

/* ---- `.tbl` text, byte for byte what src/main.rs:525-529,631-696 writes ---- */
/* Returns the number of bytes written (no NUL), or G1S_ERR_CAPACITY. */
long g1s_format_tbl(const g1s_segment_t *segs, size_t n, char *buf, size_t cap);
int g1s_write_tbl(const char *path, const g1s_segment_t *segs, size_t n);
/* The reader of the same text: av1_grain::parse_grain_table as `apply` calls it (src/main.rs:228-241).
 * *n_out = number of segments (also when cap is too small: G1S_ERR_CAPACITY); reason of a failure in err. */
int g1s_parse_tbl(const char *text, size_t len, g1s_segment_t *out, size_t cap, size_t *n_out, char *err, size_t errcap);
/* The segment `apply` stamps on a frame with presentation time packet_ts (src/parser/frame.rs:617-633): the
 * first one with start_time <= ts < end_time, or -1.  Like the reference, every hit advances that segment's
 * random_seed by DEFAULT_GRAIN_SEED (wrapping) before it is used. */
long g1s_tbl_segment_for(g1s_segment_t *segs, size_t n, uint64_t packet_ts);

/* ---- measurement hooks (bench.py) ---- */
typedef struct {
  uint64_t frames;            /* frame pairs processed by the kernels */
  uint64_t blocks, flat_blocks;
  /* HIP-event time per kernel family, summed over launches, milliseconds */
  double ms_flat_features, ms_flat_select, ms_ar_accumulate, ms_total_gpu;
  uint64_t launches_flat_features, launches_flat_select, launches_ar_accumulate;
  double ms_host_fold;        /* wall time spent in the ordered host fold */
  double ms_residual;         /* part of ms_ar_accumulate: the K0 residual pass over the input planes */
  uint64_t literal_blocks;    /* timed batches only: blocks the certified flat-block fast path left to the literal f64 kernel */
  double ms_chain;            /* set_timing(2): HIP-event time from the first kernel's start to the last kernel's end, summed over batches */
  uint64_t chain_batches;     /* ... the batches in that sum */
} g1s_stats_t;
int g1s_diff_get_stats(const g1s_diff_t *, g1s_stats_t *out);
/* Enable HIP-event timing of the batches (off by default: events serialise batches; a timed batch runs on one stream, alone on
 * the chip).  1: an event in front of every kernel (g1s_diff_kernel_times, the ms_* family sums); 2: ONE pair of events around the
 * batch's whole chain of kernels (ms_chain / chain_batches) -- no barrier packet between two of its launches. */
int g1s_diff_set_timing(g1s_diff_t *, int enable);
/* Timed batches: one line per kernel, "name\tmilliseconds\tlaunches\n" (HIP events around each launch, on the
 * stream the kernel runs on; the names are the ones rocprofv3 --kernel-trace prints).  Returns the number of bytes
 * written (no NUL) or G1S_ERR_CAPACITY. */
long g1s_diff_kernel_times(g1s_diff_t *, char *buf, size_t cap);
/* Flat-block finder: 0 (default) = integer moments + certified evaluation, literal f64 evaluation (one
 * wave per block) only for the blocks the certificate leaves open; 1 = literal evaluation of every
 * block, one lane per block; 2 = of every block, one wave per block (all three must agree bit for
 * bit: tests/test_gpu_parity.py).  Takes effect from the next batch. */
int g1s_diff_set_flat_finder(g1s_diff_t *, int mode);

/* ---- introspection of the most recently *completed* frame (parity tests) ---- */
/* Copies the frame's record (layout: g1s_record_* accessors below). */
int g1s_diff_last_record(const g1s_diff_t *, void *buf, size_t cap_bytes);
/* Record field accessors (so that bindings need not know the layout). */
int g1s_record_geometry(const void *rec, uint32_t *nbw, uint32_t *nbh, uint32_t *nplanes, uint32_t *lag);
const uint8_t *g1s_record_flat_mask(const void *rec);
const float *g1s_record_scores(const void *rec);
/* n x n sums S[i*n+j] and Sb[i] of plane c (chroma regressor n-1 pre-scaled by
 * ns = (1<<xdec)*(1<<ydec)); returns n. */
int g1s_record_ar_sums(const void *rec, uint32_t c, const int64_t **S, const int64_t **Sb, int64_t *nobs);
int g1s_record_block_stats(const void *rec, uint32_t c, const uint32_t **luma_sum,
                           const int32_t **sum_d, const uint32_t **sum_d2);

/* ---- the caller of the path: `grav1synth diff`'s frame-pair loop and a raw-video frame source ---- */
/* A frame source == BitstreamReader::get_frame (src/reader.rs:122-170) as the diff loop uses it:
 * returns 1 and fills *out (host or device planes, valid until the next call on this source),
 * 0 at end of stream (`None`), a negative G1S_ERR_* on failure (`Err`, `?`-propagated). */
typedef int (*g1s_next_frame_fn)(void *user, g1s_frame_t *out);
/* The loop of Commands::Diff (src/main.rs:432-521) with get_filtered_frame_pair (src/main.rs:615-629):
 * one frame from each source (source first), diff_frame on the pair, until a source ends.
 * Both ended together: normal end.  Only one ended: *unequal = 1 -- the reference warns "Videos did
 * not have equal frame counts. Resulting grain table may not be as expected." and stops there too.
 * The first error ends the loop and is returned.  g1s_diff_finish() is left to the caller
 * (src/main.rs:524).  *frames = pairs handed to diff_frame. */
int g1s_diff_run(g1s_diff_t *, g1s_next_frame_fn source, void *source_user, g1s_next_frame_fn denoised,
                 void *denoised_user, uint64_t *frames, int *unequal);

/* ---- `--filters` (N3): FilterChain of /root/reference/src/filters.rs ---- */
/* FilterChain::new (src/filters.rs:16-110): "name:arg=value,...;name:..." with the filters crop (top, bottom, left,
 * right) and resize (width, height, alg = hermite | catmullrom | mitchell | lanczos | spline36; default catmullrom).
 * Same grammar, same error texts ("Invalid filter syntax in \"..\"", "Unrecognized filter \"..\"", "Unrecognized crop
 * arg \"..\"", "invalid digit found in string", "Both width and height must be provided to resize filter", ...).
 * NULL + reason in err on a parse error; "" is the empty chain. */
typedef struct g1s_filters g1s_filters_t;
typedef struct {
  uint32_t kind;                     /* 0 = crop, 1 = resize */
  uint64_t top, bottom, left, right; /* crop */
  uint64_t width, height;            /* resize */
  char alg[16];                      /* resize */
} g1s_filter_desc_t;
g1s_filters_t *g1s_filters_new(const char *text, char *err, size_t errcap);
size_t g1s_filters_len(const g1s_filters_t *);
int g1s_filters_get(const g1s_filters_t *, size_t i, g1s_filter_desc_t *out);
/* FilterChain::apply (src/filters.rs:112-116) on a frame descriptor.  crop is extent arithmetic: *out points into
 * *in's planes (host or device), same strides, smaller width / height -- no sample is touched, so it costs nothing on
 * the device.  Crop amounts must be multiples of the chroma subsampling and leave at least one sample
 * (G1S_ERR_INVALID otherwise).  A chain with a resize filter is served by g1s_filters_apply_bd below (this call, without a
 * bit depth, takes 8-bit samples only and answers G1S_ERR_UNSUPPORTED for deeper ones).  filters == NULL: *out = *in. */
int g1s_filters_apply(const g1s_filters_t *, const g1s_frame_t *in, g1s_frame_t *out, char *err, size_t errcap);
/* FilterChain::apply(frame, source_bd) (src/filters.rs:112-116) with the resize filter served: crop as above; resize
 * (src/filters.rs:150-178: hermite / catmullrom / mitchell / lanczos / spline36) runs ON THE DEVICE `device` (-1: the
 * current one; host planes are staged there) and the resized frame comes back as device planes (on_device = 1) inside
 * buffer `slot` of a ring the chain owns -- valid until the chain is applied with the same slot again, or freed.  No CPU
 * fallback.  bit_depth = the source bit depth (8..16).  g1s_filters_apply = this with bit_depth 8 for 8-bit samples and a
 * refusal (G1S_ERR_UNSUPPORTED) for deeper ones when the chain resizes. */
int g1s_filters_apply_bd(const g1s_filters_t *, const g1s_frame_t *in, uint32_t bit_depth, int32_t device, uint32_t slot,
                         g1s_frame_t *out, char *err, size_t errcap);
int g1s_filters_has_resize(const g1s_filters_t *);
/* The taps of one axis of a resize (test / documentation aid): output i = sum over k < *taps of coef[i * taps + k] *
 * in[idx[i * taps + k]], k ascending, in f32 without fused multiply-adds; cap = entries idx / coef hold (dst * taps). */
int g1s_resize_plan(const char *alg, uint32_t src, uint32_t dst, uint32_t *taps, int32_t *idx, float *coef, size_t cap);
/* One frame (host or device planes) through the device resize, result into host planes (tests, the Python FilterChain).
 * A target above 65535 x 65535 is refused here as the filter parser refuses it (G1S_ERR_INVALID, the same text); a source
 * has no limit of its own: any width and height the frame's uint32_t fields and the device's memory hold. */
int g1s_resize_frame_to_host(const char *alg, const g1s_frame_t *in, uint32_t bit_depth, uint32_t out_w, uint32_t out_h,
                             int32_t device, void *const out_planes[3], const size_t out_stride_bytes[3], char *err, size_t errcap);
void g1s_filters_free(g1s_filters_t *);
/* g1s_diff_run with get_filtered_frame_pair's filter step (src/main.rs:615-629): the chain is applied to every SOURCE
 * frame before the pair is handed to diff_frame; the denoised frame is taken as it comes.  A frame index goes with
 * every error text.  filters == NULL: exactly g1s_diff_run. */
int g1s_diff_run_filtered(g1s_diff_t *, g1s_next_frame_fn source, void *source_user, g1s_next_frame_fn denoised,
                          void *denoised_user, const g1s_filters_t *filters, uint64_t *frames, int *unequal);

/* YUV4MPEG2 frame source: stands where the libav reader stands in the reference (what reaches the
 * estimator is the same planar Y,U,V u8 / little-endian u16 frame, src/reader.rs:172-212).  Frames
 * are read ahead by a thread (big frames: four positional reads at a time) into pinned host memory (a ring
 * of 4), so file IO, the H2D copies of
 * g1s_diff_frame and the kernels of earlier frames overlap.  Colour spaces: C420* / C422 / C444 /
 * Cmono with an optional p9..p16 depth suffix (8-, 10-, 12-bit 4:2:0 / 4:2:2 / 4:4:4 are what
 * src/reader.rs:51-85 accepts). */
typedef struct g1s_y4m g1s_y4m_t;
typedef struct {
  uint32_t width, height, bit_depth, xdec, ydec, nplanes;
  int64_t fps_num, fps_den;
} g1s_y4m_info_t;
g1s_y4m_t *g1s_y4m_open(const char *path, char *err, size_t errcap); /* NULL on failure, reason in err */
int g1s_y4m_get_info(const g1s_y4m_t *, g1s_y4m_info_t *out);
int g1s_y4m_next(void *y4m, g1s_frame_t *out); /* a g1s_next_frame_fn; user = the g1s_y4m_t* */
/* Bind the reader to the generator its frames go to (frame i of the reader = frame pair i of the generator): frames
 * then come out with on_device = 2 -- g1s_diff_frame queues their copies straight from the reader's pinned ring and
 * returns -- and the reader recycles a ring buffer only when g1s_diff_frames_copied() covers its frame.  Close the
 * reader after the generator has synced / finished.  NULL unbinds. */
int g1s_y4m_bind(g1s_y4m_t *, g1s_diff_t *);
const char *g1s_y4m_last_error(const g1s_y4m_t *);
void g1s_y4m_close(g1s_y4m_t *);
/* `grav1synth diff SOURCE DENOISED -o OUT` for two .y4m files (src/main.rs:414-531): frame rate from
 * the source, bit depths from each file, the loop above, finish, "filmgrn1" table to out_tbl. */
int g1s_diff_y4m_files(const char *source, const char *denoised, const char *out_tbl, const g1s_opts_t *opts,
                       uint64_t *frames, int *unequal, char *err, size_t errcap);
/* The same with `-f FILTERS` (src/main.rs:370-380): filters = NULL or "" for none.  A chain that does not parse:
 * G1S_ERR_INVALID and err = "Invalid filter chain: <reason>" (the reference logs that line and exits). */
int g1s_diff_y4m_files_filtered(const char *source, const char *denoised, const char *out_tbl, const g1s_opts_t *opts,
                                const char *filters, uint64_t *frames, int *unequal, char *err, size_t errcap);
/* The same command over several devices (north_star: frames shard across the GPUs of a node; the loop of src/main.rs:414-531):
 * ONE process, a generator per entry of `devices` (an ordinal may repeat), the two files' frame pairs dealt batch by batch
 * (batch j -> generator j % n_devices), the frame-shard rounds above with the host as the transport.  Same table, byte for
 * byte, as one generator; same return values and error texts as g1s_diff_y4m_files_filtered. */
int g1s_diff_y4m_files_sharded(const char *source, const char *denoised, const char *out_tbl, const g1s_opts_t *opts,
                               const char *filter_text, const int32_t *devices, uint32_t n_devices, uint64_t *frames_out,
                               int *unequal_out, char *err, size_t errcap);

/* ---- N4: `grav1synth estimate` (feature "unstable", src/main.rs:534-608): the single-source noise estimator ---- */
/* av1_grain::estimate_plane_noise(&frame.y_plane, bit_depth) per frame (the port of libaom's
 * av1_estimate_noise_from_single_plane: Sobel-gated mean |Laplacian| of the luma plane), on the device: one pass over
 * the luma plane, exact integer sums, the f64 formed on the host with the reference's three operations.
 * g1s_estimate_new: NULL without a HIP device (no CPU fallback) or for a bit depth outside 8..16. */
typedef struct g1s_estimate g1s_estimate_t;
g1s_estimate_t *g1s_estimate_new(uint32_t bit_depth, int32_t device, uint32_t batch_frames);
/* One frame (only data[0], the luma plane, is read; on_device 0 = host, copied before the call returns; 1 = device,
 * valid until the next g1s_estimate_finish or until batch_frames more frames have been handed over). */
int g1s_estimate_frame(g1s_estimate_t *, const g1s_frame_t *frame);
/* frame_estimates (src/main.rs:563-590): one f64 per frame, -1.0 where the reference has None (fewer than 16 smooth
 * pixels).  G1S_ERR_CAPACITY leaves them in place (*n_out = count); more frames may follow. */
int g1s_estimate_finish(g1s_estimate_t *, double *out, size_t cap, size_t *n_out);
/* HIP-event time of the kernel launches so far (enable = 1 from the next batch on). */
int g1s_estimate_set_timing(g1s_estimate_t *, int enable, double *ms_kernel, uint64_t *frames);
/* What the last batch's launch was cut into, and the integers behind the estimates (a test and measurement aid).  Depths up to
 * 12 bits take the packed kernel, whose strip height is chosen per launch from the plane, the batch, the device's compute
 * units and the kernel's occupancy (csrc/estimate_plan.h), or given by G1S_ESTIMATE_ROWS=N (clamped into 8 .. 256); deeper
 * samples and G1S_ESTIMATE=wide take the 32-bit kernel and strips of 32 rows. */
typedef struct {
  uint32_t strip_rows;  /* output rows a wave strip */
  uint32_t row_strips;  /* strips down a plane */
  int32_t packed;       /* 1: the packed kernel */
  int32_t launched;     /* 0: the plane has no interior pixel, nothing ran */
  int32_t cus;          /* what the plan was given: compute units and workgroups of the kernel a unit as the occupancy query */
  int32_t wgs_per_cu;   /* answered (below 1: the plan took its fallback); both 0 for the 32-bit kernel */
} g1s_estimate_launch_t;
/* *launch (may be NULL): the last batch that held a frame.  sums: accum and count of every frame g1s_estimate_finish has an
 * estimate for, in its order, two words a frame, from the same words the estimates were formed from; *n_out = the frames.
 * sums NULL with cap 0: the launch alone.  Too small a cap: G1S_ERR_CAPACITY.  Frames still queued are not launched. */
int g1s_estimate_last_launch(g1s_estimate_t *, g1s_estimate_launch_t *launch, uint64_t *sums, size_t cap, size_t *n_out);
const char *g1s_estimate_last_error(const g1s_estimate_t *);
void g1s_estimate_free(g1s_estimate_t *);
/* The command's output (src/main.rs:596-603): "filmgrn1\n" then "{:.3}\n" per frame.  Bytes written or G1S_ERR_CAPACITY. */
long g1s_format_estimates(const double *estimates, size_t n, char *buf, size_t cap);

/* ---- noise levels, rules N1 - N8: how much noise a single clip has at each intensity, per plane ----
 * The estimator above folds a luma plane into one number.  A noise level function keeps its stencil and its gate and sums per
 * intensity bin and per plane, so that one clip alone says what `denoise` otherwise has to be told: the shape of the grain
 * over intensity (a prior's curve, rules 12 - 13 of `denoise`) and its size (the strength h).  Everything is integer except
 * where a rule says otherwise.  A frame has bit depth B in {8, 10, 12}, one plane or three (xdec <= 1, ydec <= xdec);
 * sh = B - 8, half = sh ? 1 << (sh - 1) : 0.  Plane c has size pw x ph and samples u; its INTERIOR is 1 <= x <= pw - 2,
 * 1 <= y <= ph - 2, empty when either side is shorter than 3.
 *  N1. Stencil.  At an interior p with 3 x 3 neighbourhood m_ij (row i, column j): Gx = (m00 - m02) + (m20 - m22) +
 *      2 (m10 - m12), Gy = (m00 - m20) + (m02 - m22) + 2 (m01 - m21), L = 4 m11 - 2 (m01 + m21 + m10 + m12) + (m00 + m02 +
 *      m20 + m22), all at full bit depth: the estimator's.  p COUNTS iff (|Gx| + |Gy| + half) >> sh < 50.
 *  N2. Intensity, 32 bins.  Luma: S9(p) = the plain sum of the nine samples, k(p) = floor(S9 / (9 2^(B - 5))).  The box sum
 *      is orthogonal to the Laplacian mask (the mask's weights sum to zero), so binning by it does not select on the noise
 *      being measured; binning by the sample itself would.  Chroma: rule 2 of `measure` on the frame's own luma: averageLuma
 *      at (xs, ys) = (x << xdec, y << ydec), (Y(xs, ys) + Y(min(xs + 1, W - 1), ys) + 1) >> 1 if xdec, else Y(xs, ys); then
 *      >> (B - 5).
 *  N3. Sums.  Per plane and bin, over the counting p: n[k] the count (u64), a[k] = sum of (|L| + half) >> sh (u64: the
 *      estimator's term), q[k] = sum of L^2 (u64).  |L| <= 8 (2^B - 1) (the centre and the corners against the four
 *      neighbours: a checkerboard of 0 and 2^B - 1 reaches it and passes the gate), so one L^2 reaches 32760^2 =
 *      1 073 217 600: four fit u32 and five do not.  Everything is exact for the largest frame the checks admit
 *      (65536 x 65536: below 2^32 samples of less than 2^31 each).
 *  N4. Record.  g1s_nlf_record_t, zeros for the planes a frame lacks.  A clip's record is the checked 64-bit sum of its
 *      frames' (g1s_nlf_sum): an overflow is a refusal.  Identity: sum_k n[0][k] and sum_k a[0][k] are the estimator's two
 *      sums of the frame, so a / (6 n) sqrt(pi / 2), formed with the same three operations, is g1s_estimate_finish's f64
 *      bit for bit.
 *  N5. Levels.  For a bin with n >= Nmin (min_count; 0 = 4096): t[k] = isqrt(floor(2^16 q[k] / (36 n[k]))), the product
 *      formed in 128 bits.  The mask's squared weights sum to 36, so t = 256 sigma for white noise.
 *  N6. Prior.  No valid luma bin: refused ("no luma bin has enough smooth samples for a prior").  Else, tmax the largest
 *      valid t: y[k] = max(1, floor(255 t[k] / max(tmax, 1))); bin centres c_k = (k << (B - 5)) + (1 << (B - 6)); s(v),
 *      v = 0 .. 2^B - 1: at or below the first valid centre that bin's y, at or above the last valid centre that bin's y,
 *      between adjacent valid centres c_i < c_j: y_i + floor(((y_j - y_i)(v - c_i) 2 + (c_j - c_i)) / (2 (c_j - c_i))),
 *      floor towards minus infinity.  s lies in 1 .. 255, the domain rule 12 of `denoise` already has; the curve is rule 12
 *      from "floor = ..." onwards and rule 13 on this s unchanged (g1s_denoise_curve_sigma), so their proofs hold as they
 *      stand.  A 12-bit clip is refused with rule 12's text.
 *  N7. Strength.  h_luma = sqrt(2 Q / (36 N)) / 2^(B - 8), Q and N the q and n of plane 0 summed over all bins, taken as f64
 *      from the exact integers (2 Q and 36 N are formed in f64).  Rule 3 of `denoise` gives a patch that differs only by
 *      noise an expected weight of exp(-2 sigma^2 / h^2); h = sqrt(2) sigma puts it at 1/e: that is the derivation, there is
 *      no tuning constant.  h_chroma: the same over planes 1 and 2 pooled.  Refused when N < Nmin or the result is outside
 *      rule 3's 0 < h <= 1000.  Under a curve rule 14 makes h the strength at the curve's mean slope.
 *  N8. Report.  g1s_format_noise_levels writes plain text; the grammar is at its declaration.
 *  N9. Chroma prior (rule 23 of `denoise`).  Planes 1 and 2 pooled per bin: n = n[1][k] + n[2][k], q = q[1][k] + q[2][k];
 *      t[k] by N5 with the same Nmin.  No valid bin: refused ("no chroma bin has enough smooth samples for a prior").  y[k]
 *      and the interpolation exactly as in N6 with B = 8 -- centres c_k = 8 k + 4, v = 0 .. 255 -- whatever the clip's depth:
 *      the bins are bins of averageLuma's top five bits.  A 12-bit clip is fine here: a gain needs no headroom.
 * The gate is the estimator's and has its bias: above about sigma = 5 eight-bit code values it thins the sample and keeps
 * the quieter part.  In a numpy run of N1 - N3 on a noisy ramp it kept 64 % of the samples at sigma = 8, and the per-bin
 * sigma stayed within 2.3 % of the truth.  The gate is not corrected for.
 * Frames queue up to batch_frames (0 = 32; at most 256) and go out as one kernel launch per plane class (luma; the two chroma
 * planes) and a small summing launch, on the meter's own stream.  Errors are sticky (g1s_nlf_last_error). */
typedef struct {
  uint64_t n[3][32];
  uint64_t a[3][32];
  uint64_t q[3][32];
} g1s_nlf_record_t;
typedef struct {
  uint32_t struct_size; /* sizeof(g1s_nlf_opts_t) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  uint32_t batch_frames;
} g1s_nlf_opts_t;
typedef struct g1s_nlf g1s_nlf_t;
/* bit_depth 8, 10 or 12.  NULL on failure, the reason from g1s_last_global_error() ("no HIP device available: noise levels
 * has no CPU fallback" without a device).  opts == NULL: current device, defaults. */
g1s_nlf_t *g1s_nlf_new(uint32_t bit_depth, const g1s_nlf_opts_t *opts);
/* One frame, only read.  on_device: 0 = host (copied before the call returns), 1 = device, 2 = pinned host (the copy is
 * queued).  Device and pinned planes must stay valid and unmodified until the batch they are in has gone out: batch_frames
 * frames later, or at g1s_nlf_finish.  A frame whose geometry differs from the one before it sends the queue out first. */
int g1s_nlf_frame(g1s_nlf_t *, const g1s_frame_t *frame);
/* Launches what is queued, waits, and hands over one record per frame since the last hand-over, in order.  cap too small
 * (or per_frame NULL): G1S_ERR_CAPACITY, *n_out = the count, the records stay (the error is not sticky). */
int g1s_nlf_finish(g1s_nlf_t *, g1s_nlf_record_t *per_frame, size_t cap, size_t *n_out);
/* HIP-event time of the luma and of the chroma launches so far, milliseconds, and the frames they covered (enable = 1:
 * timed from the next batch on).  tools/bench_estimate.py --levels. */
int g1s_nlf_set_timing(g1s_nlf_t *, int enable, double *ms_luma, double *ms_chroma, uint64_t *frames);
const char *g1s_nlf_last_error(const g1s_nlf_t *);
void g1s_nlf_free(g1s_nlf_t *);
/* The five below are host only: they need no device. */
/* N4: *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_nlf_sum(const g1s_nlf_record_t *recs, size_t n, g1s_nlf_record_t *total);
/* N5 - N6: s[1 << bit_depth] from the luma bins of a clip's record.  G1S_ERR_INVALID with the reason from
 * g1s_last_global_error(): a bit depth other than 8 and 10 (rule 12's texts), no valid luma bin. */
int g1s_nlf_sigma(const g1s_nlf_record_t *total, uint32_t bit_depth, uint64_t min_count, uint8_t *s);
/* N7 for one plane class (0: luma; 1: the two chroma planes pooled): *h.  G1S_ERR_INVALID with the reason from
 * g1s_last_global_error() ("too few smooth samples for a strength", "the measured strength is outside 0 < h <= 1000"). */
int g1s_nlf_strength(const g1s_nlf_record_t *total, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h);
/* N9: s[256] from the chroma bins of a clip's record, whatever its bit depth.  G1S_ERR_INVALID with the reason from
 * g1s_last_global_error() when no chroma bin is valid. */
int g1s_nlf_chroma_sigma(const g1s_nlf_record_t *total, uint64_t min_count, uint8_t s[256]);
/* Rule 12 from "floor = ..." onwards and rule 13 on a given s[1 << bit_depth] (N6's, or any other): the pair (f, g) as
 * g1s_denoise_curve makes it from a table's s.  The same refusals for bit depth and range. */
int g1s_denoise_curve_sigma(const uint8_t *s, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv);
/* N8: the report of a clip's record of `frames` frames.  Every value is formed in f64 from the exact integers in the order
 * written here and printed "%.4f", in code values of the clip's depth.  Grammar:
 *   noiselevels1
 *   frames N bit_depth B planes P
 *   plane c                          for c in 0 .. P - 1
 *   bin k n sigma_q sigma_a          the bins with n > 0: sigma_q = sqrt((double)q / (double)(36 n)),
 *                                    sigma_a = (double)a / (double)(6 n) * sqrt(pi / 2) * 2^(B - 8)
 *   plane_sigma v                    sigma_q of the plane's bins summed; "-" when no sample counts
 *   auto_strength h_luma h_chroma    after the planes: N7's two values, each "-" where N7 refuses
 * Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a bit depth or plane count the rules do not have). */
long g1s_format_noise_levels(const g1s_nlf_record_t *total, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, uint64_t min_count, char *buf,
                             size_t cap);
/* `estimate SOURCE --levels PATH` for a .y4m file: the first max_frames frames (0 = all), the clip's record into *total
 * (may be NULL), the report into out_report (may be NULL).  Returns the number of frames, or a negative G1S_ERR_* with the
 * reason in err. */
int64_t g1s_nlf_y4m_file(const char *source, const char *out_report, const g1s_nlf_opts_t *opts, uint64_t max_frames, g1s_nlf_record_t *total,
                         char *err, size_t cap);

/* ---- temporal noise levels, rules T1 - T8: the noise of a clip from the difference of consecutive frames ----
 * N5 says what the 3 x 3 mask assumes: white noise.  Film grain is not white, and on correlated grain the mask sees only the
 * part of the grain's power at the highest frequencies: in a numpy run of N1, N3 and N7 on a 200 x 200 10-bit picture under
 * Gaussian grain of sigma 16 it read 16.1 for white grain, 3.8 for 3 x 3 box-filtered and 2.5 for 5 x 5 box-filtered grain.
 * Grain is independent from frame to frame and picture content is not: where the picture stands still, the difference of
 * two consecutive frames has variance 2 sigma^2 whatever the grain's spatial correlation.  A meter made temporal
 * (g1s_nlf_new_temporal) keeps its ordinary records, byte for byte, and adds for every frame of a run but the first a
 * temporal record against the frame before.  A RUN is the sequence of frames given to one temporal meter with one geometry;
 * a change of geometry or g1s_nlf_cut ends it.  Frame t of a run, t >= 1, has a temporal record against frame t - 1.  B, sh,
 * half, the planes, the INTERIOR and the stencils are those of N1 - N2.  Everything is integer except where a rule says
 * otherwise.  For plane c with samples u_t and u_(t-1):
 *  T1. Difference.  e(p) = u_t(p) - u_(t-1)(p), signed, |e| < 2^B.
 *  T2. Gate.  An interior p COUNTS iff N1's gate passes at p in frame t, N1's gate passes at p in frame t - 1, and
 *      |S9_t(p) - S9_(t-1)(p)| < 144 2^sh, S9 the plain sum of the plane's own nine samples around p (luma and chroma
 *      alike).  The first two exclude edges, where any motion shows; the third excludes what moved or changed anyway.  144 is
 *      9 x 16: a box mean that moved by 16 eight-bit code values; for white grain of sigma 8 that is 4.2 standard deviations
 *      of the box-mean difference.
 *  T3. Bins, 32, symmetric in the two frames so that a bin does not select on one frame's noise.  Luma:
 *      k = floor((S9_t + S9_(t-1)) / (18 2^(B - 5))).  Chroma: a_t and a_(t-1) N2's averageLuma at p, each from its own
 *      frame's luma; k = (a_t + a_(t-1)) >> (B - 4).
 *  T4. Sums.  Per plane and bin, over the counting p: n[k] (u64), s[k] = sum of e (i64), q[k] = sum of e^2 (u64).  One e^2 is
 *      below 2^24; a plane of 65536 x 65536 keeps q below 2^56.
 *  T5. Record.  g1s_nlf_trecord_t, zeros for the planes a frame lacks.  A clip's temporal record is the checked 64-bit sum
 *      of its pairs' records (g1s_nlf_sum_temporal; s as a signed sum): an overflow is a refusal.
 *  T6. Levels.  For a bin with n >= Nmin: t_T[k] = isqrt(floor(2^16 (n q - s^2) / (2 n^2))), the products formed in 128 bits
 *      (n q - s^2 >= 0 for sums of integers; the quotient is taken as floor(floor(2^15 (n q - s^2) / n) / n), the same number,
 *      which leaves 128 bits for no u64 sums).  That is 256 sigma with the bin's mean difference removed, so that a fade or a
 *      flicker is not read as grain.
 *  T7. Prior and strength.  N6 and N9 on t_T in the place of t, unchanged otherwise: the same refusals, the same texts (N9
 *      pools n, s and q of planes 1 and 2 per bin; a pooled sum that leaves 64 bits is refused with T5's text).  h_luma =
 *      sqrt(max(Q / N - (S / N)^2, 0)) / 2^(B - 8), N, S, Q plane 0's sums over all bins; the two quotients are formed in f64
 *      from the exact integers, in that order.  This is sqrt(2) sigma, since the variance of e is 2 sigma^2.  h_chroma: the
 *      same over planes 1 and 2 pooled.  N7's refusals apply.
 *  T8. Report.  g1s_format_noise_levels_temporal writes plain text; the grammar is at its declaration.
 * The gate is not tuned and not corrected for.  In a numpy run on the still picture above the estimate read 6.03 / 6.03 / 5.96
 * at sigma 6 (white, 3 x 3 box, 5 x 5 box), 16.05 / 15.72 / 16.09 at sigma 16 and 31.9 / 29.0 / 26.9 at sigma 32: from about
 * 8 eight-bit code values on T2's box condition cuts tails, minus 10 to 16 % on correlated grain.  Motion biases sigma_t
 * upwards and is not compensated: on a pan of 2 samples a frame over that picture it read 9.6 at sigma 6 and 17.6 at sigma
 * 16.  The vectors kd_motion finds are not used.  So N's estimate is a lower bound and T's an upper bound; they meet on
 * white grain over a still picture.  Their ratio is reported (T8); no verdict is drawn from it, and choosing coarse levels
 * from it is not part of this.  All of these are numpy runs on synthetic content.
 * The predecessor of a batch's first frame is the last frame of the batch before.  Host and pinned frames are on the device
 * already; of a device frame the meter keeps a copy when it is a batch's last, so the planes of a device frame stay the
 * caller's to keep valid no longer than g1s_nlf_frame says. */
typedef struct {
  uint64_t n[3][32];
  int64_t s[3][32];
  uint64_t q[3][32];
} g1s_nlf_trecord_t;
/* g1s_nlf_new for a temporal meter: g1s_nlf_frame and g1s_nlf_finish as before, and the temporal records beside. */
g1s_nlf_t *g1s_nlf_new_temporal(uint32_t bit_depth, const g1s_nlf_opts_t *opts);
/* Ends the run: the next frame has no predecessor.  Waits for nothing; what is queued stays queued.  On a meter made by
 * g1s_nlf_new it does nothing. */
int g1s_nlf_cut(g1s_nlf_t *);
/* g1s_nlf_finish for the temporal records: one per frame with a predecessor since the last hand-over, in order.  The
 * ordinary records stay for g1s_nlf_finish.  Capacity as there.  On a meter made by g1s_nlf_new: G1S_ERR_INVALID, "not a
 * temporal meter: make it with g1s_nlf_new_temporal" (not sticky). */
int g1s_nlf_finish_temporal(g1s_nlf_t *, g1s_nlf_trecord_t *per_pair, size_t cap, size_t *n_out);
/* HIP-event time of the temporal luma and chroma launches so far, milliseconds, and the pairs they covered; timed while
 * g1s_nlf_set_timing has it enabled.  tools/bench_estimate.py --levels-temporal. */
int g1s_nlf_temporal_times(g1s_nlf_t *, double *ms_luma, double *ms_chroma, uint64_t *pairs);
/* The five below are host only: they need no device. */
/* T5: *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_nlf_sum_temporal(const g1s_nlf_trecord_t *recs, size_t n, g1s_nlf_trecord_t *total);
/* T6 - T7: g1s_nlf_sigma, g1s_nlf_chroma_sigma and g1s_nlf_strength on a clip's temporal record: the same outputs, the same
 * refusals. */
int g1s_nlf_sigma_temporal(const g1s_nlf_trecord_t *total, uint32_t bit_depth, uint64_t min_count, uint8_t *s);
int g1s_nlf_chroma_sigma_temporal(const g1s_nlf_trecord_t *total, uint64_t min_count, uint8_t s[256]);
int g1s_nlf_strength_temporal(const g1s_nlf_trecord_t *total, uint32_t bit_depth, uint64_t min_count, uint32_t plane_class, double *h);
/* T8: the report of a clip's temporal record of `pairs` pairs.  `ordinary` (may be NULL) is the ordinary record of the same
 * frames: those with a predecessor, of the same runs.  Values as in N8: f64 from the exact integers in the order written,
 * "%.4f", code values of the clip's depth; "-" where a value is undefined.  Grammar:
 *   noiselevels_t1
 *   pairs N bit_depth B planes P
 *   plane c                          for c in 0 .. P - 1
 *   bin k n sigma_t                  the bins with n > 0: sigma_t = sqrt(max(((double)q / n - ((double)s / n)^2) / 2, 0))
 *   plane_sigma_t v                  sigma_t of the plane's bins summed; "-" when no sample counts
 *   ratio v                          plane_sigma_t over N8's plane_sigma of `ordinary`; "-" when either is undefined, when
 *                                    plane_sigma is zero or without `ordinary`
 *   auto_strength_t h_luma h_chroma  after the planes: T7's two values, each "-" where N7's refusals apply
 * Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a bit depth or plane count the rules do not have). */
long g1s_format_noise_levels_temporal(const g1s_nlf_trecord_t *total, const g1s_nlf_record_t *ordinary, uint64_t pairs, uint32_t bit_depth,
                                      uint32_t nplanes, uint64_t min_count, char *buf, size_t cap);
/* g1s_nlf_y4m_file with a temporal meter, the file one run: out_report and *total as there (all frames), the temporal report
 * into out_treport (may be NULL; its ratio from the ordinary record of the frames after the first), the clip's temporal
 * record into *ttotal (may be NULL).  A clip of one frame has no pair: a report of "-".  `estimate SOURCE --levels-temporal
 * PATH`. */
int64_t g1s_nlf_y4m_file_temporal(const char *source, const char *out_report, const char *out_treport, const g1s_nlf_opts_t *opts, uint64_t max_frames,
                                  g1s_nlf_record_t *total, g1s_nlf_trecord_t *ttotal, char *err, size_t cap);

/* ---- lagged noise levels, rules L1 - L10: the lagged products of a clip's frame differences ----
 * T1 - T8 give the grain's size per intensity: a table's scaling function.  The other half of a table, its AR
 * coefficients, is in the same difference: where the picture stands still e is grain and only grain, and the covariance of
 * e(p) and e(p + d) is twice the grain's at lag d.  A meter made for lags (g1s_nlf_new_lags) is a temporal meter -- its
 * ordinary and temporal records are those of g1s_nlf_new_temporal byte for byte -- that adds for every pair of a run a lag
 * record: the sums from which the covariances at every lag an AR fit of lag 1 .. 3 needs are formed, and for chroma those
 * against the luma difference under it.  No denoiser is involved.  B, sh, the planes, the INTERIOR, T1's e and T2's gate are
 * as they stand.  Everything is integer.  For plane c of size pw x ph:
 *  L1. Gate bit.  g_c(p) = 1 iff p is interior and COUNTS by T2, else 0.  It is 0 outside the plane.
 *  L2. Lags.  46 offsets d_i = (dx, dy): dy = 0, dx = 0 .. 6 (i = 0 .. 6); dy = 1, 2, 3, dx = -6 .. 6
 *      (i = 7 + 13 (dy - 1) + dx + 6).  These are the differences of two members of {the causal lag-3 neighbourhood,
 *      (0, 0)}, one of each +- pair.
 *  L3. Sums.  n[i] = the number of p with g(p) g(p + d_i) = 1 (u64), r[i] = the sum of e(p) e(p + d_i) over them (i64),
 *      s = the sum of e(p) over g(p) = 1 (i64).  Pairs with an end outside the plane do not exist: skipped, not clamped.
 *      One product is below 2^24, so a 65536 x 65536 plane stays below 2^56.  With the temporal record of the same pair:
 *      n[0] = sum_k n_T[c][k], r[0] = sum_k q_T[c][k], s = sum_k s_T[c][k].
 *  L4. Luma under chroma, for a frame of three planes.  Lbar(p), p on the chroma grid, is rule 12 of `measure` (the
 *      specification's box, Round2 with an arithmetic shift, the clamp) on the luma difference e_0 -- e_0 itself, gated or
 *      not.  gL(p) = 1 iff g_0 = 1 at every luma sample of that box, at the clamped coordinates.  delta_j are rule 4 of
 *      `measure`'s 25 offsets: the 24 causal ones in the table's coefficient order, (0, 0) at index 24.  For c = 1, 2:
 *      xn[c - 1][j] = the number of p with gL(p) g_c(p + delta_j) = 1, xr[c - 1][j] = the sum of Lbar(p) e_c(p + delta_j)
 *      over them (i64); p and p + delta_j on the chroma grid, skipped where either is outside.  Once per frame, over the
 *      chroma grid: ln = the number of p with gL(p) = 1, ls = the sum of Lbar over them (i64), l2 = the sum of Lbar^2
 *      (u64).  At 4:4:4 Lbar = e_0 and gL = g_0.  A frame of one plane has zeros here.  The clamp bears on no record: a box
 *      that needs it holds a sample of the luma plane's last column or row, which is not interior, so gL = 0 there whatever
 *      Lbar is; it is stated so that Lbar is defined at every p.
 *  L5. Record.  g1s_nlf_lrecord_t, zeros for the planes a frame lacks.  A clip's record is the checked 64-bit sum of its
 *      pairs' (g1s_nlf_sum_lags; r, s, xr and ls as signed sums): an overflow is a refusal, as in T5.
 * The gate's bias is T2's and is not corrected: in a numpy run on a 240 x 320 10-bit ramp under lag-3 AR grain (taps 0.45 /
 * 0.40 / -0.15 / ...) a Yule-Walker fit on these sums returned the 24 coefficients within 0.011 at sigma = 8 code values
 * (the gate kept 99 %; ungated: 0.012), and under a pan of 2 samples a frame still within 0.011 where the ungated fit was off
 * by 0.235; at sigma = 24 the gate kept 49 % and cut tails: the large taps read 0.40 / 0.36 for 0.45 / 0.40.  Motion is
 * gated, not compensated; the vectors kd_motion finds are not used.  These are numpy runs on synthetic content; nothing here
 * has been run on real footage.
 * The two lag launches (luma; both chroma planes) of a batch's pairs follow k_nlf_t's on the meter's stream. */
typedef struct {
  uint64_t n[3][46];
  int64_t r[3][46];
  int64_t s[3];
  uint64_t xn[2][25];
  int64_t xr[2][25];
  uint64_t ln;
  int64_t ls;
  uint64_t l2;
} g1s_nlf_lrecord_t;
/* g1s_nlf_new_temporal for a lag meter: everything a temporal meter does, and the lag records beside.  Capacity, stickiness,
 * g1s_nlf_cut, the copy of the frame before and the lifetime rules are the temporal meter's. */
g1s_nlf_t *g1s_nlf_new_lags(uint32_t bit_depth, const g1s_nlf_opts_t *opts);
/* g1s_nlf_finish for the lag records: one per frame with a predecessor since the last hand-over, in order.  The ordinary and
 * temporal records stay for their own calls.  Capacity as there.  On a meter made otherwise: G1S_ERR_INVALID, "not a lag
 * meter: make it with g1s_nlf_new_lags" (not sticky). */
int g1s_nlf_finish_lags(g1s_nlf_t *, g1s_nlf_lrecord_t *per_pair, size_t cap, size_t *n_out);
/* HIP-event time of the luma and chroma lag launches so far, milliseconds, and the pairs they covered; timed while
 * g1s_nlf_set_timing has it enabled.  tools/bench_estimate.py --lags. */
int g1s_nlf_lag_times(g1s_nlf_t *, double *ms_luma, double *ms_chroma, uint64_t *pairs);
/* Host only.  L5: *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_nlf_sum_lags(const g1s_nlf_lrecord_t *recs, size_t n, g1s_nlf_lrecord_t *total);
/* Host only.  Rules L6 - L7: the AR coefficients of one plane from a clip's lag record, before quantisation.
 *  L6. Covariances, f64 from the exact integers in the order written.  m = (double)s / n[0]; C(d_i) = (double)r[i] / n[i] -
 *      m m, and C(-d) = C(d); mL = ls / ln, VL = l2 / ln - mL^2; X(delta_j) = xr[j] / xn[j] - mL m.  Nmin is min_count, 0 = 4096.
 *      Refused with "too few static sample pairs for a table" when n of any lag the chosen `lag` needs is below Nmin; on a
 *      chroma plane the same holds for xn and ln.
 *  L7. AR system for lag L in 1 .. 3; o_1 .. o_m the table's causal offsets (dy = -L .. 0, dx = -L .. L, raster, stopping before
 *      (0, 0)), m = 2 L (L + 1).  Luma: N = n[0], A[i][j] = N C(o_i - o_j), b[i] = N C(o_i).  Chroma adds row and column m:
 *      A[i][m] = A[m][i] = N X(o_i), A[m][m] = N VL, b[m] = N X((0, 0)).  Every entry is divided by 4^(B - 8) 255^2: the fold
 *      (`diff`) forms its normal equations from eight-bit code values over 255, and its solver's thresholds are in those
 *      units.  Solved by the fold's own elimination, with its gain (the square root of the variance over the innovation's) and,
 *      for a singular chroma system, its fallback: zero coefficients and the luma coefficient b[m] / A[m][m].  A singular luma
 *      system is refused with the fold's text.
 * x[0 .. m) are the coefficients in the table's order, x[m] on a chroma plane the luma coefficient, the rest zeros; *gain the
 * fold's gain.  xdec and ydec are checked and otherwise unused (Lbar is a mean already).  G1S_ERR_INVALID with the reason from
 * g1s_last_global_error().  The fit divides out what the gate does to the scale and keeps what it does to the shape: see the
 * bias stated above. */
int g1s_nlf_ar(const g1s_nlf_lrecord_t *ltotal, uint32_t plane, uint32_t bit_depth, uint32_t xdec, uint32_t ydec, uint32_t lag, uint64_t min_count,
               double x[25], double *gain);
/* Host only.  Rules L8 - L9: a table's segment from a clip's temporal record (the scaling functions) and its lag record (the AR
 * coefficients): a grain table from the clip alone, no denoiser involved.
 *  L8. Strength.  Per plane, for every bin k of the temporal record with n >= Nmin, in ascending k, one measurement goes into
 *      the fold's strength solver: N6's bin centre in eight-bit code values (8 k + 4) and the bin's standard deviation,
 *      sqrt(T6's variance of e / 2) / 2^(B - 8), divided by the plane's gain exactly as the fold's per-frame half does: luma
 *      sqrt(v) / gain; chroma sqrt(max(v / 16, v - (x[m] g_0 y(8 k + 4))^2)) / gain, x[m] the plane's luma coefficient, g_0 the
 *      luma gain and y the luma curve just solved.  No valid luma bin: N6's refusal.  A chroma plane without a valid bin gets
 *      no points.
 *  L9. Segment.  The three states go through the fold's own quantisation (the function `diff` ends a segment with): one
 *      segment [0, INT64_MAX), the default seed, overlap_flag 1 and the fold's other constants, as a `diff` table has them.
 * nplanes 1 or 3; lag 1 .. 3; min_count as in L6.  G1S_ERR_INVALID with the reason from g1s_last_global_error(): L6's and L7's
 * refusals, N6's, "Solving latest noise strength failed!".  Closure, measured on the CPU (tests/test_nlf_lags_cpu.py,
 * profiles/noise_lags.txt): the table made from five 256 x 192 frames of a lag-3 table's rendered grain, rendered again onto flat
 * grey, has the original's sigma within 1.2 % / 0.7 % / 3.9 % (Y / Cb / Cr). */
int g1s_nlf_table(const g1s_nlf_trecord_t *ttotal, const g1s_nlf_lrecord_t *ltotal, uint32_t bit_depth, uint32_t xdec, uint32_t ydec,
                  uint32_t nplanes, uint32_t lag, uint64_t min_count, g1s_segment_t *out);
/* Host only.  Rule L10: the report of a clip's lag record of `pairs` pairs at lag L.  Every value is formed in f64 from the exact
 * integers in the order written and printed "%.4f"; "-" where L6 refuses.  Grammar:
 *   noiselags1
 *   pairs N bit_depth B planes P lag L
 *   plane c                           for c in 0 .. P - 1
 *   n0 n sigma_t v gain g             n = n[c][0]; v = sqrt(max(C(0), 0) / 2), code values of the clip's depth, "-" when n < Nmin;
 *                                     g the fit's gain, "-" when L6 or L7 refuses the plane's fit at lag L
 *   rho i dx dy v                     the causal offsets o_i = (dx, dy), i = 0 .. m - 1: v = C(o_i) / C(0); "-" when n[c][0] or the
 *                                     lag's n is below Nmin or C(0) <= 0
 *   coef i v                          i = 0 .. m - 1: the solved coefficients (L7), all "-" when the fit is refused
 *   luma v                            planes 1 and 2 only: the luma coefficient, "-" when the fit is refused
 * Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a bit depth, plane count or lag the rules do not have). */
long g1s_format_noise_lags(const g1s_nlf_lrecord_t *ltotal, uint64_t pairs, uint32_t bit_depth, uint32_t nplanes, uint32_t lag, uint64_t min_count,
                           char *buf, size_t cap);
/* `estimate SOURCE --table PATH` for a .y4m file through a lag meter, the file one run: the first max_frames frames (0 = all).
 * The table (g1s_nlf_table at `lag`, `min_count`) is made first: a refusal ("a table needs two frames" for a clip of fewer, the
 * host function's otherwise) writes nothing.  Then the .tbl through g1s_format_tbl into out_table, the lag report into out_lags,
 * the noise levels into out_report and the temporal noise levels into out_treport (each may be NULL), the segment into
 * *segment_out (may be NULL).  Returns the number of frames, or a negative G1S_ERR_* with the reason in err. */
int64_t g1s_nlf_y4m_file_table(const char *source, const char *out_table, const char *out_report, const char *out_treport, const char *out_lags,
                               const g1s_nlf_opts_t *opts, uint64_t max_frames, uint32_t lag, uint64_t min_count, g1s_segment_t *segment_out, char *err,
                               size_t cap);

/* ---- `render`: AV1 film grain synthesis on the device (the inverse of `diff`: a table's grain onto frames) ----
 * The film grain synthesis process of the AV1 specification (clause 7.18.3: random number process, generate grain
 * process, scaling lookup initialisation, add noise synthesis process), integer-exact, written from the standard.
 * A g1s_segment_t carries the film grain parameters as a table does: AR coefficients as signed values, ar_coeff_shift
 * (6..9) and scaling_shift (8..11) as the shifts themselves, cb_mult / cb_luma_mult / cb_offset as coded (128, 128 and
 * 256 are subtracted where the standard does).  Scaling points must have strictly increasing values.
 * Frames queue up to batch_frames (0 = 32; at most 256) and go out as two kernel launches per batch on the
 * synthesizer's own stream.  Errors are sticky: after a failure every call returns it (g1s_grain_last_error). */
typedef struct {
  uint32_t struct_size;              /* sizeof(g1s_grain_opts_t) */
  int32_t device;                    /* HIP device ordinal; -1 = current device */
  uint32_t batch_frames;
  uint32_t clip_to_restricted_range; /* the sequence's clip_to_restricted_range: 16..235 (240 chroma) << (bit depth - 8) */
  uint32_t mc_identity;              /* matrix_coefficients == MC_IDENTITY: chroma clips like luma under the flag above */
} g1s_grain_opts_t;
typedef struct g1s_grain g1s_grain_t;
/* bit_depth 8, 10 or 12.  NULL on failure, reason from g1s_last_global_error().  opts == NULL: current device, defaults. */
g1s_grain_t *g1s_grain_new(uint32_t bit_depth, const g1s_grain_opts_t *opts);
/* One frame.  params->random_seed is THE grain_seed of this frame (g1s_tbl_segment_for has already advanced it); the
 * struct is copied.  params == NULL (no segment covers the frame: apply_grain = 0): *out becomes a copy of *in.
 * in / out follow g1s_frame_t.on_device independently: 0 = host (in: copied before the call returns; out: written by
 * g1s_grain_sync at the latest), 1 = device, 2 = pinned host (copies queued).  Device and pinned planes of in must stay
 * valid and unmodified, and every plane of out must stay valid, until g1s_grain_sync.  in and out must be DISTINCT,
 * non-overlapping buffers: a chroma sample is scaled by the co-located INPUT luma, which another workgroup may already
 * have replaced if the kernel wrote in place.  in and out have the same geometry; a frame whose geometry differs from the
 * one before it drains the queue first (the host planes of queued out frames are then complete). */
int g1s_grain_frame(g1s_grain_t *, const g1s_segment_t *params, const g1s_frame_t *in, g1s_frame_t *out);
/* Launches what is queued and waits: the out planes of every frame handed over are complete. */
int g1s_grain_sync(g1s_grain_t *);
/* Stage 1 alone, for tests: the grain templates (luma 73 x 82; cb, cr 38 or 73 rows x 44 or 82 columns by ydec / xdec,
 * row-major, no padding) and the three 256-entry scaling tables for these parameters.  Any output may be NULL. */
int g1s_grain_templates(g1s_grain_t *, const g1s_segment_t *params, uint32_t xdec, uint32_t ydec,
                        int16_t *luma, int16_t *cb, int16_t *cr, uint8_t lut[3][256]);
/* Gaussian_Sequence[2048] of the specification's "Additional tables". */
const int16_t *g1s_grain_gaussian_sequence(void);
/* HIP-event time of the kernels so far, milliseconds, and the frames they covered (enable = 1: timed from the next
 * batch on; a timed batch is waited for).  tools/bench_grain.py. */
int g1s_grain_set_timing(g1s_grain_t *, int enable, double *ms_template, double *ms_apply, uint64_t *frames);
const char *g1s_grain_last_error(const g1s_grain_t *);
void g1s_grain_free(g1s_grain_t *);
/* `render INPUT -g TABLE -o OUTPUT`: every frame of a .y4m through the table's lookup (g1s_parse_tbl,
 * g1s_tbl_segment_for at the frame's presentation time: frame k of a video lies at the time the fold gives a segment
 * that starts with frame k), written as .y4m (the input's header line, "FRAME\n", the planes without padding).
 * Returns the number of frames, or a negative G1S_ERR_* with the reason in err. */
int64_t g1s_grain_y4m_file(const char *in, const char *tbl, const char *out, const g1s_grain_opts_t *opts, char *err, size_t cap);

/* ---- `denoise`: an integer-exact non-local-means filter on the device (the clip `diff` compares the source with) ----
 * This is the project's OWN definition of non-local means: it has the structure of ffmpeg's nlmeans and of KNLMeansCL,
 * not their bits, and its output is not any other tool's.  Every plane is filtered on its own grid (rules 8 - 11 below are
 * the exception, behind a flag).  Bit depth B in
 * {8, 10, 12}, samples u(x, y) of a W x H plane, clamp() replicates the plane's edge samples; search radius A (1..7),
 * patch radius S (1..4), n = (2S + 1)^2, strength h > 0 in 8-bit code values:
 *   1. D(p, d) = sum over |kx|, |ky| <= S of (u(clamp(p + k)) - u(clamp(p + d + k)))^2 for |dx|, |dy| <= A (exact in 32 bits).
 *   2. An offset takes part at p only if p + d lies inside the plane (skipped, not clamped; only patch coordinates
 *      clamp), so D(p, d) = D(p + d, -d) for every pair that takes part.  d = 0 always takes part, with D = 0.
 *   3. w(p, d) = T[min(D >> q, 1023)]: 1024 uint16 entries, T[0] = 4096, non-increasing, T[1023] = 0;
 *      T[i] = round(4096 exp(-((i + 1/2) 2^q) / (n h^2 4^(B - 8)))) for i >= 1, q the smallest shift >= 0 that gives
 *      T[1023] = 0.  g1s_denoise_weights returns the table the kernels use.
 *   4. out(p) = (sum_d w u(p + d) + (sum_d w >> 1)) / sum_d w, integer division (uint32 suffices for A <= 7).
 * The temporal part: with a temporal radius D (0..3; g1s_denoise_new_temporal) the mean of rule 4 also runs over the
 * search windows of the D frames before and the D frames after the frame in hand.  A CLIP is the run of frames handed
 * to one denoiser between two clip ends, numbered t = 0 .. N - 1, all of one geometry; a clip ends at
 * g1s_denoise_sync, at a frame whose geometry differs from the one before it (that frame starts the next clip) and at
 * g1s_denoise_free.  For plane u_t of frame t, with the same A, S, q and T:
 *   5. For k in -D .. D, frame t + k takes part only if 0 <= t + k < N: skipped, not clamped (rule 2's idea in time; a
 *      one-frame clip is filtered as with D = 0).
 *   6. For k != 0: D_k(p, d) = sum over |kx|, |ky| <= S of (u_t(clamp(p + k)) - u_{t+k}(clamp(p + d + k)))^2 for ALL
 *      |dx|, |dy| <= A, d = 0 included (with its real distance, not a forced 0).  (p, d, k) takes part only if p + d
 *      lies inside the plane.  w = T[min(D_k >> q, 1023)]: the same table, no attenuation with |k|.  For k = 0 rules
 *      1 - 3 as they stand.
 *   7. out_t(p) = (sum_{k,d} w u_{t+k}(p + d) + (sum w >> 1)) / sum w, integer division, the sums over everything that
 *      takes part; (k = 0, d = 0) carries 4096 as in rule 4.  sum w <= (2D + 1)(2A + 1)^2 4096 fits 32 bits; the
 *      numerator does not (12 bit, A = 7, D = 1: 1.1e10) and is kept in 64.  Exact for every accepted (B, A, D).
 * D = 0 is rules 1 - 4.
 * Luma-guided joint chroma: with the flag G1S_DENOISE_JOINT_CHROMA (g1s_denoise_new_ex) the two chroma planes of a frame
 * with three planes share one weight, taken from Cb, Cr and the luma at the same place.  Luma is filtered by rules 1 - 7
 * as without the flag; a luma-only frame is filtered as without it.  Chroma size cw x ch, cw = (W + xdec) >> xdec,
 * ch = (H + ydec) >> ydec:
 *   8. The guide G is the frame's INPUT luma Y at chroma resolution, a rounded box mean:
 *      G(x, y) = (sum over j <= ydec, i <= xdec of Y(min((x << xdec) + i, W - 1), min((y << ydec) + j, H - 1))
 *                 + ((1 << (xdec + ydec)) >> 1)) >> (xdec + ydec).  For 4:4:4 G = Y.  The input luma, not the denoised
 *      one: the chroma launch depends on no other launch's output.
 *   9. D_J(p, d) = D_Cb(p, d) + D_Cr(p, d) + D_G(p, d), each term rule 1 on the cw x ch grid with the clamp at the chroma
 *      plane's edges (G is a cw x ch plane).  Rule 2 holds unchanged, so D_J(p, d) = D_J(p + d, -d).  Exact in UNSIGNED
 *      32 bits (3 x 81 x 4095^2 = 4 074 873 075 < 2^32); it does not fit int32.
 *  10. w(p, d) = T_J[min(D_J >> q_J, 1023)]: (T_J, q_J) is rule 3 with n replaced by 3n and h = the chroma strength, the
 *      same rounding and the same non-increasing clamp.  g1s_denoise_weights_ex returns it.
 *  11. out_Cb(p) and out_Cr(p) are each rule 4 with the one shared w.  11t: with a temporal radius rules 5 - 7 hold with D_k
 *      the sum over Cb, Cr and G of rule 6's distance between frame t and frame t + k (G of frame t + k from that
 *      frame's input luma), the same T_J, and both numerators in 64 bits.
 * A grain prior (g1s_denoise_new_curve): luma is filtered in a domain where a grain table's grain has one size at every
 * intensity -- a variance-stabilising curve f in front of rules 1 - 7 and its inverse g behind them.  B in {8, 10},
 * M = 2^B - 1; the stabilised domain is always 12 bits (0 .. 4095):
 *  12. The curve from n >= 1 segments.  s_i(v), v = 0 .. M, is the AV1 specification's scale_lut (7.18.3.5) over the
 *      luma ScalingLut (7.18.3.4) of segment i, s_i = 0 for a segment without luma points;
 *      s(v) = (sum_i s_i(v) + (n >> 1)) / n, the unweighted mean (the last segment's end_time is effectively infinite, so
 *      durations cannot weight it).  Range R in 1 .. 2^(12 - B) (16 at 8 bits, 4 at 10), 0 = min(4, 2^(12 - B)):
 *      floor = max(1, ceil(max_v s(v) / R)), sigma'(v) = max(s(v), floor), r(v) = floor(2^24 / sigma'(v)),
 *      C(x) = sum over v < x of r(v) in 64 bits, f(x) = (4095 C(x) + (C(M) >> 1)) / C(M).  f(0) = 0, f(M) = 4095, and the
 *      bound on R makes every slope at least 1.0006, so f is strictly increasing (the builder checks it: a failure is an
 *      internal error).  R = 1, or a table without luma grain, gives the flat curve.
 *  13. The inverse g(y), y = 0 .. 4095, is the smallest x with |f(x) - y| minimal, so g(f(x)) = x: the algebraic inverse,
 *      no bias correction.
 *  14. Luma: u' = f[min(u, M)]; u' is filtered by rules 1 - 7 as a 12-bit plane with rule 3's table at B = 12 and the luma
 *      strength h (g1s_denoise_weights(12, S, h)) into v; out = g[v].  Where the curve's slope is its mean (about
 *      2^(12 - B)) the strength is h; elsewhere it is h x mean slope / slope(x): proportional to the table's grain, within a
 *      factor R between the weakest and the strongest.
 *  15. Chroma is untouched unless a chroma gain is given (rules 21 - 24): the two chroma planes are filtered, independently or jointly, exactly as without a curve, and
 *      rule 8's guide stays the unstabilised input luma.  A 12-bit clip has no headroom in 12-bit kernels and is refused.
 * With a curve the denoiser keeps (2 batch_frames + 2 D) 12-bit u16 luma planes on the device; the caller's input luma is
 * never written.
 * Motion (g1s_denoise_new_motion): rules 5 - 7 work while the picture stands still to within A; on a pan the neighbour
 * frames hold the right samples further away.  With a motion range Mr (full-resolution samples of the plane, even, 0 .. 64;
 * M = Mr / 2; Mr = 0 is the filter of rules 1 - 15) every tile of the filter gets one integer vector towards every
 * neighbour frame, found by a coarse search, and rule 6 reads the neighbour there.  Integers throughout:
 *  16. The search plane.  For a W x H plane u, u' is w' x h' with w' = (W + 1) >> 1, h' = (H + 1) >> 1; u'(x, y) =
 *      (u(min(2x, W-1), min(2y, H-1)) + u(min(2x+1, W-1), min(2y, H-1)) + u(min(2x, W-1), min(2y+1, H-1)) +
 *      u(min(2x+1, W-1), min(2y+1, H-1)) + 2) >> 2: rule 8's box at xdec = ydec = 1.
 *  17. Motion blocks are the filter's tiles: 64 x 48 samples aligned at the plane's origin, 32 x 24 on the search plane,
 *      ragged at the right and bottom edges.  For frame t, neighbour k != 0, block b and every candidate m' = (mx', my')
 *      with |mx'|, |my'| <= M: SAD(m') = the sum over the block's search-plane samples p' inside w' x h' of
 *      |u'_t(p') - u'_{t+k}(clamp(p' + m'))|, the clamp to the search plane's edges.  Every (t, k) is searched directly,
 *      never by chaining vectors.
 *  18. The vector minimises key = SAD 2^21 + (|mx'| + |my'|) 2^14 + (my' + M) 2^7 + (mx' + M).  SAD <= 768 x 4095 < 2^22
 *      (twice that for rule 20's pair): the key fits 64 bits and is injective -- no ties, and the zero vector wins among
 *      equal SADs.  m_{t,k}(b) = 2 m'.
 *  19. Rule 6 under motion.  For p in block b and m = m_{t,k}(b): D_k(p, d) = sum over |kx|, |ky| <= S of (u_t(clamp(p + k)) -
 *      u_{t+k}(clamp(p + m + d + k)))^2; (p, d, k) takes part only if p + m + d lies inside the plane; the sample averaged
 *      in is u_{t+k}(p + m + d).  Rules 5 and 7, the table, q and the 64-bit numerator are unchanged.
 *  20. Every plane searches on its own samples and its own grid.  Under G1S_DENOISE_JOINT_CHROMA a chroma tile has one
 *      vector for Cb, Cr and the guide: its SAD is the sum of Cb's and Cr's, the guide takes no part in the search, and the
 *      guide of frame t + k is staged at the moved place by rule 8 as it stands.  With a grain prior the luma search runs
 *      on the stabilised 12-bit planes, which are what the filter filters.
 * Sub-tile and sub-sample vectors, smoothing of the vector field and scene-cut detection are not part of it.
 * A chroma gain (g1s_denoise_new_gain): chroma grain is a function of the luma under it -- every table `diff` writes has
 * cb_mult = cr_mult = 128, so its chroma scaling function is indexed by averageLuma alone -- and a curve on the chroma sample
 * cannot follow that.  The strength of the joint chroma filter becomes a strength per pair of samples, read from the guide.
 * Integers throughout:
 *  21. Gain from a scaling function s(i), i = 0 .. 255, values 0 .. 255, and a range R in 1 .. 8 (0 = 4): top = max_i s(i),
 *      floor = max(1, ceil(top / R)), s'(i) = max(s(i), floor), sbar = (sum_i s'(i) + 128) >> 8,
 *      m(i) = min(16384, max(1, (256 sbar^2 + (s'(i)^2 >> 1)) / s'(i)^2)): a Q8 multiplier, kept as uint16.  s' >= top / R and
 *      sbar <= top, so m <= 256 R^2 <= 16384; sbar >= floor >= s' / R, so m >= 256 / R^2 = 4 at R = 8: the clamp only catches
 *      rounding.  R = 1, or a function that is 0 everywhere, gives m = 256 for every i: the FLAT gain.  The strength at a
 *      sample is h s'(i) / sbar: proportional to the grain, and h where the grain has its unweighted mean.
 *  22. s from a table, n >= 1 segments.  For both chroma planes of every segment: the plane's ScalingLut (7.18.3.4; under
 *      chroma_scaling_from_luma the luma points', all zeros for a plane without points) at idx(v), v = 0 .. 255:
 *      idx(v) = v under chroma_scaling_from_luma, else Clip3(0, 255, ((v (luma_mult - 128) + 128 (mult - 128)) >> 6) +
 *      (offset - 256)) with an arithmetic shift -- the 8-bit form of 7.18.3.5 with the chroma sample at mid-grey.
 *      s(v) = (the sum of the 2 n functions + n) / (2 n), the rounded mean.  Exact for tables with mult = 128, which all of
 *      `diff`'s own are (luma_mult = 192, offset = 256: idx(v) = v); otherwise it is the function's section at mid-grey.
 *  23. s from noise levels: rule N9 of "noise levels".
 *  24. The weight under a gain m[256]; it exists only under G1S_DENOISE_JOINT_CHROMA.  v(p) = min(G(p) >> (B - 8), 255) (the
 *      clamp only for samples above the bit depth's maximum, which are the caller's error).  For a pair (p, p'):
 *      mp = (m(v(p)) + m(v(p')) + 1) >> 1, where p' = p + d in the frame itself with G of frame t (rule 9), p' = p + d in a
 *      neighbour frame with G of frame t + k (rule 11t), p' = p + m_{t,k}(b) + d under motion (rule 19).
 *      w = T_J[min((D_J mp) >> (q_J + 8), 1023)], the product formed in 64 bits: D_J < 2^32 and mp <= 2^14, so it stays
 *      below 2^46 < 2^47.  mp is symmetric in the pair, so D(p, d) = D(p + d, -d) still gives one weight for both ends of a
 *      pair.  Rules 2, 5 - 7, 9, 11, 11t and 19 - 20 are otherwise unchanged; (k = 0, d = 0) carries 4096.  With the flat gain
 *      the bytes are those of rules 8 - 11t: (D 256) >> (q + 8) = D >> q.  Luma never sees the gain, and a luma-only frame
 *      is filtered as without it.
 * Coarse levels (g1s_denoise_new_levels): the filter compares patches of at most 9 x 9 samples and assumes white noise; film
 * grain is correlated, so its coarse part stays in the "clean" clip.  With K coarse levels the 2 x 2 box mean of the frame is
 * filtered as well -- grain of twice the size looks there like grain of the original size -- and that result takes the place of
 * the low frequencies of the full-resolution result.  Integers throughout:
 *  25. The coarse frame.  For a frame X with planes u_c of W_c x H_c samples, X' has the planes u'_c = rule 16's box of u_c, the
 *      rounded 2 x 2 mean with the min(.., W-1) clamps, of ((W_c + 1) >> 1) x ((H_c + 1) >> 1) samples, and the same bit depth,
 *      xdec and ydec.  X' is a valid frame of luma size W' = (W + 1) >> 1, H' = (H + 1) >> 1: its chroma width
 *      (W' + xdec) >> xdec equals (cw + 1) >> 1 for cw = (W + xdec) >> xdec (xdec = 0: both are W'; xdec = 1: cw = W', and
 *      (W' + 1) >> 1 on both sides), and likewise its height.
 *  26. Levels.  F_0(X; h, hc, Mr) is the filter of rules 1 - 24 with every option the denoiser was made with.  For K >= 1:
 *      F_K(X; h, hc, Mr) = Merge(F_0(X; h, hc, Mr), F_{K-1}(X'; rho h, rho hc, Mr')), Mr' = 2 ceil(Mr / 4) (64 -> 32 -> 16,
 *      2 -> 2).  The strengths of level l are rho times those of level l - 1, the product formed in double precision level
 *      by level.  A, S, D, the flags, the curve (fwd, inv) and the chroma gain m[256] are the same on every level: both are
 *      indexed by intensity, which the box mean keeps.  The coarse frames of a clip are a clip with the same ends.  On a
 *      coarse level rule 8's guide is made from the coarse frame's input luma, and with a curve the coarse level applies
 *      the curve itself: Merge sees only finished B-bit outputs.
 *  27. Merge, per plane: v the full-resolution output (W x H), c the coarse level's output (W' x H').  d = c - box(v), signed,
 *      with the box of rule 16.  For the fine sample (x, y): xa = x >> 1, xb = clamp(xa + (x & 1 ? 1 : -1), 0, W' - 1), and
 *      ya, yb likewise.  U = (9 d(xa, ya) + 3 d(xb, ya) + 3 d(xa, yb) + d(xb, yb) + 8) >> 4, an arithmetic shift (floor);
 *      out = Clip3(0, 2^B - 1, v + U).  d = 0 gives out = v, and a constant plane stays constant.
 *  28. K = coarse_levels in 0 .. 2; rho = coarse_ratio in 0.0625 .. 4, 0 = 1.0.  The default is 1, not the 1/2 that white
 *      noise would ask for: the grain a coarse level is there for is as strong at the coarse scale as at the fine one.
 *      Every level's strengths must pass rule 3's bounds; the refusal is rule 3's text with "level l " in front.
 *  29. K = 0 is the filter of rules 1 - 24: the same launches, the same bytes.  A ratio given with K = 0 is refused.
 *      g1s_denoise_motion_search is unaffected: it answers for level 0.
 * More than two coarse levels, A or S per level, choosing K from a scales record of `measure`, and a merge fused into the filter
 * kernel are not part of it.  A level keeps (3 batch_frames + 2 D) coarse frames on the device, two thirds of them at the clip's
 * sample size and one third as int16: about (3 batch_frames + 2 D) / 4 frames of memory, and a quarter of that for the level under it.
 * No dithering.  Samples above the bit depth's maximum are the caller's error.
 * Frames queue up to batch_frames (0 = 32; at most 256) and go out as one kernel launch per plane class (luma; the two
 * chroma planes -- under the flag one workgroup filters both) on the denoiser's own stream.  A workgroup's LDS grows
 * with A, S, a temporal radius and the flag; a parameter set that needs more than the device gives a workgroup is
 * refused when the denoiser is made.  Errors are sticky (g1s_denoise_last_error). */
#define G1S_DENOISE_JOINT_CHROMA 1u
typedef struct {
  uint32_t struct_size;    /* sizeof(g1s_denoise_opts_t) */
  int32_t device;          /* HIP device ordinal; -1 = current device */
  uint32_t batch_frames;
  uint32_t search_radius;  /* A: 1..7; 0 = default (3) */
  uint32_t patch_radius;   /* S: 1..4; 0 = default (2) */
  double strength;         /* h, in 8-bit code values, 0 < h <= 1000; 0 = default (4.0) */
  double chroma_strength;  /* the same for the chroma planes; 0 = the luma strength */
} g1s_denoise_opts_t;
typedef struct g1s_denoise g1s_denoise_t;
/* bit_depth 8, 10 or 12.  Parameters out of range and other bit depths are refusals, not clamps: NULL, the reason from
 * g1s_last_global_error() (they are checked before a device is looked for).  opts == NULL: current device, defaults. */
g1s_denoise_t *g1s_denoise_new(uint32_t bit_depth, const g1s_denoise_opts_t *opts);
/* The same with a temporal radius D (rules 5 - 7); g1s_denoise_new is temporal_radius = 0.  A radius above 3 is a
 * refusal like the others ("temporal_radius must be 0..3"). */
g1s_denoise_t *g1s_denoise_new_temporal(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius);
/* The same with flags (G1S_DENOISE_*; rules 8 - 11); g1s_denoise_new_temporal is flags = 0.  An unknown flag bit is a
 * refusal like the others ("unknown denoise flags"), checked before a device is looked for. */
g1s_denoise_t *g1s_denoise_new_ex(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags);
/* The same with a grain prior's curve (rules 12 - 15): fwd[1 << bit_depth] is f, inv[4096] is g, as g1s_denoise_curve
 * makes them (copied before the call returns).  The pair is checked as given -- bit_depth 8 or 10 (12 is refused: no
 * headroom), fwd[0] = 0, fwd[M] = 4095, fwd strictly increasing, inv non-decreasing and at most M, inv[fwd[x]] = x -- and
 * anything else is a refusal with its text, like the others checked before a device is looked for.  Every other
 * g1s_denoise_new* call is the case without a curve. */
g1s_denoise_t *g1s_denoise_new_curve(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                     const uint16_t *fwd, const uint16_t *inv);
/* The same with a motion range (rules 16 - 20).  fwd = inv = NULL: no curve.  motion_range = 0 is g1s_denoise_new_curve
 * (or, without a curve, g1s_denoise_new_ex): the same launches, the same bytes.  Two more refusals, checked before a
 * device is looked for: "motion_range must be even and 0..64" and, for a range above 0 with temporal radius 0,
 * "motion_range needs a temporal radius".  The vectors are found on the denoiser's stream in front of each batch's
 * filter launches (kd_motion) and kept on the device: 2 D pairs of int8 a tile and plane. */
g1s_denoise_t *g1s_denoise_new_motion(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                      const uint16_t *fwd, const uint16_t *inv, uint32_t motion_range);
/* The same with a chroma gain (rules 21 - 24): chroma_gain[256], copied before the call returns, works for 8, 10 and 12 bits,
 * with or without a curve, a temporal radius or motion.  chroma_gain == NULL is g1s_denoise_new_motion: the same launches, the
 * same bytes.  Any table with every entry in 1 .. 16384 is accepted; it need not come from the builders below.  Two more
 * refusals, checked before a device is looked for: "chroma gain must be 1..16384 (at I)" and, without
 * G1S_DENOISE_JOINT_CHROMA, "a chroma gain needs joint chroma" (chroma filtered plane by plane has no guide in hand).
 * g1s_denoise_motion_search is unaffected: the guide takes no part in the search. */
g1s_denoise_t *g1s_denoise_new_gain(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const uint16_t *fwd, const uint16_t *inv, uint32_t motion_range, const uint16_t *chroma_gain);
/* The same with coarse levels (rules 25 - 29).  coarse_levels = 0 (and coarse_ratio = 0) is g1s_denoise_new_gain: the same
 * launches, the same bytes.  Their refusals come after those of the parameters before them and before a device is looked for:
 * "coarse_levels must be 0..2", "coarse_ratio must be 0.0625..4 (0 = 1)", "coarse_ratio needs coarse_levels", and for a level l
 * whose scaled strength leaves rule 3's bounds "level l strength must be greater than 0 and at most 1000" (or "level l
 * chroma_strength ...").  A level is a whole denoiser on the coarse frames, on the same stream; three small kernels (kd_down,
 * kd_lowres, kd_add) stand around it, and the merge works in place on the planes the full-resolution launch wrote. */
g1s_denoise_t *g1s_denoise_new_levels(uint32_t bit_depth, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                      const uint16_t *fwd, const uint16_t *inv, uint32_t motion_range, const uint16_t *chroma_gain,
                                      uint32_t coarse_levels, double coarse_ratio);
/* ms spent by the timed batches so far in kd_down, kd_lowres, kd_add and the coarse levels' own launches (a part of
 * g1s_denoise_set_timing's ms_kernel); 0 for a denoiser without coarse levels. */
int g1s_denoise_level_time(g1s_denoise_t *, double *ms_level);
/* The part of g1s_denoise_level_time spent in kd_down, kd_lowres and kd_add themselves, over every level (the inner levels are
 * timed with the outer one).  tools/bench_denoise.py --levels puts the bytes the three kernels move over it. */
int g1s_denoise_level_kernel_time(g1s_denoise_t *, double *ms_kernels);
/* Rules 22 + 21: the gain from both chroma planes of n >= 1 segments of a grain table, range R (0 = 4).  Host only.
 * G1S_ERR_INVALID (reason from g1s_last_global_error()) for n = 0, a range above 8 ("chroma gain range must be 1..8 (0 = the
 * default)"), and luma or chroma points whose values do not increase. */
int g1s_denoise_chroma_gain(const g1s_segment_t *segs, size_t n, uint32_t range, uint16_t gain[256]);
/* Rule 21 on a given s[256] (N9's, or any other).  Host only.  The same refusal for the range. */
int g1s_denoise_chroma_gain_sigma(const uint8_t s[256], uint32_t range, uint16_t gain[256]);
/* Stage 1 alone (rules 16 - 18, 20), as g1s_grain_templates is for render: the vectors of frame `cur` towards frame `ref`
 * of the same geometry, for a denoiser made with a motion range.  mv[c] takes plane c's vectors as pairs (mx, my) in
 * full-resolution samples of that plane, blocks in raster order; cap_pairs[c] is its capacity in pairs going in and the
 * plane's block count coming out (G1S_ERR_CAPACITY, nothing written, when one is too small).  Under the joint flag planes
 * 1 and 2 carry the same shared vectors.  Frames follow on_device as elsewhere; the call waits for the denoiser's stream
 * and does not touch a clip in progress. */
int g1s_denoise_motion_search(g1s_denoise_t *, const g1s_frame_t *cur, const g1s_frame_t *ref, int16_t *mv[3], size_t cap_pairs[3]);
/* ms spent in kd_motion by the timed batches so far (a part of g1s_denoise_set_timing's ms_kernel). */
int g1s_denoise_motion_time(g1s_denoise_t *, double *ms_motion);
/* Rules 12 and 13: the pair (f, g) for the luma scaling functions of n >= 1 segments of a grain table, range R (0 = the
 * default).  fwd: 1 << bit_depth entries, inv: 4096.  Host only: needs no device.  G1S_ERR_INVALID (reason from
 * g1s_last_global_error()) for bit_depth 12 or any other than 8 and 10, a range above 2^(12 - bit_depth), n = 0, and luma
 * points whose values do not increase. */
int g1s_denoise_curve(const g1s_segment_t *segs, size_t n, uint32_t bit_depth, uint32_t range, uint16_t *fwd, uint16_t *inv);
/* One frame.  in / out follow g1s_frame_t.on_device independently, as in g1s_grain_frame: 0 = host (in: copied before
 * the call returns; out: written by g1s_denoise_sync at the latest), 1 = device, 2 = pinned host (copies queued).  Device
 * and pinned planes of in must stay valid and unmodified, and every plane of out must stay valid, until
 * g1s_denoise_sync.  in and out must be DISTINCT, non-overlapping buffers (a workgroup reads the samples around its
 * tile, which another one would already have replaced).  Same geometry on both sides; a frame whose geometry differs
 * from the one before it ends the clip: what is queued goes out and finishes first.
 * With a temporal radius D > 0 a frame is launched once the D frames after it have been handed over: a full batch goes
 * out without the last D frames, which wait for their neighbours (or the end of the clip).  Frame n, counted since the
 * denoiser was made as g1s_denoise_drain counts, is read by the frames up to n + D: device and pinned planes of in must
 * stay valid and unmodified until frames_complete exceeds n + D, or until g1s_denoise_sync.  Host planes are still copied
 * before the call returns (the denoiser keeps a batch and the 2 D frames around it on the device).  out as above: valid
 * until frames_complete exceeds n, or until g1s_denoise_sync; it must not overlap a plane the queue still reads.
 * Under G1S_DENOISE_JOINT_CHROMA the chroma launch also reads the luma plane of in, which must already stay valid. */
int g1s_denoise_frame(g1s_denoise_t *, const g1s_frame_t *in, g1s_frame_t *out);
/* Launches what is queued and waits: the out planes of every frame handed over are complete.  This ends the clip: with a
 * temporal radius the last D frames go out with the neighbours they have, and the next frame starts a new clip. */
int g1s_denoise_sync(g1s_denoise_t *);
/* Launches every queued frame whose D later neighbours have been handed over, waits, and reports in *frames_complete
 * (may be NULL) how many frames since the denoiser was made have complete out planes.  It does NOT end the clip.  With
 * temporal radius 0 it completes what g1s_denoise_sync completes. */
int g1s_denoise_drain(g1s_denoise_t *, uint64_t *frames_complete);
/* HIP-event time of the kernels so far, milliseconds, and the frames they covered (enable = 1: timed from the next
 * batch on; a timed batch is waited for).  tools/bench_denoise.py. */
int g1s_denoise_set_timing(g1s_denoise_t *, int enable, double *ms_kernel, uint64_t *frames);
const char *g1s_denoise_last_error(const g1s_denoise_t *);
void g1s_denoise_free(g1s_denoise_t *);
/* (q, T) of rule 3 as the kernels use them.  Host only: needs no device.  G1S_ERR_INVALID (reason from
 * g1s_last_global_error()) for a bit depth, patch radius or strength out of range. */
int g1s_denoise_weights(uint32_t bit_depth, uint32_t patch_radius, double strength, uint16_t T[1024], uint32_t *q);
/* The same with flags: rule 10's (q_J, T_J) under G1S_DENOISE_JOINT_CHROMA (strength = the chroma strength), rule 3's
 * without it.  An unknown flag bit is G1S_ERR_INVALID ("unknown denoise flags"). */
int g1s_denoise_weights_ex(uint32_t bit_depth, uint32_t patch_radius, double strength, uint32_t flags, uint16_t T[1024], uint32_t *q);
/* `denoise INPUT -o OUTPUT`: every frame of a .y4m through the filter, written as .y4m (the input's header line,
 * "FRAME\n", the planes without padding).  Returns the number of frames, or a negative G1S_ERR_* with the reason in err. */
int64_t g1s_denoise_y4m_file(const char *in, const char *out, const g1s_denoise_opts_t *opts, char *err, size_t cap);
/* The same with a temporal radius; the whole file is one clip.  g1s_denoise_y4m_file is temporal_radius = 0. */
int64_t g1s_denoise_y4m_file_temporal(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, char *err,
                                      size_t cap);
/* The same with flags (G1S_DENOISE_*); g1s_denoise_y4m_file_temporal is flags = 0. */
int64_t g1s_denoise_y4m_file_ex(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags, char *err,
                                size_t cap);
/* The same with a grain prior (`--grain-prior`): the curve of the table at prior_tbl for the clip's bit depth, range
 * prior_range (0 = the default), from segment prior_segment alone or, when that is negative, from the mean of all of them.
 * A table that does not parse, a segment the table does not have and a 12-bit clip are refusals with their text.
 * prior_tbl == NULL is g1s_denoise_y4m_file_ex. */
int64_t g1s_denoise_y4m_file_curve(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                   const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, char *err, size_t cap);
/* The same with a motion range (rules 16 - 20, as g1s_denoise_new_motion takes it); motion_range = 0 is
 * g1s_denoise_y4m_file_curve. */
int64_t g1s_denoise_y4m_file_motion(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, char *err,
                                    size_t cap);
/* The same with what the clip itself says (noise levels, rules N5 - N7), from a pre-pass over the first profile_frames frames
 * (0 = all) of the file, which is then opened again and filtered as by g1s_denoise_y4m_file_motion.  G1S_AUTO_PRIOR: the curve
 * of rules 12 - 13 from the clip's own levels (N6; prior_range as for a table) instead of a table's; G1S_AUTO_STRENGTH: the
 * strength and the chroma strength from N7 (where N7 refuses for chroma, a luma-only clip, the luma strength).  min_count is
 * N5's and N7's Nmin (0 = 4096).  Refusals, each with its text: an unknown flag bit, G1S_AUTO_PRIOR with prior_tbl,
 * G1S_AUTO_STRENGTH with a non-zero strength or chroma_strength in opts, a source that is not a regular file (a pipe is read
 * once), and what N6 and N7 refuse.  auto_flags = 0 is g1s_denoise_y4m_file_motion. */
#define G1S_AUTO_PRIOR 1u
#define G1S_AUTO_STRENGTH 2u
int64_t g1s_denoise_y4m_file_auto(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                  const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                  uint64_t profile_frames, uint64_t min_count, char *err, size_t cap);
/* The same with the job's prior extended to chroma (rules 21 - 24).  chroma_prior = 0 is g1s_denoise_y4m_file_auto; 1: with
 * prior_tbl the gain of rule 22 on the segments prior_segment selects, with G1S_AUTO_PRIOR the gain of N9 on the pre-pass
 * record that is summed already (no second pass); prior_range serves both, and a range above 8 is refused with rule 21's text
 * though luma at 8 bits takes up to 16.  Refusals: a value other than 0 or 1 ("chroma_prior is 0 or 1"), "a chroma prior needs
 * a grain prior (a table or the clip's own levels)", "a chroma gain needs joint chroma", and what N9 refuses. */
int64_t g1s_denoise_y4m_file_chroma(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                    uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, char *err, size_t cap);
/* The same with coarse levels (rules 25 - 29, as g1s_denoise_new_levels takes them and refuses them); coarse_levels = 0 is
 * g1s_denoise_y4m_file_chroma.  An auto strength is level 0's; the levels scale it. */
int64_t g1s_denoise_y4m_file_levels(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                    const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                    uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio,
                                    char *err, size_t cap);
/* The same with the pre-pass made temporal (rules T1 - T7); auto_temporal = 0 is g1s_denoise_y4m_file_levels: the same
 * launches, the same bytes.  1: the pre-pass meter is a temporal one, and G1S_AUTO_PRIOR, G1S_AUTO_STRENGTH and the chroma
 * prior take T7's values in the place of N6's, N7's and N9's.  Refusals: a value other than 0 or 1 ("auto_temporal is 0 or
 * 1"), 1 without an auto flag ("temporal noise levels need an auto flag (an auto prior or an auto strength)"), a pre-pass of
 * fewer than two frames ("temporal noise levels need two frames").  The bits of auto_flags stay as they are. */
int64_t g1s_denoise_y4m_file_auto_temporal(const char *in, const char *out, const g1s_denoise_opts_t *opts, uint32_t temporal_radius, uint32_t flags,
                                           const char *prior_tbl, uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags,
                                           uint64_t profile_frames, uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio,
                                           uint32_t auto_temporal, char *err, size_t cap);
/* `diff SOURCE --denoise -o OUT`: g1s_diff_y4m_files with the second file made on the device.  The source is read once
 * and copied to the device once; each frame is denoised there and the pair (source, denoised) goes to the generator as
 * device frames, in buffers that are used again once g1s_diff_frames_released() covers their frame.  The denoiser runs
 * on the generator's device (dopts->device is ignored).  keep_denoised != NULL: the denoised clip is also written
 * there as .y4m.  The table is the one g1s_diff_y4m_files makes from SOURCE and that clip. */
int g1s_diff_y4m_file_denoised(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                               const g1s_denoise_opts_t *dopts, uint64_t *frames, char *err, size_t cap);
/* The same with a temporal radius; the whole file is one clip, and a source buffer is used again only when the denoiser
 * is past the D frames after it as well.  g1s_diff_y4m_file_denoised is temporal_radius = 0. */
int g1s_diff_y4m_file_denoised_temporal(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                        const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint64_t *frames, char *err, size_t cap);
/* The same with flags (G1S_DENOISE_*); g1s_diff_y4m_file_denoised_temporal is flags = 0. */
int g1s_diff_y4m_file_denoised_ex(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                  const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, uint64_t *frames, char *err,
                                  size_t cap);
/* The same with a grain prior, as g1s_denoise_y4m_file_curve takes it: typically the table a first `diff SOURCE --denoise`
 * made.  prior_tbl == NULL is g1s_diff_y4m_file_denoised_ex. */
int g1s_diff_y4m_file_denoised_curve(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                     const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                     uint32_t prior_range, int32_t prior_segment, uint64_t *frames, char *err, size_t cap);
/* The same with a motion range; motion_range = 0 is g1s_diff_y4m_file_denoised_curve. */
int g1s_diff_y4m_file_denoised_motion(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint64_t *frames, char *err,
                                      size_t cap);
/* The same with the auto flags of g1s_denoise_y4m_file_auto (the pre-pass runs on the generator's device); auto_flags = 0 is
 * g1s_diff_y4m_file_denoised_motion. */
int g1s_diff_y4m_file_denoised_auto(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                    const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                    uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                    uint64_t min_count, uint64_t *frames, char *err, size_t cap);
/* The same with chroma_prior as g1s_denoise_y4m_file_chroma takes it; chroma_prior = 0 is g1s_diff_y4m_file_denoised_auto.
 * This closes the loop table -> prior -> better table for all three planes. */
int g1s_diff_y4m_file_denoised_chroma(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                      uint64_t min_count, uint32_t chroma_prior, uint64_t *frames, char *err, size_t cap);
/* The same with coarse levels; coarse_levels = 0 is g1s_diff_y4m_file_denoised_chroma.  Their refusals are looked at with the
 * flags', in front of the prior and the device (with the strengths of dopts, 0 = the default; an auto strength's levels are
 * checked when the denoiser is made).  This rung makes the generator, on a device, before the denoiser, so here -- and only
 * here -- they also come in front of the denoiser's older parameter refusals (search_radius, patch_radius, motion_range, the
 * strengths), which g1s_denoise_new_levels and g1s_denoise_y4m_file_levels name first; a strength that rule 3 refuses, or opts
 * of another size, is left to the constructor and the levels are looked at over the default strengths. */
int g1s_diff_y4m_file_denoised_levels(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                      const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                      uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                      uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio, uint64_t *frames, char *err,
                                      size_t cap);
/* The same with auto_temporal as g1s_denoise_y4m_file_auto_temporal takes and refuses it; 0 is
 * g1s_diff_y4m_file_denoised_levels. */
int g1s_diff_y4m_file_denoised_auto_temporal(const char *source, const char *out_tbl, const char *keep_denoised, const g1s_opts_t *opts,
                                             const g1s_denoise_opts_t *dopts, uint32_t temporal_radius, uint32_t flags, const char *prior_tbl,
                                             uint32_t prior_range, int32_t prior_segment, uint32_t motion_range, uint32_t auto_flags, uint64_t profile_frames,
                                             uint64_t min_count, uint32_t chroma_prior, uint32_t coarse_levels, double coarse_ratio, uint32_t auto_temporal,
                                             uint64_t *frames, char *err, size_t cap);

/* ---- `measure` and `check`: exact grain statistics of a frame pair (how well a table fits) ----
 * An AV1 grain table says how strong the grain is as a function of intensity and how it is correlated over the causal
 * lag-3 neighbourhood.  `measure` takes those two things of a residual noisy - clean, whole-plane, at full bit depth,
 * in exact integers; `check` takes them twice, of source - denoised and of render(denoised, table) - denoised.
 * Two frames of one geometry and one bit depth B in {8, 10, 12}: a (noisy) and b (clean), luma only or three planes
 * (xdec <= 1, ydec <= xdec).  For every plane c of size pw x ph:
 *   1. d(p) = a(p) - b(p), signed, |d| < 2^B.  A sample above the bit depth's maximum is the caller's error.
 *   2. The intensity I(p): for luma b_Y(p); for chroma the specification's averageLuma of the CLEAN frame: with
 *      ys = y << ydec, xs = x << xdec: (b_Y(xs, ys) + b_Y(min(xs + 1, W - 1), ys) + 1) >> 1 if xdec, else b_Y(xs, ys).
 *      The bin is k(p) = I(p) >> (B - 5): 32 bins.
 *   3. Per bin k, over all p of the plane with k(p) = k: n[k] the count (u64), s1[k] = sum of d (i64), s2[k] = sum of
 *      d^2 (u64).
 *   4. Lagged products over 25 offsets (dx, dy): the first 24 are the lag-3 causal neighbourhood in the table's
 *      coefficient order (dy = -3 .. 0, dx = -3 .. 3, raster, stopping before (0, 0)); (0, 0) is index 24.
 *      r[i] = sum of d(p) d(p + delta_i) (i64) over every p for which p AND p + delta_i lie inside the plane: skipped,
 *      not clamped.  The number of terms is (pw - |dx|)(ph - |dy|), or 0 where that is not positive; it is not stored.
 *   5. A frame's record is the three planes' {n[32], s1[32], s2[32], r[25]}, zeros for the planes the frame does not
 *      have.  Everything is exact: s2 <= 2^24 2^32 for the largest frame the checks admit (65536 x 65536).
 *   6. A clip's record is the sum of its frames' records, formed on the host with checked 64-bit additions
 *      (g1s_measure_sum): an overflow is a refusal, not a wrap.
 * A temporal meter (g1s_measure_new_temporal) also says whether the residual is independent from frame to frame, as grain
 * is and picture detail a denoiser removed is not.  A RUN is the sequence of pairs given one after another to one temporal
 * meter with one geometry; a change of geometry or g1s_measure_cut ends it.  Pair t of a run, t >= 1, has a TEMPORAL RECORD
 * against pair t - 1; d_t and d_{t-1} are rule 1 of their own pairs.  For every plane c:
 *   7. Bins.  k(p) is rule 2 on the clean frame of pair t.  Per bin k, over the p of the plane with k(p) = k: n[k] the
 *      count (u64), x[k] = sum of d_t(p) d_{t-1}(p) (i64), u[k] = sum of d_t(p)^2 (u64), v[k] = sum of d_{t-1}(p)^2 (u64).
 *      So n and u equal the n and s2 of pair t's own record.
 *   8. Offsets.  25 offsets dy = -2 .. 2, dx = -2 .. 2 in raster order: index i = (dy + 2) 5 + (dx + 2), (0, 0) is index
 *      12.  The window is not causal: across frames both signs mean something.  c[i] = sum of d_t(p) d_{t-1}(p + delta_i)
 *      (i64) over every p for which p AND p + delta_i lie inside the plane: skipped, not clamped.  The number of terms is
 *      (pw - |dx|)(ph - |dy|), or 0 where that is not positive.
 *   9. Record.  g1s_measure_trecord_t, zeros for the planes the frame does not have.  Everything is exact within rule 5's
 *      bounds.
 *  10. Sum.  A clip's temporal record is the checked 64-bit sum of its pairs' temporal records
 *      (g1s_measure_sum_temporal): an overflow is a refusal.
 *  11. Report.  g1s_format_measure_temporal writes plain text; the grammar is at its declaration.
 * A cross meter (g1s_measure_new_modes with G1S_MEASURE_CROSS) also looks across the planes: how much of the chroma residual
 * is the luma residual at the same place -- the last AR coefficient of each chroma plane of a table, the one field rules 1 - 11
 * are blind to -- and whether Cb and Cr are correlated beyond what the shared luma explains.  For a pair with three planes,
 * luma W x H, chroma cw x ch (cw = (W + xdec) >> xdec, ch = (H + ydec) >> ydec), d_Y, d_Cb, d_Cr as in rule 1:
 *  12. The luma residual at chroma resolution.  L(x, y) = Round2(S, xdec + ydec), S the sum over i <= ydec, j <= xdec of
 *      d_Y(min((x << xdec) + j, W - 1), min((y << ydec) + i, H - 1)); Round2(v, s) = (v + ((1 << s) >> 1)) >> s with an
 *      ARITHMETIC shift: it rounds towards minus infinity, also for negative sums.  For 4:4:4, L = d_Y.  This is the
 *      specification's own box and rounding for the luma grain under a chroma sample (7.18.3.3), with the clamp of rule 8 of
 *      `denoise`.  |L| <= 2^B - 1: L is as wide as a residual.  The rounded mean and not the sum, for two reasons: it is what
 *      the synthesis multiplies the coefficient by, so a slope on L is a number in the table's own units; and it keeps every
 *      product below 2^24, so that the 32-bit schedule of the temporal kernel holds unchanged.
 *  13. Three pairings (a_j, b_j) on the chroma grid: j = 0: (d_Cb, L); j = 1: (d_Cr, L); j = 2: (d_Cb, d_Cr).
 *  14. Bins.  k(p) is rule 2's chroma bin (averageLuma of the clean frame), the same for all three pairings.  Per pairing and
 *      bin: n[k] the count (u64), x[k] = sum of a b (i64), u[k] = sum of a^2 (u64), v[k] = sum of b^2 (u64).
 *  15. Offsets.  Rule 8's 25 offsets (dy, dx = -2 .. 2 in raster order, (0, 0) at index 12).  c[i] = sum of a(p) b(p + delta_i)
 *      (i64) over every p for which p AND p + delta_i lie inside the chroma plane: skipped, not clamped.  L is a cw x ch plane
 *      like any other: the clamp of rule 12 is inside L, and nothing outside the chroma grid takes part.
 *  16. Record.  g1s_measure_xrecord_t is g1s_measure_trecord_t with the pairing where the plane is.  All zeros for a pair with
 *      one plane.  EVERY pair has a cross record: no predecessor is needed.  A clip's record is the checked 64-bit sum
 *      (g1s_measure_sum_cross).  Everything is exact within rule 5's bounds.
 *  17. Report.  g1s_format_measure_cross writes plain text; the grammar is at its declaration.
 * A scales meter (g1s_measure_new_scales) also looks further than 3 samples: how the variance of the residual summed over
 * 2^k x 2^k boxes grows with k.  White grain grows by 4^k; grain with a correlation length grows faster and then runs
 * parallel to 4^k; a residual whose low frequencies a denoiser kept grows slower.  For a pair as in rules 1 - 2, every plane
 * c of size pw x ph and every scale k = 1 .. 5 with L = 2^k:
 *  18. Boxes.  Boxes are aligned at the plane's origin: box (i, j) holds x in [iL, iL + L), y in [jL, jL + L), for
 *      i < pw >> k and j < ph >> k.  A box that is not whole is skipped, not clamped; a plane narrower or lower than L has
 *      no boxes at that scale.
 *  19. Box sum and box bin.  B = the sum over the box of d(p) of rule 1: |B| <= 4^k (2^B - 1) < 2^22.  C = the sum over the
 *      box of I(p), rule 2's intensity of each sample as it stands: for chroma the per-sample averageLuma with its own
 *      + 1 >> 1, then summed -- not a sum of luma samples.  The bin is K = min(C >> (2k + B - 5), 31): the floor of the box
 *      mean's bin.  There is no rounding: a box of three samples on a bin's lower edge and one sample one below it lies in
 *      the lower bin.
 *  20. Sums.  Per plane, scale and bin, over the boxes with that K: n the count (u64), s1 = sum of B (i64), s2 = sum of
 *      B^2 (u64), every square formed in 64 bits.
 *  21. Record and bound.  g1s_measure_srecord_t, 11 520 bytes; scale index 0 is k = 1; zeros for the planes the frame does
 *      not have.  s2 <= 4^k (2^B - 1)^2 pw ph, which at k = 5 stays below 2^64 for every plane the checks admit but a 12-bit
 *      plane of more than 2^30 samples: on a scales meter such a pair is refused from its geometry alone, before any sample
 *      is read (G1S_ERR_INVALID, "a scales meter takes 12-bit planes of at most 2^30 samples", sticky like the meter's other
 *      geometry refusals).  Scale 0 is not stored: it is the plain record.
 *  22. Sum.  A clip's scale record is the checked 64-bit sum of its pairs' records (g1s_measure_sum_scales): an overflow is
 *      a refusal, not a wrap.
 *  23. Report.  g1s_format_measure_scales writes plain text; the grammar is at its declaration.
 * Frames queue up to batch_frames (0 = 32; at most 256) and go out as one kernel launch per plane class (luma; the two
 * chroma planes) and a small summing launch, on the meter's own stream.  Errors are sticky (g1s_measure_last_error). */
typedef struct {
  uint64_t n[3][32];
  int64_t s1[3][32];
  uint64_t s2[3][32];
  int64_t r[3][25];
} g1s_measure_record_t;
typedef struct {
  uint32_t struct_size; /* sizeof(g1s_measure_opts_t) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  uint32_t batch_frames;
} g1s_measure_opts_t;
typedef struct g1s_measure g1s_measure_t;
/* bit_depth 8, 10 or 12.  NULL on failure, the reason from g1s_last_global_error() ("no HIP device available: measure
 * has no CPU fallback" without a device).  opts == NULL: current device, defaults. */
g1s_measure_t *g1s_measure_new(uint32_t bit_depth, const g1s_measure_opts_t *opts);
/* One frame pair; both are only read.  Each follows g1s_frame_t.on_device on its own: 0 = host (copied before the call
 * returns), 1 = device, 2 = pinned host (the copy is queued).  Device and pinned planes must stay valid and unmodified
 * until the batch they are in has gone out: batch_frames pairs later, or at g1s_measure_finish.  A pair whose geometry
 * differs from the one before it sends the queued pairs out first. */
int g1s_measure_frame(g1s_measure_t *, const g1s_frame_t *noisy, const g1s_frame_t *clean);
/* Launches what is queued, waits, and hands over one record per pair since the last hand-over, in order.  cap too
 * small (or per_frame NULL): G1S_ERR_CAPACITY, *n_out = the count, the records stay (the error is not sticky).  After
 * G1S_OK the meter holds no records; more pairs may follow. */
int g1s_measure_finish(g1s_measure_t *, g1s_measure_record_t *per_frame, size_t cap, size_t *n_out);
/* Rule 6 (host only, needs no device): *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_measure_sum(const g1s_measure_record_t *recs, size_t n, g1s_measure_record_t *total);
/* The report (host only): plain text from a clip's record of `frames` frames of one geometry.  synth == NULL: one value
 * column; else two (total = source - denoised, synth = rendered - denoised) and two summary lines a plane.  Every value is
 * formed in f64 from the exact integers and printed "%.4f"; "-" where it is undefined.  Grammar:
 *   grainprofile1
 *   frames N bit_depth B planes P
 *   plane c                                      for c in 0 .. P - 1
 *   bin k n mean sigma [mean' sigma']            the bins with n > 0 (n is total's): mean = s1 / n,
 *                                                sigma = sqrt(max(s2 / n - mean mean, 0))
 *   lag dx dy rho [rho']                         the 24 lags: rho = (r[i] / terms_i) / (r[24] / terms_24), terms_i =
 *                                                frames (pw - |dx|)(ph - |dy|); "-" when r[24] = 0 or terms_i = 0
 *   max_rho_diff v                               (two columns) the largest |rho' - rho| over the lags where both exist
 *   sigma_ratio v                                (two columns) the n-weighted mean of sigma' / sigma over the bins where
 *                                                both are positive
 * Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a geometry rule 5 does not have). */
long g1s_format_measure(const g1s_measure_record_t *total, const g1s_measure_record_t *synth, uint64_t frames, uint32_t bit_depth,
                        uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap);
/* HIP-event time of the kernels so far, milliseconds, and the frames they covered (enable = 1: timed from the next
 * batch on).  tools/bench_measure.py. */
int g1s_measure_set_timing(g1s_measure_t *, int enable, double *ms_kernel, uint64_t *frames);
const char *g1s_measure_last_error(const g1s_measure_t *);
void g1s_measure_free(g1s_measure_t *);
/* `measure NOISY CLEAN -o REPORT` for two .y4m files of one geometry and bit depth: the frame pairs until the shorter
 * file ends (*unequal = 1 when only one ended), the clip's record, the report.  Returns the number of frames, or a
 * negative G1S_ERR_* with the reason in err. */
int64_t g1s_measure_y4m_files(const char *noisy, const char *clean, const char *out_report, const g1s_measure_opts_t *opts, int *unequal,
                              char *err, size_t cap);
/* `check SOURCE DENOISED -g TABLE -o REPORT`: per frame k the table's lookup as g1s_grain_y4m_file makes it, the grain
 * rendered onto the denoised frame into a device buffer, then measure(source, denoised) and measure(rendered,
 * denoised): the denoised frame is uploaded once and the rendered frame never leaves the device.  A frame no segment
 * covers is measured with rendered = denoised.  The two-column report; no verdict.  gopts->device is ignored (one
 * device: opts->device).  Returns as g1s_measure_y4m_files. */
int64_t g1s_check_y4m_files(const char *source, const char *denoised, const char *tbl, const char *out_report, const g1s_measure_opts_t *opts,
                            const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap);

/* -- the temporal meter (rules 7 - 11 above) -- */
typedef struct {
  uint64_t n[3][32];
  int64_t x[3][32];
  uint64_t u[3][32];
  uint64_t v[3][32];
  int64_t c[3][25];
} g1s_measure_trecord_t;
/* A meter in temporal mode: g1s_measure_new with the same refusals.  g1s_measure_frame and g1s_measure_finish do on it
 * what they do on a plain meter (the ordinary records are the same); from the second pair of a run on, g1s_measure_frame
 * also queues the temporal job against the pair before.  Lifetime on a temporal meter: device and pinned planes of a pair
 * must stay valid and unmodified until the batch that holds the NEXT pair has gone out, or until g1s_measure_cut,
 * g1s_measure_finish or g1s_measure_finish_temporal (which keep a device copy of the run's last pair).  Host frames go
 * into rings of batch_frames + 1 slots, so that the pair before a batch's first pair is still there: no pair is
 * uploaded twice. */
g1s_measure_t *g1s_measure_new_temporal(uint32_t bit_depth, const g1s_measure_opts_t *opts);
/* Ends the run: what is queued goes out, and the next pair has no temporal record.  Scene cuts are the caller's knowledge
 * (the .y4m commands never call this).  On a plain meter: G1S_ERR_INVALID, the text names g1s_measure_new_temporal; not
 * sticky, the meter goes on working. */
int g1s_measure_cut(g1s_measure_t *);
/* As g1s_measure_finish, for the temporal records: one per pair that has a predecessor in its run, in order, since the last
 * hand-over.  G1S_ERR_CAPACITY is not sticky and the records stay.  g1s_measure_finish and g1s_measure_finish_temporal each
 * flush; each keeps the other's records until they are fetched.  On a plain meter as g1s_measure_cut. */
int g1s_measure_finish_temporal(g1s_measure_t *, g1s_measure_trecord_t *per_pair, size_t cap, size_t *n_out);
/* Rule 10 (host only, needs no device): *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_measure_sum_temporal(const g1s_measure_trecord_t *recs, size_t n, g1s_measure_trecord_t *total);
/* Rule 11 (host only): plain text from a clip's temporal record of `pairs` records of one geometry.  synth == NULL: one
 * value column; else two (total = source - denoised, synth = rendered - denoised).  Every value is formed in f64 from the
 * exact integers in exactly the order written here, without fused multiply-add, and printed "%.4f"; "-" where undefined.
 *   graintemporal1
 *   pairs N bit_depth B planes P
 *   plane c                          for c in 0 .. P - 1; with pairs = 0 nothing stands under it (a clip of one frame)
 *   bin k n rho [rho']               the bins with n > 0 (n is total's): rho = (double)x / sqrt((double)u * (double)v);
 *                                    "-" when u == 0 or v == 0
 *   lag dx dy rho [rho']             the 25 lags in index order: rho = ((double)c[i] / terms_i) / sqrt(((double)U / T) *
 *                                    ((double)V / T)), U = sum of u[k], V = sum of v[k] (u64 sums), T = pairs pw ph,
 *                                    terms_i = pairs (pw - |dx|)(ph - |dy|); "-" when U == 0, V == 0 or terms_i == 0
 *   temporal_rho v [v']              the (0, 0) lag
 *   peak_rho dx dy v [dx' dy' v']    the lag of largest |rho|, the first in index order on ties; "- - -" when no lag is
 *                                    defined
 * There is no verdict.  Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a geometry rule 5 does not have). */
long g1s_format_measure_temporal(const g1s_measure_trecord_t *total, const g1s_measure_trecord_t *synth, uint64_t pairs, uint32_t bit_depth,
                                 uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, uint32_t nplanes, char *buf, size_t cap);
/* HIP-event time of km_measure_t and km_tail_t in the batches g1s_measure_set_timing had timed, milliseconds, and the
 * temporal records they made.  tools/bench_measure.py --temporal. */
int g1s_measure_temporal_timing(g1s_measure_t *, double *ms_kernel, uint64_t *pairs);
/* g1s_measure_y4m_files that also writes the clip's temporal report to out_treport (one run: frames - 1 records).
 * out_treport == NULL is exactly g1s_measure_y4m_files. */
int64_t g1s_measure_y4m_files_temporal(const char *noisy, const char *clean, const char *out_report, const char *out_treport,
                                       const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap);
/* g1s_check_y4m_files that also writes the two-column temporal report to out_treport: total = source - denoised, synth =
 * rendered - denoised.  The previous rendered and the previous denoised frame stay on the device for one more frame:
 * nothing extra crosses PCIe.  out_treport == NULL is exactly g1s_check_y4m_files. */
int64_t g1s_check_y4m_files_temporal(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                     const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err, size_t cap);

/* -- the cross meter (rules 12 - 17 above) -- */
#define G1S_MEASURE_TEMPORAL 1u
#define G1S_MEASURE_CROSS 2u
/* the temporal record's layout with the pairing where the plane is: n[3][32], x[3][32], u[3][32], v[3][32], c[3][25] */
typedef g1s_measure_trecord_t g1s_measure_xrecord_t;
/* A meter with the modes asked for (G1S_MEASURE_*, or'ed): g1s_measure_new is modes 0, g1s_measure_new_temporal is modes 1.
 * An unknown bit is refused (NULL, the reason from g1s_last_global_error()) before anything else is looked at, a device
 * included.  g1s_measure_opts_t is not extended.  A meter launches only what its modes ask for: with G1S_MEASURE_CROSS one
 * km_measure_x launch and one summing launch a batch, behind the ordinary ones on the meter's stream.  A cross job reads only
 * the planes of its own pair: the lifetime rules of a plain meter stand for modes 2, those of a temporal meter for modes 3. */
g1s_measure_t *g1s_measure_new_modes(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes);
/* As g1s_measure_finish_temporal, for the cross records: one per pair since the last hand-over, in order (zeros for a pair
 * with one plane).  G1S_ERR_CAPACITY is not sticky and the records stay.  Each of the three finish calls flushes; each keeps
 * the others' records until they are fetched.  On a meter without G1S_MEASURE_CROSS: G1S_ERR_INVALID, the text names
 * g1s_measure_new_modes; not sticky, the meter goes on working. */
int g1s_measure_finish_cross(g1s_measure_t *, g1s_measure_xrecord_t *per_pair, size_t cap, size_t *n_out);
/* Rule 16 (host only, needs no device): *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_measure_sum_cross(const g1s_measure_xrecord_t *recs, size_t n, g1s_measure_xrecord_t *total);
/* Rule 17 (host only): plain text from a clip's cross record of `frames` records of one three-plane geometry.  synth == NULL:
 * one value column; else two (total = source - denoised, synth = rendered - denoised).  Every value is formed in f64 from the
 * exact integers in exactly the order written here, without fused multiply-add, and printed "%.4f"; "-" where undefined.
 *   graincross1
 *   frames N bit_depth B
 *   pairing cb_luma                  then cr_luma, then cb_cr; with frames = 0 nothing stands under it
 *   bin k n rho beta [rho' beta']    the bins with n > 0 (n is total's): rho = (double)x / sqrt((double)u * (double)v), "-" when
 *                                    u == 0 or v == 0; beta = (double)x / (double)v, "-" when v == 0
 *   lag dx dy rho [rho']             the 25 lags in index order: rho = ((double)c[i] / terms_i) / sqrt(((double)U / T) *
 *                                    ((double)V / T)), U = sum of u[k], V = sum of v[k] (u64 sums), T = frames cw ch,
 *                                    terms_i = frames (cw - |dx|)(ch - |dy|); "-" when U == 0, V == 0 or terms_i == 0
 *   zero_rho v [v']                  the (0, 0) lag
 *   peak_rho dx dy v [dx' dy' v']    the lag of largest |rho|, the first in index order on ties; "- - -" when none is defined
 *   beta v [v']                      (double)c[12] / (double)V; "-" when V == 0
 *   partial_rho v [v']               after the third pairing only (and not with frames = 0): with r0, r1, r2 the three
 *                                    zero_rho of the column, f0 = 1 - r0 * r0, f1 = 1 - r1 * r1:
 *                                    (r2 - r0 * r1) / sqrt(f0 * f1); "-" when one of r0, r1, r2 is undefined or f0 <= 0 or f1 <= 0
 * What the numbers mean: rho is a correlation coefficient about zero (grain has no mean).  beta of a luma pairing is the
 * least-squares slope of the chroma residual on L alone: for a table whose chroma AR part is zero it is the table's last
 * chroma coefficient over 2^ar_coeff_shift; with a chroma AR part it is larger, because the filter feeds the luma term back
 * through the chroma neighbours.  So beta is not the coefficient: `check` puts the same number of the rendered grain beside
 * it, and that comparison is the one that counts.  A peak_rho of a luma pairing away from (0, 0) is what a chroma siting error
 * looks like.  beta of cb_cr is the slope of d_Cb on d_Cr; partial_rho is the correlation of Cb and Cr that the shared luma
 * does not explain: the AV1 model cannot express one, so away from zero it means picture detail was removed.  There is no
 * verdict and no threshold.  Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for a geometry rule 5 does not have). */
long g1s_format_measure_cross(const g1s_measure_xrecord_t *total, const g1s_measure_xrecord_t *synth, uint64_t frames, uint32_t bit_depth,
                              uint32_t width, uint32_t height, uint32_t xdec, uint32_t ydec, char *buf, size_t cap);
/* HIP-event time of km_measure_x and its summing launch in the batches g1s_measure_set_timing had timed, milliseconds, and
 * the cross records they made.  tools/bench_measure.py --cross. */
int g1s_measure_cross_timing(g1s_measure_t *, double *ms_kernel, uint64_t *pairs);
/* HIP-event time of the chroma launches alone in the timed batches: km_measure's and, on a temporal meter, km_measure_t's (the
 * yardstick of km_measure_x).  The events are recorded only while timing is on.  tools/bench_measure.py --cross. */
int g1s_measure_chroma_timing(g1s_measure_t *, double *ms_chroma, double *ms_temporal_chroma);
/* g1s_measure_y4m_files_temporal that also writes the clip's cross report to out_xreport (one record a frame).  A clip without
 * chroma planes is refused with out_xreport set ("--cross compares chroma with luma: the clip has no chroma planes") before a
 * device is looked for or an output is opened.  out_xreport == NULL is exactly g1s_measure_y4m_files_temporal. */
int64_t g1s_measure_y4m_files_modes(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                    const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap);
/* g1s_check_y4m_files_temporal that also writes the two-column cross report: total = source - denoised, synth = rendered -
 * denoised, whose L comes from rendered_Y - denoised_Y.  Nothing extra crosses PCIe and the rendered frame stays on the
 * device.  out_xreport == NULL is exactly g1s_check_y4m_files_temporal. */
int64_t g1s_check_y4m_files_modes(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                  const char *out_xreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts, int *unequal, char *err,
                                  size_t cap);

/* -- the scales meter (rules 18 - 23 above) -- */
typedef struct {
  uint64_t n[3][5][32]; /* [plane][k - 1][bin] */
  int64_t s1[3][5][32];
  uint64_t s2[3][5][32];
} g1s_measure_srecord_t;
/* g1s_measure_new_modes(bit_depth, opts, modes) with the same refusals in the same order (bit 4 and above are unknown mode
 * bits here too), plus the scale record for every pair: one km_measure_s launch a plane class and one summing launch a batch,
 * behind the meter's other launches on its stream.  g1s_measure_opts_t is not extended.  A scale job reads only the planes of
 * its own pair: the lifetime rules are those of the meter's modes.  A pair with a 12-bit plane of more than 2^30 samples is
 * refused (rule 21).  A meter not made by this call launches what it launched and returns the bytes it returned. */
g1s_measure_t *g1s_measure_new_scales(uint32_t bit_depth, const g1s_measure_opts_t *opts, uint32_t modes);
/* As g1s_measure_finish_cross, for the scale records: one per pair since the last hand-over, in order.  G1S_ERR_CAPACITY is
 * not sticky and the records stay.  Each of the four finish calls flushes; each keeps the others' records until they are
 * fetched.  On a meter not made by g1s_measure_new_scales: G1S_ERR_INVALID, the text names g1s_measure_new_scales; not
 * sticky, the meter goes on working. */
int g1s_measure_finish_scales(g1s_measure_t *, g1s_measure_srecord_t *per_pair, size_t cap, size_t *n_out);
/* Rule 22 (host only, needs no device): *total = the sum of recs[0 .. n).  G1S_ERR_INVALID when a sum leaves 64 bits. */
int g1s_measure_sum_scales(const g1s_measure_srecord_t *recs, size_t n, g1s_measure_srecord_t *total);
/* Rule 23 (host only): plain text from a clip's PLAIN record `total` (rule 6) and its SCALE record `stotal` of `frames`
 * frames.  synth == NULL and ssynth == NULL: one value column; both given: two (total = source - denoised, synth =
 * rendered - denoised); one of them alone is G1S_ERR_INVALID.  Every value is formed in f64 from the exact integers in
 * exactly the order written here, without fused multiply-add, and printed "%.4f"; "-" where undefined.
 *   grainscales1
 *   frames N bit_depth B planes P
 *   plane c                                   for c in 0 .. P - 1; with frames = 0 nothing stands under it
 *   scale k boxes m sigma gain [sigma' gain'] k = 1 .. 5; m = the u64 sum over the bins of n[k] (total's);
 *                                             sigma = sqrt(max(V_k, 0)) / 2^k, "-" when the column's own m = 0;
 *                                             gain = V_k / (4^k * V_0), "-" when the column's m = 0, its m_0 = 0 or V_0 <= 0
 *   sbin k j n sigma [sigma']                 after the five scale lines, k = 1 .. 5 and within k the bins j with n > 0 (n is
 *                                             total's): mean = (double)s1 / (double)n, sigma = sqrt(max((double)s2 / (double)n -
 *                                             mean * mean, 0)) / 2^k; sigma' is "-" where the second column's n is 0
 *   gain_ratio k v                            (two columns) after the sbin lines, k = 1 .. 5: gain' / gain, "-" unless both
 *                                             exist and gain > 0
 * The pooled variance: V_k = S / (double)m, S the sum in bin order over the bins j with n_j > 0 of
 * (double)s2_j - ((double)s1_j * (double)s1_j) / (double)n_j: the WITHIN-bin variance, so that a bias that differs from bin to
 * bin does not read as coarse grain.  V_0 and m_0 are the same expressions over n, s1, s2 of the plane in the plain record.
 * What the numbers mean: sigma is the per-sample-equivalent size of the grain at that scale; white grain reads the same at
 * every scale and its gain is 1.  Correlated grain has a gain above 1 that levels off once the box is wider than the
 * correlation (a 3 x 3 box filter of white noise: ((9 L - 8) / (3 L))^2 -- 2.78, 5.44, 7.11, 8.03, 8.51).  A gain that is still
 * rising at k = 4 and 5 where the rendered column has levelled off is grain coarser than a lag-3 table can say: measure at a
 * lower resolution.  A gain below the rendered column's, most at small k, is a denoiser that kept the coarse part of the grain
 * in its "clean" frame.  The rendered column's largest scales are statistics of ONE usable 64 x 64 template a frame -- a luma
 * box at k = 5 is exactly one grain block -- so that column needs a clip, not a frame, to settle.  There is no verdict and no
 * threshold.  Bytes written, or G1S_ERR_CAPACITY (G1S_ERR_INVALID for nplanes other than 1 and 3). */
long g1s_format_measure_scales(const g1s_measure_record_t *total, const g1s_measure_srecord_t *stotal, const g1s_measure_record_t *synth,
                               const g1s_measure_srecord_t *ssynth, uint64_t frames, uint32_t bit_depth, uint32_t nplanes, char *buf, size_t cap);
/* HIP-event time of km_measure_s and its summing launch in the batches g1s_measure_set_timing had timed, milliseconds, and
 * the scale records they made.  tools/bench_measure.py --scales. */
int g1s_measure_scales_timing(g1s_measure_t *, double *ms_kernel, uint64_t *pairs);
/* g1s_measure_y4m_files_modes that also writes the clip's scale report to out_sreport (one record a frame).
 * out_sreport == NULL is exactly g1s_measure_y4m_files_modes. */
int64_t g1s_measure_y4m_files_scales(const char *noisy, const char *clean, const char *out_report, const char *out_treport, const char *out_xreport,
                                     const char *out_sreport, const g1s_measure_opts_t *opts, int *unequal, char *err, size_t cap);
/* g1s_check_y4m_files_modes that also writes the two-column scale report: total = source - denoised, synth = rendered -
 * denoised.  Nothing extra crosses PCIe and the rendered frame stays on the device.  out_sreport == NULL is exactly
 * g1s_check_y4m_files_modes. */
int64_t g1s_check_y4m_files_scales(const char *source, const char *denoised, const char *tbl, const char *out_report, const char *out_treport,
                                   const char *out_xreport, const char *out_sreport, const g1s_measure_opts_t *opts, const g1s_grain_opts_t *gopts,
                                   int *unequal, char *err, size_t cap);

/* ---- decoder surfaces: NV12, P010 / P012 / P016 and MSB-aligned planes, to and from g1s_frame_t on the device ----
 * A hardware decoder (and an encoder on the same device) does not hold planar frames with the sample in the low bits: it
 * holds SEMI-PLANAR surfaces, one luma plane and one plane of interleaved Cb, Cr pairs, and above 8 bits the sample sits in
 * the HIGH bits of its little-endian 16-bit word.  A converter turns such a surface into the g1s_frame_t every operation
 * here takes (unpack) and a frame into such a surface (pack): a permutation and a shift of integers, exact.
 *   1. Chroma size.  Chroma is cw = (width + xdec) >> xdec by ch = (height + ydec) >> ydec samples.  A row of the
 *      interleaved plane holds 2 cw samples: Cb[0], Cr[0], Cb[1], Cr[1], ...; its stride must hold 2 cw bytes_per_sample
 *      bytes.
 *   2. Shift.  sh = msb_aligned ? 16 - bit_depth : 0.
 *   3. Unpack (surface to frame): frame = word >> sh.  The low sh bits of a word are ignored, whatever they hold.  With
 *      sh == 0 a word is copied as it is, and nothing is masked.
 *   4. Pack (frame to surface): word = (sample << sh) & 0xffff.  The low sh bits are written as zeros.
 *   5. Untouched bytes.  No byte outside the rows' samples is written, in either direction: not the pitch's padding and
 *      not the margin.
 *   6. No overlap.  in and out must not overlap.
 *   nplanes  msb_aligned  layouts
 *      2         0        NV12 / NV16 / NV24 (8-bit)
 *      2         1        P010 / P012 / P016, P210 / P216, P410 / P416
 *      3         1        planar MSB-aligned 16-bit 4:4:4 and its relatives
 *      1       0 or 1     monochrome, either alignment
 *   (nplanes 3 with msb_aligned 0 is a plain copy and is accepted.)
 * Frames queue up to batch_frames (0 = 32; at most 256) and go out as one kernel launch per batch on the converter's own
 * stream: a frame goes to another operation only after g1s_surface_sync.  Errors are sticky (g1s_surface_last_error). */
typedef struct {
  uint32_t width, height;      /* luma size in samples */
  uint8_t  bytes_per_sample;   /* 1 or 2 */
  uint8_t  xdec, ydec;         /* as g1s_frame_t */
  uint8_t  nplanes;            /* 1: luma only; 2: luma + one plane of interleaved Cb,Cr pairs; 3: planar */
  uint8_t  bit_depth;          /* 8..16; must be the converter's */
  uint8_t  msb_aligned;        /* 1: a sample sits in the HIGH bit_depth bits of its 16-bit word (bytes_per_sample 2 only) */
  const void *data[3];         /* nplanes == 2: data[1] is the CbCr plane, data[2] is ignored */
  size_t   stride_bytes[3];
  int32_t  on_device;          /* as g1s_frame_t: 0 host, 1 device, 2 pinned host */
} g1s_surface_t;
typedef struct {
  uint32_t struct_size; /* sizeof(g1s_surface_opts_t) */
  int32_t device;       /* HIP device ordinal; -1 = current device */
  uint32_t batch_frames;
} g1s_surface_opts_t;
typedef struct g1s_surface_conv g1s_surface_conv_t;
/* bit_depth 8 .. 16 (8: one-byte samples; above: two-byte).  NULL on failure, the reason from g1s_last_global_error().
 * opts == NULL: current device, defaults. */
g1s_surface_conv_t *g1s_surface_new(uint32_t bit_depth, const g1s_surface_opts_t *opts);
/* One surface into one frame (rule 3) / one frame into one surface (rule 4).  in / out follow on_device independently, as
 * in g1s_grain_frame: 0 = host (in: copied before the call returns; out: written by g1s_surface_sync at the latest),
 * 1 = device, 2 = pinned host (copies queued).  Device and pinned planes of in must stay valid and unmodified, and every
 * plane of out must stay valid, until g1s_surface_sync.  in and out have the same geometry, and their nplanes
 * correspond: 1 and 1; 2 or 3 on the surface and 3 on the frame.  One converter may mix the two calls and mix layouts: a
 * call whose direction, geometry or layout differs from the one before it drains the queue first (the host planes of
 * queued out frames are then complete).  Refused with G1S_ERR_INVALID (G1S_ERR_DIM_MISMATCH where in and out differ in
 * geometry or their nplanes do not correspond): bytes_per_sample or bit_depth that are not the converter's; msb_aligned
 * with one-byte samples; a frame of 2 planes; width or height 0 or above 65536; xdec > 1 or ydec > xdec; a null plane;
 * a stride that does not hold the row (rule 1), is above 0xffffffff or, for 16-bit samples, is odd; overlapping in
 * and out (rule 6). */
int g1s_surface_unpack(g1s_surface_conv_t *, const g1s_surface_t *in, g1s_frame_t *out);
int g1s_surface_pack(g1s_surface_conv_t *, const g1s_frame_t *in, g1s_surface_t *out);
/* Launches what is queued and waits: the out planes of every call so far are complete. */
int g1s_surface_sync(g1s_surface_conv_t *);
/* HIP-event time of the kernels so far, milliseconds, and the frames they covered (enable = 1: timed from the next
 * batch on; a timed batch is waited for).  tools/bench_surface.py. */
int g1s_surface_set_timing(g1s_surface_conv_t *, int enable, double *ms, uint64_t *frames);
const char *g1s_surface_last_error(const g1s_surface_conv_t *);
void g1s_surface_free(g1s_surface_conv_t *);

#ifdef __cplusplus
}
#endif
#endif /* G1S_DIFF_H */
